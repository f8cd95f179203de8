"""Timing of the trimmed refit against a prepared model: one JSON line.

scripts/refit_bench.py's shape and candidates: a 50 k crop against 1 M model rows (bench.synth), B = 107 candidate transforms at
r = 1.5.  Timed, alternately in one process after warm-up, with a host clock around a stream synchronise:
  refit      PreparedModel.refit_transforms, one step, untrimmed: what the parent commit runs for the same call
  trim1.0    the same with keep_ratio = 1.0: the whole trim pass, nothing trimmed
  trim0.6    the same with keep_ratio = 0.6
trim1.0 must give refit's bits; trim0.6 must keep keep_count(0.6, n_within) pairs of every candidate.  The difference of a trimmed
route to refit is the price of the trim pass (a memset, four histogram and four pick launches, the tie count and the mask, per batch).

    python3 scripts/trim_bench.py [--reps 25] [--warmup 3] [--B 107] [--routes refit,trim1.0,trim0.6]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402
from score_bench import transforms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--routes", default="refit,trim1.0,trim0.6", help="the routes to time, in the order of a round (the checks always run all three)")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, surf, _ = synth(1_000_000, 50_000)
    surf = surf.astype(np.float32)
    Q, B = len(surf), a.B
    r2 = float(np.float32(1.5) * np.float32(1.5))
    T = transforms(surf, B)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    q = torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev)
    Td = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)).to(dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    ws = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)

    out_plain = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), ws(L.pcreg_dev_model_refit_workspace(Q, B, pm.M)), None)
    trimmed_out = lambda: (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), i32(B), torch.empty(B, dtype=torch.float32, device=dev),
                           ws(L.pcreg_dev_model_refit_workspace(Q, B, pm.M)), None)
    out_one, out_six = trimmed_out(), trimmed_out()
    fns = {"refit": lambda: pm.refit_transforms(q, Td, r2, out=out_plain),
           "trim1.0": lambda: pm.refit_transforms(q, Td, r2, out=out_one, keep_ratio=1.0),
           "trim0.6": lambda: pm.refit_transforms(q, Td, r2, out=out_six, keep_ratio=0.6)}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    host = lambda out: [t.cpu().numpy() for t in out[:-2]]
    plain, one, six = host(out_plain), host(out_one), host(out_six)
    same = all(np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)) for x, y in zip(plain, one[:5]))
    same = bool(same and np.array_equal(one[5], plain[2]))
    keep = np.array([0 if n == 0 else min(int(n), max(1, int(math.floor(0.6 * float(n) + 0.5)))) for n in six[5]], np.int32)
    kept_ok = bool(np.array_equal(six[2], keep) and np.array_equal(six[5], plain[2]))
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"Q": Q, "M": pm.M, "B": B, "r": 1.5, "reps": a.reps, "ratio_one_has_the_untrimmed_bits": same, "ratio_0.6_keeps_the_rule": kept_ok,
           "n_within_min_max": [int(six[5].min()), int(six[5].max())], "n_close_0.6_min_max": [int(six[2].min()), int(six[2].max())],
           "fitted": [int((plain[4] == 0).sum()), int((six[4] == 0).sum())], "routes": a.routes, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    pm.close()
    print(json.dumps(res))
    if not same:
        raise SystemExit("keep_ratio = 1.0 does not give the untrimmed call's bits")
    if not kept_ok:
        raise SystemExit("keep_ratio = 0.6 does not keep keep_count(0.6, n_within) pairs of every candidate")


if __name__ == "__main__":
    main()
