"""Timing of the transform refit against a prepared model: one JSON line.

scripts/score_bench.py's shape and candidates: a 50 k crop against 1 M model rows (bench.synth), B = 107 candidate transforms at
r = 1.5.  Timed, alternately in one process after warm-up, with a host clock around a stream synchronise:
  refit      PreparedModel.refit_transforms, one step
  composed   what the entry points before it allow: PreparedModel.score_transforms(rows=True) for the [B][Q] rows, the moved
             points again (pcreg_dev_quick_tf_batched and a cast), then per transform the gather of the model rows and the
             compaction of the hits in torch (no host synchronisation) and pcreg_dev_estimate_transform_indexed, one wave each
  score      PreparedModel.score_transforms alone, counts and sums: what the refit adds to the walk
refit and composed must agree on n_close, and their T_step within 1e-9 (tests/test_gpu_refit.py's bound) wherever both fit.

    python3 scripts/refit_bench.py [--reps 25] [--warmup 3] [--B 107] [--routes refit,composed,score]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402
from score_bench import transforms  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--routes", default="refit,composed,score", help="the routes to time, in the order of a round (the checks always run all three)")
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

    # the new call, with buffers of its own
    out_refit = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B),
                 torch.empty(int(L.pcreg_dev_model_refit_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev), None)
    refit = lambda: pm.refit_transforms(q, Td, r2, out=out_refit)

    # scoring alone, and with rows for the composition
    ws = torch.empty(int(L.pcreg_dev_model_score_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev)
    out_sums = (i32(B), f64(B), None, None, ws)
    out_rows = (i32(B), f64(B), i32(B, Q), torch.empty((B, Q), dtype=torch.float32, device=dev), ws)
    score = lambda: pm.score_transforms(q, Td, r2, out=out_sums)

    m64 = mt.double()
    q64 = q.double()
    tf64 = f64(B, 3, Q)
    comp_T, comp_info = f64(B, 16), i32(B, 2)
    lst = torch.empty(Q + 1, dtype=torch.int32, device=dev)
    ar = torch.arange(Q, dtype=torch.int32, device=dev)
    dump = torch.full((), Q, dtype=torch.int64, device=dev)

    def composed():
        _n, _s, idx, _d = pm.score_transforms(q, Td, r2, rows=True, out=out_rows)
        check(L.pcreg_dev_quick_tf_batched(_p(q64), Q, Q, _p(Td), B, _p(tf64), Q, None, _stream()))
        moved = tf64.float().double()                                      # rounded once to fp32, widened again
        for b in range(B):
            hit = idx[b] >= 0
            p1 = m64[:, idx[b].clamp(min=0).long()].contiguous()           # the model row of every query (row 0 where none)
            pos = torch.cumsum(hit, 0) - 1
            lst.scatter_(0, torch.where(hit, pos, dump), ar)               # the hits' queries in ascending order; misses to the spare slot
            n = hit.sum(dtype=torch.int32).reshape(1)
            check(L.pcreg_dev_estimate_transform_indexed(_p(p1), _p(moved[b]), Q, _p(lst), 0, _p(n), Q, _p(comp_T[b]), _p(comp_info[b]), _stream()))

    fns = {"refit": refit, "composed": composed, "score": score}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    n_new, n_comp = out_refit[2].cpu().numpy(), comp_info[:, 0].cpu().numpy()
    e_new, e_comp = out_refit[4].cpu().numpy() != 0, comp_info[:, 1].cpu().numpy() != 0
    agree = bool(np.array_equal(n_new, n_comp) and np.array_equal(n_new, out_sums[0].cpu().numpy()) and np.array_equal(e_new, e_comp))
    sums_same = bool(np.array_equal(out_refit[3].cpu().numpy().view(np.uint64), out_sums[1].cpu().numpy().view(np.uint64)))
    both = ~e_new & ~e_comp
    diff = np.linalg.norm((out_refit[1].cpu().numpy() - comp_T.cpu().numpy())[both], axis=1) if both.any() else np.zeros(1)
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"Q": Q, "M": pm.M, "B": B, "r": 1.5, "reps": a.reps, "n_close_and_empty_agree": agree, "sum_bits_equal_scoring": sums_same,
           "fitted": int((~e_new).sum()), "n_close_min_max": [int(n_new.min()), int(n_new.max())], "T_step_max_difference": float(diff.max()), "routes": a.routes,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    pm.close()
    print(json.dumps(res))
    if not agree:
        raise SystemExit("the new call and the composition disagree on n_close or on which fits are empty")
    if not diff.max() < 1e-9:
        raise SystemExit("the new call's T_step and the composition's differ by %g" % diff.max())


if __name__ == "__main__":
    main()
