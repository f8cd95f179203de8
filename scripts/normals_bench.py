"""Timing of the normals of a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows), k = 6 and k = 16.  Timed, alternately in one process after warm-up, with a host clock
around a stream synchronise:
  normals    PreparedModel.normals (normals and variation, no viewpoint), buffers of its own
  composed   what the entry points before it allow: PreparedModel.knn of the model against itself in batches of at most 4 Mi
             rows, a gather of the neighbours, the float64 scatter matrices in torch, torch.linalg.eigh
Both must agree in direction (|cos| of the angle between them) on the rows whose two smallest eigenvalues are apart.  Reported
per k: median, min, max and interquartile range of each route, and the share of tile visits the walk makes ("knn_stats").
--max-seconds bounds the timed loop of one k: when it is used up the loop stops after a whole round and the JSON says how many
repetitions were made.

    python3 scripts/normals_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--ks 6,16] [--max-seconds 0]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402

KNN_BATCH = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--ks", type=str, default="6,16")
    ap.add_argument("--max-seconds", type=float, default=0.0)
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = model.astype(np.float32)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    M = pm.M
    res = {"M": M, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "k": {}}
    for k in [int(x) for x in a.ks.split(",")]:
        ws = torch.empty(max(int(L.pcreg_dev_model_normals_workspace(M, k)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty((3, M), dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev), ws)
        new = lambda: pm.normals(k, variation=True, out=out)
        comp = {}

        def composed():
            nrm = torch.empty((M, 3), dtype=torch.float64, device=dev)
            var = torch.empty(M, dtype=torch.float64, device=dev)
            gap = torch.empty(M, dtype=torch.float64, device=dev)
            rows = mt.t().double()                                                   # [M, 3]
            for b0 in range(0, M, KNN_BATCH):
                b1 = min(b0 + KNN_BATCH, M)
                idx, _dist = pm.knn(mt[:, b0:b1], k)
                nb = rows[idx.long().reshape(-1)].reshape(b1 - b0, k, 3)             # the gather (every row has k neighbours here)
                cen = nb - nb.mean(dim=1, keepdim=True)
                cov = cen.transpose(1, 2) @ cen
                lam, vec = torch.linalg.eigh(cov)
                nrm[b0:b1] = vec[:, :, 0]
                var[b0:b1] = lam[:, 0] / lam.sum(dim=1)
                gap[b0:b1] = (lam[:, 1] - lam[:, 0]) / torch.linalg.matrix_norm(cov)
            comp["normals"], comp["variation"], comp["gap"] = nrm, var, gap

        fns = {"composed": composed, "normals": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        got = out[0].t().double()
        cosang = (got * comp["normals"]).sum(dim=1).abs() / got.norm(dim=1)          # (fp32 components: not a unit vector to 1e-9)
        clear = comp["gap"] >= 1e-3
        agree = float((cosang[clear] > 1.0 - 1e-9).double().mean().item())
        var_diff = float((out[1].double() - comp["variation"]).abs().max().item())
        times = {name: [] for name in fns}
        t_loop = time.perf_counter()
        for _ in range(a.reps):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.current_stream().synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
            if a.max_seconds > 0 and time.perf_counter() - t_loop > a.max_seconds:
                break
        stats = (C.c_longlong * 4)()
        check(L.pcreg_debug_set(b"knn_stats", 1))
        check(L.pcreg_debug_knn_stats(stats, 1))
        new()
        torch.cuda.synchronize()
        check(L.pcreg_debug_knn_stats(stats, 1))
        check(L.pcreg_debug_set(b"knn_stats", 0))
        entry = {"reps_done": len(times["normals"]), "first_call_ms": first, "rows_with_clear_gap": round(float(clear.double().mean().item()), 5),
                 "direction_agrees_share": round(agree, 6), "variation_max_abs_diff": var_diff,
                 "visited_tiles": int(stats[1]), "nominal_tiles": int(stats[2]), "visited_share": round(stats[1] / stats[2], 5) if stats[2] else None}
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        res["k"][str(k)] = entry
        del comp, out, ws
    pm.close()
    print(json.dumps(res))
    bad = [k for k, e in res["k"].items() if e["direction_agrees_share"] < 0.999]
    if bad:
        raise SystemExit(f"the new call and the composition disagree in direction at k = {bad}")


if __name__ == "__main__":
    main()
