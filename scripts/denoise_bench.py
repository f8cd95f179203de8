"""Timing of the statistical outlier removal of a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows), k = 4 and k = 16, threshold 1.  Timed, alternately in one process after warm-up, with a
host clock around a stream synchronise:
  denoise    PreparedModel.denoise (mean distances, inlier rows, count and statistic), buffers of its own
  composed   what the entry points before it allow: PreparedModel.knn of the model against itself with k + 1 in batches of at most
             4 Mi rows, then in torch float64 the square root, the row mean over the k others, mean, std, compare and nonzero
Reported per k: median, min, max and interquartile range of each route, the agreement of the two inlier sets (the composition adds
in torch's order, so a row within rounding of the threshold may differ), the largest relative difference of the mean distances,
and the share of tile visits the walk makes ("knn_stats").  Seed, walk and statistic are not timed apart.
--max-seconds bounds the timed loop of one k: when it is used up the loop stops after a whole round and the JSON says how many
repetitions were made.

    python3 scripts/denoise_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--ks 4,16] [--threshold 1.0] [--max-seconds 0]
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
    ap.add_argument("--ks", type=str, default="4,16")
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=0.0)
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = model.astype(np.float32)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    M, t = pm.M, a.threshold
    res = {"M": M, "threshold": t, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "k": {}}
    for k in [int(x) for x in a.ks.split(",")]:
        ws = torch.empty(max(int(L.pcreg_dev_model_denoise_workspace(M, k)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.int32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.float64, device=dev), ws)
        new = lambda: pm.denoise(k, t, out=out)
        comp = {}

        def composed():
            d = torch.empty(M, dtype=torch.float64, device=dev)
            for b0 in range(0, M, KNN_BATCH):
                b1 = min(b0 + KNN_BATCH, M)
                _idx, dist = pm.knn(mt[:, b0:b1], k + 1)
                d[b0:b1] = dist.double().sqrt()[:, 1:].sum(dim=1) / k                # (every row has k + 1 neighbours here)
            thr = d.mean() + t * d.std()
            comp["mean_dist"], comp["thr"], comp["inliers"] = d, thr, torch.nonzero(d <= thr).squeeze(1)

        fns = {"composed": composed, "denoise": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        n_new = int(out[2].item())
        mine = torch.zeros(M, dtype=torch.bool, device=dev); mine[out[1][:n_new].long()] = True
        theirs = torch.zeros(M, dtype=torch.bool, device=dev); theirs[comp["inliers"]] = True
        differ = int((mine != theirs).sum().item())
        rel = float(((out[0] - comp["mean_dist"]).abs() / comp["mean_dist"].clamp_min(1e-300)).max().item())
        thr_rel = float(abs(out[3][0].item() - comp["thr"].item()) / comp["thr"].item())
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
        entry = {"reps_done": len(times["denoise"]), "first_call_ms": first, "inliers": n_new, "inliers_composed": int(comp["inliers"].numel()),
                 "rows_that_differ": differ, "mean_dist_max_rel_diff": rel, "thr_rel_diff": thr_rel, "thr": float(out[3][0].item()),
                 "visited_tiles": int(stats[1]), "nominal_tiles": int(stats[2]), "visited_share": round(stats[1] / stats[2], 5) if stats[2] else None}
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["denoise_ms"]["median"], 2)
        res["k"][str(k)] = entry
        del comp, out, ws
    pm.close()
    print(json.dumps(res))
    bad = [k for k, e in res["k"].items() if e["rows_that_differ"] > 1e-5 * M + 1]
    if bad:
        raise SystemExit(f"the new call and the composition disagree on the inlier set at k = {bad}")


if __name__ == "__main__":
    main()
