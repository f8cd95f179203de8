"""Timing of the radius search against a prepared model: one JSON line.

On the bench shape (bench.synth: a 50 k crop against 1 M model rows) and on uniformly scattered queries over the same box, for
r = 1, 2, 4: median device-event times of 20 calls after warm-up of the count call and of the fill call, the rows returned and
the share of (query block, tile) pairs each call visits ("knn_stats"); in the same process, alternating with them, the
k-nearest search with k = 1 and k = 32 on the same queries (the yardsticks).

    python3 scripts/range_bench.py [--reps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import BBOX, synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402


def _time_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _medians_ms(fns, reps, warmup):
    """the calls alternate inside every repetition, so that all of them see the same clocks"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(_time_ms(fn))
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def _visited(fn):
    L = lib()
    out = (C.c_longlong * 4)()
    check(L.pcreg_debug_set(b"knn_stats", 1))
    check(L.pcreg_debug_knn_stats(out, 1))
    fn()
    torch.cuda.synchronize()
    check(L.pcreg_debug_knn_stats(out, 1))
    check(L.pcreg_debug_set(b"knn_stats", 0))
    return round(out[1] / out[2], 4) if out[2] else None


def run_case(pm, surf, reps, warmup):
    L, dev = lib(), torch.device("cuda", 0)
    Q = len(surf)
    q = torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev)
    res = {"Q": Q, "M": pm.M}
    knn = {}
    for k in (1, 32):
        out = (torch.empty((Q, k), dtype=torch.int32, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev),
               torch.empty(int(L.pcreg_dev_model_knn_workspace(Q, pm.M, k)), dtype=torch.uint8, device=dev))
        knn[f"k{k}_ms"] = (lambda k=k, out=out: pm.knn(q, k, out=out))
    ws = torch.empty(int(L.pcreg_dev_model_range_workspace(Q, pm.M)), dtype=torch.uint8, device=dev)
    for r in (1.0, 2.0, 4.0):
        r2 = float(np.float32(r) ** 2)
        cnt = (torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q + 1, dtype=torch.int64, device=dev), ws)
        pm.rangesearch_count(q, r2, out=cnt)
        total = int(cnt[1][-1].item())
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        dist = torch.empty(total, dtype=torch.float32, device=dev)
        count = lambda: pm.rangesearch_count(q, r2, out=cnt)
        fill = lambda: pm.rangesearch_fill(q, r2, cnt[1], idx, dist, ws=ws)
        t = _medians_ms({"count_ms": count, "fill_ms": fill, **knn}, reps, warmup)
        t["count_plus_fill_ms"] = round(t["count_ms"] + t["fill_ms"], 4)
        t.update(rows=total, rows_per_query=round(total / Q, 2), count_visited=_visited(count), fill_visited=_visited(fill))
        res[f"r{r:g}"] = t
        del idx, dist
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    model, surf, _ = synth(1_000_000, 50_000)
    rng = np.random.default_rng(1)
    scattered = (rng.random((50_000, 3)) * BBOX).astype(np.float32)
    t = torch.from_numpy(np.ascontiguousarray(model.T)).to(torch.device("cuda", 0))
    pm = PreparedModel(t)
    out = {"bench_crop": run_case(pm, surf.astype(np.float32), a.reps, a.warmup),
           "scattered": run_case(pm, scattered, a.reps, a.warmup), "device": torch.cuda.get_device_name(0)}
    pm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
