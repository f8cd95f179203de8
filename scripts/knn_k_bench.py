"""Timing of the k-nearest search against a prepared model: one JSON line.

On the bench shape (bench.synth: a 50 k crop against 1 M model rows) and on uniformly scattered queries over the same box,
median device-event times of 20 calls after warm-up for k = 1, 2, 8, 16, 32 and for the top-2 search on the same prepared
model, plus the share of (query block, tile) pairs each search visits ("knn_stats").

    python3 scripts/knn_k_bench.py [--reps 20] [--warmup 5]
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


def _p(t):
    return C.c_void_p(t.data_ptr())


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


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
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"Q": Q, "M": pm.M}
    i2 = torch.empty((Q, 2), dtype=torch.int32, device=dev)
    d2 = torch.empty((Q, 2), dtype=torch.float32, device=dev)
    ws2 = torch.empty(L.pcreg_dev_model_search_workspace(Q, pm.M), dtype=torch.uint8, device=dev)
    top2 = lambda: check(L.pcreg_dev_model_search_f32(pm.handle, _p(q), Q, Q, C.c_int32(0), _p(i2), _p(d2), _p(ws2),
                                                      C.c_size_t(ws2.numel()), stream()))
    res["top2_ms"] = round(_median_ms(top2, reps, warmup), 4)
    res["top2_visited"] = _visited(top2)
    for k in (1, 2, 8, 16, 32):
        out = (torch.empty((Q, k), dtype=torch.int32, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev),
               torch.empty(int(L.pcreg_dev_model_knn_workspace(Q, pm.M, k)), dtype=torch.uint8, device=dev))
        fn = lambda: pm.knn(q, k, out=out)
        res[f"k{k}_ms"] = round(_median_ms(fn, reps, warmup), 4)
        res[f"k{k}_visited"] = _visited(fn)
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
