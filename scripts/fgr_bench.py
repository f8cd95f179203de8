#!/usr/bin/env python3
"""Fast global registration (pcreg_dev_fgr_batched) timed on the device tier, once per kernel form, beside
pcreg_dev_ransac_batched on the same pairs: the sweep's 107 trial sizes (170 .. 2000 pairs, 60 % outliers) as one batch, and one
registration of 100 000 pairs (chained by its size).  Prints one JSON line.  Times are medians of --reps enqueue-to-event intervals
after --warmup calls; nothing is read back inside an interval.

    python scripts/fgr_bench.py [--reps 20] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pcreg_amd._lib import DevRansacResult, RansacOpts, check, lib              # noqa: E402
from pcreg_amd.device import _p, _stream, fgr_batched_dev, fgr_results          # noqa: E402


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene(rng, n, share=0.6):
    p2 = rng.random((n, 3)) * 100.0
    R, t = rotation(rng.normal(size=3), 1.5), rng.uniform(-20, 20, 3)
    p1 = p2 @ R.T + t + rng.normal(0, 0.05, (n, 3))
    out = rng.permutation(n)[:int(share * n)]
    p1[out] = rng.random((len(out), 3)) * 140.0 - 20.0
    return p1, p2, n - len(out)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def batch(rng, sizes):
    ps = [scene(rng, n) for n in sizes]
    offs = np.zeros(len(sizes) + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    dev = torch.device("cuda")
    p1 = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[0] for p in ps]).T)).to(dev)
    p2 = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[1] for p in ps]).T)).to(dev)
    return p1, p2, torch.from_numpy(offs).to(dev), [p[2] for p in ps]


def measure(name, sizes, rng, reps, warmup, ransac_iters):
    L = lib()
    p1, p2, offs, planted = batch(rng, sizes)
    B, n_cap, ld = len(sizes), max(sizes), int(p1.shape[1])
    opts = dict(delta2=1.0)
    out = dict(case=name, B=B, pairs=int(sum(sizes)), n_cap=n_cap)
    ws = torch.empty(L.pcreg_dev_fgr_batched_workspace(n_cap, B, 128), dtype=torch.uint8, device=p1.device)
    for form in ("resident", "chain"):
        if form == "resident" and n_cap > L.pcreg_fgr_resident_capacity():
            continue
        check(L.pcreg_debug_set(b"fgr_chain", int(form == "chain")))
        res = fgr_batched_dev(p1, p2, offs, n_cap, opts, ws=ws)[0]
        rs = fgr_results(res.cpu().numpy())
        out[f"fgr_{form}_planted_recovered"] = int(sum(r.n_inliers == k and not r.failed for r, k in zip(rs, planted)))
        med, lo = timed(lambda: fgr_batched_dev(p1, p2, offs, n_cap, opts, ws=ws), reps, warmup)
        out[f"fgr_{form}_ms"], out[f"fgr_{form}_ms_min"] = round(med, 4), round(lo, 4)
    check(L.pcreg_debug_set(b"fgr_chain", 0))
    o = RansacOpts(3, ransac_iters, 1.0, 0.1, 1, 0, 7)
    wsr = torch.empty(max(L.pcreg_dev_ransac_batched_workspace(n_cap, o.iterNum, B), 256), dtype=torch.uint8, device=p1.device)
    rres = torch.zeros((B, C.sizeof(DevRansacResult)), dtype=torch.uint8, device=p1.device)
    rinl = torch.empty(ld, dtype=torch.int32, device=p1.device)
    run = lambda: check(L.pcreg_dev_ransac_batched(_p(p1), _p(p2), ld, _p(offs), B, n_cap, C.byref(o), _p(rres), _p(rinl), _p(wsr),
                                                   C.c_size_t(wsr.numel()), _stream()))
    med, lo = timed(run, reps, warmup)
    out["ransac_iters"], out["ransac_ms"], out["ransac_ms_min"] = ransac_iters, round(med, 4), round(lo, 4)
    rr = [DevRansacResult.from_buffer_copy(bytes(r)) for r in rres.cpu().numpy()]
    out["ransac_succeeded"] = int(sum(not r.failed for r in rr))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    sizes = [int(v) for v in rng.integers(170, 2001, 107)]
    res = [measure("sweep: 107 trials", sizes, rng, a.reps, a.warmup, 10_000),
           measure("one registration of 100 000 pairs", [100_000], rng, max(a.reps // 4, 3), 1, 30_000)]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
