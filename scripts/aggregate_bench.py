"""Timing of the aggregated final transform (completeExperiment.m:424-458): one JSON line.  A measurement, not a gate.

Shape: 100 spheres x 2000 putative matches each, drawn from 2000 surface and 20 000 model keypoints with the sweep's overlap (a
surface keypoint is paired in every sphere: with its true model keypoint where the sphere holds it, with another row of the
sphere where not), i.e. 2 * 10^5 stacked rows that the first unique cuts to 2000.  The buffers are laid out as a sweep leaves them
(pairs_all, n_pairs, feat_all, row offsets) and handed to SphereSweep.aggregate.  Timed, medians after warm-up, alternating in
the same process:

  resident   SphereSweep.aggregate: stack, aggregate_matches, ransac (3 * 10^4 iterations), indexed fit, the one final read (wall)
  host       the only route without the device unique: pairs to the host, the stacking and np.unique twice there, upload,
             pcreg_dev_ransac, the result read back, estimateTransform at the host tier (wall)
  sort       pcreg_dev_unique_rows3_f64 alone on the stacked surface points (device events) and the bytes per second its
             launches move: 52 n (tile sort) + 56 n per merge pass + 24 n (heads) + 28 n (compaction)

    python3 scripts/aggregate_bench.py [--reps 20] [--warmup 5] [--spheres 100] [--pairs 2000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pcreg_amd as pc  # noqa: E402
from pcreg_amd._lib import DevRansacResult, RansacOpts, check, lib  # noqa: E402
from pcreg_amd.sweep import SphereSweep  # noqa: E402

OPT = dict(minPtNum=3, iterNum=30000, thDist=0.2, thInlrRatio=0.05, REFINE=True, VERBOSE=0)      # completeExperiment.m:446-455


def _p(t):
    return C.c_void_p(t.data_ptr())


def scene(S, VS, VM=20000, seed=0):
    rng = np.random.default_rng(seed)
    featM = rng.uniform([0, 0, 0], [100, 56, 99], (VM, 3))
    centre = np.array([50.0, 28.0, 50.0])
    true = np.argsort(np.linalg.norm(featM - centre, axis=1))[:VS]
    a = 0.3
    R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    featS = featM[true] @ R.T + np.array([2.0, -1.0, 0.5]) + rng.normal(0, 0.02, (VS, 3))
    reach = np.linalg.norm(featM[true] - centre, axis=1).max()
    g = int(math.ceil(S ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.linspace(-0.5, 0.5, g)] * 3, indexing="ij"), -1).reshape(-1, 3)[:S]
    centres = centre + grid * reach                                  # sphere centres across the surface's patch, radius = its reach
    rows, pairs = [], np.zeros((S, VS, 2), dtype=np.int32)
    for i in range(S):
        r = np.nonzero(np.linalg.norm(featM - centres[i], axis=1) < reach)[0]
        pos = np.searchsorted(r, true)
        held = (pos < len(r)) & (r[np.minimum(pos, len(r) - 1)] == true)
        pairs[i, :, 0] = np.arange(1, VS + 1)
        pairs[i, :, 1] = np.where(held, pos, rng.integers(0, len(r), VS)) + 1
        rows.append(r)
    return featM, featS, centres, rows, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spheres", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=2000)
    a = ap.parse_args()
    S, VS = a.spheres, a.pairs
    dev = torch.device("cuda", 0)
    L = lib()
    featM, featS, centres, rows, pairs = scene(S, VS)
    # the state a sweep leaves behind (SphereSweep._finish_sweep), on a sweep object whose descriptors play no part here
    sw = SphereSweep(featM, np.zeros((len(featM), 1)), featS, np.zeros((VS, 1)))
    row_off = np.zeros(S + 1, dtype=np.int64); row_off[1:] = np.cumsum([len(r) for r in rows])
    result = dict(centres=centres, num_putative=np.full(S, VS, dtype=np.int64))
    feat_all = torch.from_numpy(np.ascontiguousarray(featM[np.concatenate(rows)])).to(dev)
    sw._agg = dict(result=result, pairs_all=torch.from_numpy(pairs).to(dev), n_pairs=torch.full((S,), VS, dtype=torch.int32, device=dev),
                   feat_all=feat_all, roff_dev=torch.from_numpy(row_off[:S].copy()).to(dev), featS=sw.featS, VS=VS)
    members = np.arange(S)
    st = sw._agg

    def resident():
        return sw.aggregate(result, members, OPT, seed=1)

    def host_route():
        pr = st["pairs_all"].cpu().numpy(); npr = st["n_pairs"].cpu().numpy()                  # pairs to the host
        fa = st["feat_all"].cpu().numpy(); fs = st["featS"].cpu().numpy()
        p1 = np.vstack([fs[pr[i, :npr[i], 0] - 1] for i in members])
        p2 = np.vstack([fa[row_off[i] + pr[i, :npr[i], 1] - 1] for i in members])
        _, ia = np.unique(p1, axis=0, return_index=True); p1, p2 = p1[ia], p2[ia]                # :440-441
        _, ia = np.unique(p2, axis=0, return_index=True); p1, p2 = p1[ia], p2[ia]                # :442-443
        n = len(p1)
        d1 = torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev); d2 = torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        o = RansacOpts(3, OPT["iterNum"], OPT["thDist"], OPT["thInlrRatio"], 1, 0, 1)
        res = torch.zeros(C.sizeof(DevRansacResult) // 4, dtype=torch.int32, device=dev)
        inl = torch.zeros(n, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(L.pcreg_dev_ransac_workspace(n, o.iterNum)), 256), dtype=torch.uint8, device=dev)
        check(L.pcreg_dev_ransac(_p(d1), _p(d2), _p(n_dev), n, n, C.byref(o), None, _p(res), _p(inl), _p(ws), C.c_size_t(ws.numel()),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        r = DevRansacResult.from_buffer_copy(res.cpu().numpy().tobytes())
        idx = inl[:r.n_inliers].cpu().numpy().astype(np.int64) - 1
        return dict(n_unique2=n, maxInliers=r.max_inliers, numSuccess=r.num_success, T_final=pc.estimateTransform(p1[idx], p2[idx]))

    total = S * VS
    p1 = torch.empty((3, total), dtype=torch.float64, device=dev)
    stacked = st["featS"][(st["pairs_all"][:, :, 0].reshape(-1) - 1).long()]                  # the stacked surface points
    p1.copy_(stacked.t())
    n_dev = torch.tensor([total], dtype=torch.int32, device=dev)
    ia = torch.empty(total, dtype=torch.int32, device=dev); nu = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = int(L.pcreg_dev_unique_rows3_workspace(total))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def sort_only():
        check(L.pcreg_dev_unique_rows3_f64(_p(p1), _p(n_dev), total, total, 0, _p(ia), _p(nu), _p(ws), C.c_size_t(wsb),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        resident(); host_route(); sort_only()
    t = {"resident": [], "host": [], "sort": []}
    for _ in range(a.reps):                                           # alternating: all three see the same clocks
        ms, got = wall_ms(resident); t["resident"].append(ms)
        ms, ref = wall_ms(host_route); t["host"].append(ms)
        t["sort"].append(event_ms(sort_only))
    same = (got["n_unique2"] == ref["n_unique2"] and got["maxInliers"] == ref["maxInliers"] and got["numSuccess"] == ref["numSuccess"] and
            float(np.linalg.norm(got["T_final"] - ref["T_final"])) < 1e-9)
    passes = max(0, math.ceil(math.log2(max(total / 2048, 1))))
    moved = total * (52 + 56 * passes + 24 + 28)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"spheres": S, "pairs_per_sphere": VS, "rows": total, "n_unique1": got["n_unique1"], "n_unique2": got["n_unique2"],
                      "maxInliers": got["maxInliers"], "routes_agree": bool(same), "resident_ms": round(med["resident"], 3),
                      "host_route_ms": round(med["host"], 3), "sort_ms": round(med["sort"], 4), "merge_passes": passes,
                      "sort_bytes": moved, "sort_GBps": round(moved / (med["sort"] * 1e-3) / 1e9, 1),
                      "min_ms": {k: round(float(np.min(v)), 4) for k, v in t.items()}, "reps": a.reps, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
