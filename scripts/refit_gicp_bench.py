"""Timing of the plane-to-plane (generalized ICP) step against the point-to-plane step: one JSON line.

scripts/refit_plane_bench.py's protocol: the 50 k crop against 1 M model rows (bench.synth), scripts/score_bench.py's B = 107
candidate transforms, the routes alternating in one process after warm-up, a host clock around a stream synchronise.  Both sets
of normals are computed once before anything is timed: PreparedModel.normals(8) of the model, and of a prepared model of the crop.
Timed:
  plane      PreparedModel.refit_plane, one step at r = 1.5
  gicp       PreparedModel.refit_gicp, one step at r = 1.5 with --epsilon
Reported beside the times: the pairs per candidate, and for the 11 candidates that start near the truth the RMS distance of the
moved crop from its true place before and after five steps of each route (and of the point-to-point step).  No time is a pass
criterion.

    python3 scripts/refit_gicp_bench.py [--reps 25] [--warmup 3] [--B 107] [--epsilon 1e-3] [--routes plane,gicp]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from ndt_bench import rms  # noqa: E402
from pcreg_amd._lib import lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402
from score_bench import transforms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--routes", default="plane,gicp", help="the routes to time, in the order of a round")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, surf, crop = synth(1_000_000, 50_000)
    surf = surf.astype(np.float32)
    truth = model[crop].astype(np.float64)
    Q, B = len(surf), a.B
    r2 = float(np.float32(1.5) * np.float32(1.5))
    T = transforms(surf, B)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    q = torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev)
    Td = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)).to(dev)
    nrm = pm.normals(8)
    pq = PreparedModel(q)
    nq = pq.normals(8)
    torch.cuda.synchronize()
    pq.close()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    outs = {k: (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), f64(B), i32(B),
                torch.empty(int(L.pcreg_dev_model_refit_gicp_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev), None) for k in ("plane", "gicp")}
    fns = {"plane": lambda: pm.refit_plane(q, Td, r2, nrm, out=outs["plane"]),
           "gicp": lambda: pm.refit_gicp(q, Td, r2, nrm, nq, epsilon=a.epsilon, out=outs["gicp"])}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    pairs = {k: outs[k][4].cpu().numpy() for k in outs}
    fitted = {k: int((outs[k][6].cpu().numpy() == 0).sum()) for k in outs}
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    near = slice(0, min(11, B))
    five = {"start": rms(surf, Td.cpu().numpy()[near], truth)}
    five["gicp"] = rms(surf, pm.refit_gicp(q, Td, r2, nrm, nq, epsilon=a.epsilon, steps=5)[0].cpu().numpy()[near], truth)
    five["plane"] = rms(surf, pm.refit_plane(q, Td, r2, nrm, steps=5)[0].cpu().numpy()[near], truth)
    five["point"] = rms(surf, pm.refit_transforms(q, Td, r2, steps=5)[0].cpu().numpy()[near], truth)
    res = {"Q": Q, "M": pm.M, "B": B, "epsilon": a.epsilon, "reps": a.reps,
           "pairs_near_min_max": {k: [int(pairs[k][near].min()), int(pairs[k][near].max())] for k in pairs},
           "pairs_all_min_max": {k: [int(pairs[k].min()), int(pairs[k].max())] for k in pairs}, "fitted": fitted,
           "rms_after_five_steps_near": {k: {"median": round(float(np.nanmedian(v)), 4), "max": round(float(np.nanmax(v)), 4), "fits": int(np.isfinite(v).sum())}
                                         for k, v in five.items()},
           "routes": a.routes, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    pm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
