"""Timing of the NDT step against the point-to-plane refit: one JSON line.

scripts/refit_plane_bench.py's protocol: the 50 k crop against 1 M model rows (bench.synth), scripts/score_bench.py's B = 107
candidate transforms, the routes alternating in one process after warm-up, a host clock around a stream synchronise.  Timed:
  ndt1       NdtModel.refit, one step, neighbors = 1
  ndt7       NdtModel.refit, one step, neighbors = 7
  plane      PreparedModel.refit_plane, one step at r = 1.5 (normals: PreparedModel.normals(8), computed once before anything is timed)
  build      NdtModel(model, step): the one-off table of the 1 M rows (the handle's release, which synchronises the device, is not timed)
Reported beside the times: the table's voxels and Gaussians at --step, the pairs per candidate, and for the 11 candidates that
start near the truth the RMS distance of the moved crop from its true place before and after five steps of each route.  No time
is a pass criterion.

    python3 scripts/ndt_bench.py [--reps 25] [--warmup 3] [--B 107] [--step 2.0] [--routes ndt1,ndt7,plane,build]
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
from pcreg_amd._lib import lib  # noqa: E402
from pcreg_amd.device import NdtModel, PreparedModel  # noqa: E402
from score_bench import transforms  # noqa: E402


def rms(surf, T16, truth):
    """the RMS distance of the crop moved by each [16] transform (the library's layout) from its true place; NaN for an empty one"""
    out = []
    for t in T16:
        T = t.reshape(4, 4).T
        if not T.any():
            out.append(float("nan"))
            continue
        moved = surf.astype(np.float64) @ T[:3, :3] + T[3, :3]
        out.append(float(np.sqrt(((moved - truth) ** 2).sum(axis=1).mean())))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--step", type=float, default=2.0)
    ap.add_argument("--routes", default="ndt1,ndt7,plane,build", help="the routes to time, in the order of a round")
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
    nm = NdtModel(mt, a.step)
    q = torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev)
    Td = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)).to(dev)
    nrm = pm.normals(8)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)

    out_plane = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), f64(B), i32(B),
                 torch.empty(int(L.pcreg_dev_model_refit_plane_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev), None)
    outs_ndt = {nb: (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B),
                     torch.empty(max(int(L.pcreg_dev_ndt_refit_workspace(Q, B)), 256), dtype=torch.uint8, device=dev), None) for nb in (1, 7)}
    built = []

    def build():
        built.append(NdtModel(mt, a.step))                                 # (synchronises: the Gaussian count is read back)

    fns = {"ndt1": lambda: nm.refit(q, Td, neighbors=1, out=outs_ndt[1]), "ndt7": lambda: nm.refit(q, Td, neighbors=7, out=outs_ndt[7]),
           "plane": lambda: pm.refit_plane(q, Td, r2, nrm, out=out_plane), "build": build}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    pairs = {nb: outs_ndt[nb][2].cpu().numpy() for nb in (1, 7)}
    fitted = {nb: int((outs_ndt[nb][4].cpu().numpy() == 0).sum()) for nb in (1, 7)}
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            while built:
                built.pop().close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    while built:
        built.pop().close()
    near = slice(0, min(11, B))
    five = {"start": rms(surf, Td.cpu().numpy()[near], truth)}
    five["ndt1"] = rms(surf, nm.refit(q, Td, neighbors=1, steps=5)[0].cpu().numpy()[near], truth)
    five["ndt7"] = rms(surf, nm.refit(q, Td, neighbors=7, steps=5)[0].cpu().numpy()[near], truth)
    five["plane"] = rms(surf, pm.refit_plane(q, Td, r2, nrm, steps=5)[0].cpu().numpy()[near], truth)
    five["point"] = rms(surf, pm.refit_transforms(q, Td, r2, steps=5)[0].cpu().numpy()[near], truth)
    res = {"Q": Q, "M": pm.M, "B": B, "step": a.step, "reps": a.reps, "voxels": nm.n_voxels, "gaussians": nm.n_gaussians,
           "pairs_near_min_max": {str(nb): [int(pairs[nb][near].min()), int(pairs[nb][near].max())] for nb in (1, 7)},
           "pairs_all_min_max": {str(nb): [int(pairs[nb].min()), int(pairs[nb].max())] for nb in (1, 7)}, "fitted": {str(nb): fitted[nb] for nb in (1, 7)},
           "rms_after_five_steps_near": {k: {"median": round(float(np.nanmedian(v)), 4), "max": round(float(np.nanmax(v)), 4), "fits": int(np.isfinite(v).sum())}
                                         for k, v in five.items()},
           "routes": a.routes, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    nm.close()
    pm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
