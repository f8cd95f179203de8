"""Timing of the coherent-point-drift step against the point-to-plane step on the same downsampled clouds: one JSON line.

scripts/refit_plane_bench.py's protocol: bench.synth's 50 k crop and 1 M model rows, both reduced by downsample_grid (pcdownsample's
'gridAverage') to about --crop-points and --model-points points -- coherent point drift pairs every point with every row, so it is
run on downsampled clouds --, scripts/score_bench.py's B = 107 candidate transforms, the routes alternating in one process after
warm-up, a host clock around a stream synchronise.  The model's normals (k = 8) are computed once before anything is timed.
Timed:
  plane      PreparedModel.refit_plane, one step at r = 1.5
  cpd        PreparedModel.refit_cpd, one step from --sigma2 (0: the initial variance) with --outlier
Reported beside the times: the pairs of a step (B x live queries x live rows) and pairs per second of the whole step, and for the
11 candidates that start near the truth the RMS distance of the (full) moved crop from its true place before and after five
steps of each route (and of the point-to-point step).  No time is a pass criterion.

    python3 scripts/refit_cpd_bench.py [--reps 25] [--warmup 3] [--B 107] [--outlier 0.1] [--sigma2 0] [--crop-points 5000] [--model-points 20000]
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
from pcreg_amd.device import PreparedModel, downsample_grid  # noqa: E402
from score_bench import transforms  # noqa: E402


def reduced(cloud: torch.Tensor, target: int):
    """the cloud downsampled to about `target` points: the grid step found by bisection -> (a contiguous [3, n] tensor, the step)"""
    ext = float((cloud.max(dim=1).values - cloud.min(dim=1).values).max())
    lo, hi = ext * 1e-4, ext
    for _ in range(24):
        step = (lo * hi) ** 0.5
        out, _c, _l, n_out, _i = downsample_grid(cloud, step)
        n = int(n_out.item())
        if abs(n - target) <= 0.02 * target:
            break
        lo, hi = (lo, step) if n < target else (step, hi)
    return out[:, :n].contiguous(), step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--outlier", type=float, default=0.1)
    ap.add_argument("--sigma2", type=float, default=0.0, help="the variance every candidate starts from; 0: coherent point drift's initial value")
    ap.add_argument("--crop-points", type=int, default=5000)
    ap.add_argument("--model-points", type=int, default=20000)
    ap.add_argument("--routes", default="plane,cpd", help="the routes to time, in the order of a round")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, surf, crop = synth(1_000_000, 50_000)
    surf = surf.astype(np.float32)
    truth = model[crop].astype(np.float64)
    B = a.B
    r2 = float(np.float32(1.5) * np.float32(1.5))
    T = transforms(surf, B)
    mt, m_step = reduced(torch.from_numpy(np.ascontiguousarray(model.T)).to(dev), a.model_points)
    q, q_step = reduced(torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev), a.crop_points)
    pm = PreparedModel(mt)
    Q = int(q.shape[1])
    Td = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)).to(dev)
    nrm = pm.normals(8)
    torch.cuda.synchronize()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    ws = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
    out_plane = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), f64(B), i32(B), ws(L.pcreg_dev_model_refit_plane_workspace(Q, B, pm.M)), None)
    out_cpd = (f64(B, 16), f64(B, 16), f64(B), f64(B), f64(B), f64(B), i32(B), i32(B), ws(L.pcreg_dev_model_refit_cpd_workspace(Q, B, pm.M)), None)
    fns = {"plane": lambda: pm.refit_plane(q, Td, r2, nrm, out=out_plane),
           "cpd": lambda: pm.refit_cpd(q, Td, sigma2=a.sigma2, outlier=a.outlier, out=out_cpd)}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    n_live = out_cpd[6].cpu().numpy()
    fitted = {"plane": int((out_plane[6].cpu().numpy() == 0).sum()), "cpd": int((out_cpd[7].cpu().numpy() == 0).sum())}
    pairs = int(n_live.astype(np.int64).sum()) * pm.M
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
    five["cpd"] = rms(surf, pm.refit_cpd(q, Td, sigma2=a.sigma2, outlier=a.outlier, steps=5)[0].cpu().numpy()[near], truth)
    five["cpd20"] = rms(surf, pm.refit_cpd(q, Td, sigma2=a.sigma2, outlier=a.outlier, steps=20)[0].cpu().numpy()[near], truth)
    five["plane"] = rms(surf, pm.refit_plane(q, Td, r2, nrm, steps=5)[0].cpu().numpy()[near], truth)
    five["point"] = rms(surf, pm.refit_transforms(q, Td, r2, steps=5)[0].cpu().numpy()[near], truth)
    res = {"Q": Q, "M": pm.M, "B": B, "crop_step": round(q_step, 4), "model_step": round(m_step, 4), "outlier": a.outlier, "sigma2_in": a.sigma2, "reps": a.reps,
           "pairs_per_step": pairs, "fitted": fitted,
           "rms_after_five_steps_near": {k: {"median": round(float(np.nanmedian(v)), 4), "max": round(float(np.nanmax(v)), 4), "fits": int(np.isfinite(v).sum())}
                                         for k, v in five.items()},
           "routes": a.routes, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    if "cpd" in times:
        res["cpd_pairs_per_second_whole_step"] = float(f"{pairs / (np.median(times['cpd']) * 1e-3):.4g}")
    pm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
