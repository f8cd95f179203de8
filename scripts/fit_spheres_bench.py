"""Timing of MSAC sphere extraction on a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows) with three synthetic marker spheres added by this script's own seed (radii 4, 3 and 2.5,
--marker-rows rows each, radial sigma 0.05), max_distance 0.5, B = 1000 trials, P = 1 and P = 4 spheres, min_inliers 4.  Timed,
alternately in one process after warm-up, with a host clock around a stream synchronise:
  fit_spheres  PreparedModel.fit_spheres, buffers of its own
  composed     what the entry points before it allow, through torch: per round four random alive rows per trial, the circumspheres
               in float64, the [rows] x [trials] radial residuals as one fp32 distance matrix per chunk of trials (chunked so that a
               chunk's matrix stays under --chunk-mb), the truncated squared residuals summed per trial, argmin, the algebraic
               least-squares refit of its inliers in float64, the classification, ONE host read per round (the inlier count, which
               decides whether to go on) and a boolean gather of the remaining rows
The composition is the baseline, not a restatement of the contract: its sums are floating point and its sampler is torch's, so
the two routes find spheres of similar, not equal, size; the sizes are reported.  No time is fixed in advance.  --route fit_spheres
runs the new call alone (for a kernel trace).

    python3 scripts/fit_spheres_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--B 1000] [--spheres 1,4] [--t 0.5] [--route both]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402

MARKER_RADII = (4.0, 3.0, 2.5)


def with_markers(model: np.ndarray, rows_each: int, seed: int = 31) -> np.ndarray:
    """the model with three marker spheres written over its last 3 * rows_each rows, centres inside its box"""
    rng = np.random.default_rng(seed)
    out = np.array(model, np.float32)
    lo, hi = out.min(axis=0).astype(np.float64), out.max(axis=0).astype(np.float64)
    at = len(out) - 3 * rows_each
    for k, R in enumerate(MARKER_RADII):
        c = lo + (hi - lo) * rng.uniform(0.2, 0.8, 3)
        v = rng.normal(size=(rows_each, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        out[at + k * rows_each:at + (k + 1) * rows_each] = (c + v * (R + rng.normal(0, 0.05, (rows_each, 1)))).astype(np.float32)
    return out[rng.permutation(len(out))]


def composed_spheres(p, t, B, P, min_inliers, chunk, gen):
    """p: [M, 3] float32 on the device -> the inlier counts of the spheres found"""
    t2 = float(np.float32(t) * np.float32(t))
    s = float(np.float32(2.0 ** 20 / t2))
    rows = p[torch.isfinite(p).all(dim=1)]
    counts = []
    for _ in range(P):
        nA = rows.shape[0]
        if nA < 4:
            break
        pick = torch.randint(0, nA, (B, 4), device=p.device, generator=gen)
        q = rows[pick].double()                                               # [B, 4, 3]
        d = q[:, 1:] - q[:, :1]                                               # [B, 3, 3]
        bb = (d * d).sum(dim=2)
        X = torch.stack([torch.linalg.cross(d[:, 1], d[:, 2]), torch.linalg.cross(d[:, 2], d[:, 0]), torch.linalg.cross(d[:, 0], d[:, 1])], dim=1)
        det = (d[:, 0] * X[:, 0]).sum(dim=1)
        u = (bb[:, :, None] * X).sum(dim=1) / (2.0 * det)[:, None]
        R = u.norm(dim=1)
        srt = pick.sort(dim=1).values
        ok = (det != 0) & torch.isfinite(u).all(dim=1) & torch.isfinite(R) & (srt[:, 1:] != srt[:, :-1]).all(dim=1)
        cf = torch.where(ok[:, None], q[:, 0] + u, torch.zeros_like(u)).float()
        Rf = torch.where(ok, R, torch.zeros_like(R)).float()
        cost = torch.empty(B, dtype=torch.float64, device=p.device)
        cnt = torch.empty(B, dtype=torch.int64, device=p.device)
        for b0 in range(0, B, chunk):
            r = torch.cdist(rows, cf[b0:b0 + chunk]) - Rf[None, b0:b0 + chunk]   # [nA, chunk]
            r2 = r * r
            inl = r2 <= t2
            cost[b0:b0 + chunk] = torch.where(inl, r2 * s, torch.full_like(r2, 2.0 ** 20)).sum(dim=0, dtype=torch.float64)
            cnt[b0:b0 + chunk] = inl.sum(dim=0)
        cost = torch.where(ok & (cnt >= 4), cost, torch.full_like(cost, float("inf")))
        best = torch.argmin(cost)
        r = (rows - cf[best]).norm(dim=1) - Rf[best]
        g = (rows[r * r <= t2] - q[best, 0].float()).double()                 # the algebraic refit: g . a + beta = |g|^2
        A = torch.cat([g, torch.ones_like(g[:, :1])], dim=1)
        sol = torch.linalg.solve(A.t() @ A, A.t() @ (g * g).sum(dim=1))          # (its normal equations, 4 x 4)
        cg = sol[:3] / 2
        R2 = (sol[3] + (cg * cg).sum()).float().sqrt()
        centre = (q[best, 0] + cg).float()
        r = (rows - centre).norm(dim=1) - R2
        keep = ~(r * r <= t2)
        n_in = int((~keep).sum().item())                                      # the round's one host read
        if not bool(torch.isfinite(cost[best]).item()) or n_in < min_inliers:
            break
        counts.append(n_in)
        rows = rows[keep]
    return counts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--spheres", default="1,4")
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--marker-rows", type=int, default=2000)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--route", choices=("both", "fit_spheres"), default="both")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = with_markers(model.astype(np.float32), a.marker_rows)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    rows = mt.t().contiguous()
    pm = PreparedModel(mt)
    M, B = pm.M, a.B
    chunk = max(1, min(B, (a.chunk_mb << 20) // (4 * M)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    res = {"M": M, "B": B, "max_distance": a.t, "reps": a.reps, "warmup": a.warmup, "chunk_trials": chunk, "marker_rows": a.marker_rows,
           "device": torch.cuda.get_device_name(0), "spheres": {}}
    for P in [int(x) for x in a.spheres.split(",")]:
        i32, f64 = torch.int32, torch.float64
        ws = torch.empty(max(int(L.pcreg_dev_model_fit_spheres_workspace(M, B)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty(M, dtype=i32, device=dev), torch.empty((P, 4), dtype=f64, device=dev), torch.empty(P, dtype=i32, device=dev),
               torch.empty(P, dtype=f64, device=dev), torch.empty(P, dtype=i32, device=dev), torch.empty(1, dtype=i32, device=dev),
               torch.empty(P, dtype=i32, device=dev), torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=i32, device=dev), ws)
        new = lambda: pm.fit_spheres(a.t, max_spheres=P, n_trials=B, min_inliers=4, seed=9, out=out)
        comp = {}

        def composed():
            comp["counts"] = composed_spheres(rows, a.t, B, P, 4, chunk, gen)

        fns = {"composed": composed, "fit_spheres": new} if a.route == "both" else {"fit_spheres": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        entry = {"first_call_ms": first, "n_spheres": int(out[5].item()), "counts": out[2].cpu().tolist(),
                 "radii": [round(v, 4) for v in out[1][:, 3].cpu().tolist()], "rmse": [round(v, 5) for v in out[3].cpu().tolist()],
                 "refit_used": out[4].cpu().tolist(), "best_count": out[8].cpu().tolist()}
        times = {name: [] for name in fns}
        for _ in range(a.reps):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.current_stream().synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        if comp:
            entry["composed_counts_last"] = comp["counts"]
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        if comp:
            entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["fit_spheres_ms"]["median"], 2)
            entry["median_below_composed_min"] = bool(entry["fit_spheres_ms"]["median"] < entry["composed_ms"]["min"])
        res["spheres"][str(P)] = entry
        del out, ws
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))
    bad = [P for P, e in res["spheres"].items() if e.get("median_below_composed_min") is False]
    if bad:
        raise SystemExit(f"the call's median is not below the composition's minimum at P = {bad}")


if __name__ == "__main__":
    main()
