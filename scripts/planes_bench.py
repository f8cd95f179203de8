"""Timing of MSAC plane extraction on a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows), max_distance 0.5, B = 1000 trials, P = 1 and P = 4 planes, min_inliers 3.  Timed,
alternately in one process after warm-up, with a host clock around a stream synchronise:
  planes     PreparedModel.fit_planes, buffers of its own
  composed   what the entry points before it allow, through torch: per round three random alive rows per trial, the normals in
             float64, the [rows] x [trials] residuals as one fp32 matrix product per chunk of trials (chunked so that a chunk's
             matrix stays under --chunk-mb), the truncated squared residuals summed per trial, the best trial, the covariance of
             its inliers and torch.linalg.eigh, the classification, and ONE host read per round (the inlier count, which decides
             whether to go on and sizes the next round's rows)
The composition is the baseline, not a restatement of the contract: its sums are floating point and its sampler is torch's, so
the two routes find planes of similar, not equal, size; the sizes are reported.  No time is fixed in advance.  --route planes runs
the new call alone (for a kernel trace).

    python3 scripts/planes_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--B 1000] [--planes 1,4] [--t 0.5] [--route both]
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


def composed_planes(p, t, B, P, min_inliers, chunk, gen):
    """p: [M, 3] float32 on the device -> the inlier counts of the planes found"""
    t2 = float(np.float32(t) * np.float32(t))
    s = float(np.float32(2.0 ** 20 / t2))
    rows = p[torch.isfinite(p).all(dim=1)]
    counts = []
    for _ in range(P):
        nA = rows.shape[0]
        if nA < 3:
            break
        pick = torch.randint(0, nA, (B, 3), device=p.device, generator=gen)
        q = rows[pick].double()                                               # [B, 3, 3]
        c = torch.linalg.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        L = c.norm(dim=1)
        ok = (L > 0) & (pick[:, 0] != pick[:, 1]) & (pick[:, 0] != pick[:, 2]) & (pick[:, 1] != pick[:, 2])
        nrm = (c / L.clamp_min(1e-300)[:, None]).float()
        p0 = q[:, 0].float()
        off = (nrm * p0).sum(dim=1)
        cost = torch.empty(B, dtype=torch.float64, device=p.device)
        cnt = torch.empty(B, dtype=torch.int64, device=p.device)
        for b0 in range(0, B, chunk):
            r = rows @ nrm[b0:b0 + chunk].t() - off[None, b0:b0 + chunk]      # [nA, chunk]
            r2 = r * r
            inl = r2 <= t2
            cost[b0:b0 + chunk] = torch.where(inl, r2 * s, torch.full_like(r2, 2.0 ** 20)).sum(dim=0, dtype=torch.float64)
            cnt[b0:b0 + chunk] = inl.sum(dim=0)
        cost = torch.where(ok & (cnt >= 3), cost, torch.full_like(cost, float("inf")))
        best = torch.argmin(cost)
        r = (rows - p0[best]) @ nrm[best]
        d = (rows[r * r <= t2] - p0[best]).double()
        mean = d.mean(dim=0)
        cov = (d - mean).t() @ (d - mean)
        _w, V = torch.linalg.eigh(cov)
        n2 = V[:, 0].float()
        centre = (p0[best].double() + mean).float()
        r = (rows - centre) @ n2
        keep = r * r > t2
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
    ap.add_argument("--planes", default="1,4")
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--route", choices=("both", "planes"), default="both")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = model.astype(np.float32)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    rows = mt.t().contiguous()
    pm = PreparedModel(mt)
    M, B = pm.M, a.B
    chunk = max(1, min(B, (a.chunk_mb << 20) // (4 * M)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    res = {"M": M, "B": B, "max_distance": a.t, "reps": a.reps, "warmup": a.warmup, "chunk_trials": chunk, "device": torch.cuda.get_device_name(0),
           "planes": {}}
    for P in [int(x) for x in a.planes.split(",")]:
        i32, f64 = torch.int32, torch.float64
        ws = torch.empty(max(int(L.pcreg_dev_model_fit_planes_workspace(M, B)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty(M, dtype=i32, device=dev), torch.empty((P, 4), dtype=f64, device=dev), torch.empty((P, 3), dtype=f64, device=dev),
               torch.empty(P, dtype=i32, device=dev), torch.empty(P, dtype=f64, device=dev), torch.empty(1, dtype=i32, device=dev),
               torch.empty(P, dtype=i32, device=dev), torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=i32, device=dev), ws)
        new = lambda: pm.fit_planes(a.t, max_planes=P, n_trials=B, min_inliers=3, seed=9, out=out)
        comp = {}

        def composed():
            comp["counts"] = composed_planes(rows, a.t, B, P, 3, chunk, gen)

        fns = {"composed": composed, "planes": new} if a.route == "both" else {"planes": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        entry = {"first_call_ms": first, "n_planes": int(out[5].item()), "counts": out[3].cpu().tolist(), "rmse": [round(v, 5) for v in out[4].cpu().tolist()],
                 "best_count": out[8].cpu().tolist()}
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
            entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["planes_ms"]["median"], 2)
            entry["median_below_composed_min"] = bool(entry["planes_ms"]["median"] < entry["composed_ms"]["min"])
        res["planes"][str(P)] = entry
        del out, ws
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))
    bad = [P for P, e in res["planes"].items() if e.get("median_below_composed_min") is False]
    if bad:
        raise SystemExit(f"the call's median is not below the composition's minimum at P = {bad}")


if __name__ == "__main__":
    main()
