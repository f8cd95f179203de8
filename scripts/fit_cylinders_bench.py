"""Timing of MSAC cylinder extraction on a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows) with three synthetic rods added by this script's own seed (radii 3, 2 and 1.5, lengths 40,
30 and 25, --rod-rows rows each, radial sigma 0.05), normals from PreparedModel.normals(12) ONCE, outside the timed region,
max_distance 0.5, B = 1000 trials, P = 1 and P = 4 cylinders, min_inliers 4.  Timed, alternately in one process after warm-up, with
a host clock around a stream synchronise:
  fit_cylinders  PreparedModel.fit_cylinders, buffers of its own
  composed       what the entry points before it allow, through torch: per round two random alive rows per trial, the trial
                 cylinders in float64 (the axis along n_0 x n_1, the axis point on the first row's normal line), the [rows] x
                 [trials] radial residuals as fp32 matrices per chunk of trials (chunked so that a chunk's matrix stays under
                 --chunk-mb), the truncated squared residuals summed per trial, argmin, the two-pass refit of its inliers in float64
                 (the axis from the normals' scatter by eigh, the circle by its 3 x 3 normal equations), the classification, ONE
                 host read per round (the inlier count, which decides whether to go on) and a boolean gather of the remaining rows
                 and normals
The composition is the baseline, not a restatement of the contract: its sums are floating point and its sampler is torch's, so
the two routes find cylinders of similar, not equal, size; the sizes are reported.  No time is fixed in advance.  --route
fit_cylinders runs the new call alone (for a kernel trace).

    python3 scripts/fit_cylinders_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--B 1000] [--cylinders 1,4] [--t 0.5] [--route both]
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

RODS = ((3.0, 40.0), (2.0, 30.0), (1.5, 25.0))


def with_rods(model: np.ndarray, rows_each: int, seed: int = 37) -> np.ndarray:
    """the model with three rods written over its last 3 * rows_each rows, centres inside its box, random axes"""
    rng = np.random.default_rng(seed)
    out = np.array(model, np.float32)
    lo, hi = out.min(axis=0).astype(np.float64), out.max(axis=0).astype(np.float64)
    at = len(out) - 3 * rows_each
    for k, (R, L) in enumerate(RODS):
        c = lo + (hi - lo) * rng.uniform(0.3, 0.7, 3)
        w = rng.normal(size=3)
        w /= np.linalg.norm(w)
        u = np.cross(w, np.eye(3)[int(np.argmin(np.abs(w)))])
        u /= np.linalg.norm(u)
        v = np.cross(w, u)
        th, hh = rng.uniform(0, 2 * np.pi, rows_each), rng.uniform(-L / 2, L / 2, rows_each)
        rad = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
        out[at + k * rows_each:at + (k + 1) * rows_each] = (c + hh[:, None] * w + rad * (R + rng.normal(0, 0.05, (rows_each, 1)))).astype(np.float32)
    return out[rng.permutation(len(out))]


def _radial(rows, a, w, R):
    """[nA, 3] rows against [C] cylinders (a, w [C, 3], R [C]) -> the radial residuals [nA, C] in fp32"""
    d = rows[:, None, :] - a[None, :, :]
    return torch.linalg.cross(d, w[None, :, :].expand_as(d)).norm(dim=2) - R[None, :]


def composed_cylinders(p, nrm, t, B, P, min_inliers, chunk, gen):
    """p, nrm: [M, 3] float32 on the device -> the inlier counts of the cylinders found"""
    t2 = float(np.float32(t) * np.float32(t))
    s = float(np.float32(2.0 ** 20 / t2))
    fin = torch.isfinite(p).all(dim=1)
    rows, nr = p[fin], nrm[fin]
    counts = []
    for _ in range(P):
        nA = rows.shape[0]
        if nA < 4:
            break
        pick = torch.randint(0, nA, (B, 2), device=p.device, generator=gen)
        q, n = rows[pick].double(), nr[pick].double()                          # [B, 2, 3]
        W = torch.linalg.cross(n[:, 0], n[:, 1])
        L2 = (W * W).sum(dim=1)
        w = W / L2.sqrt()[:, None]
        sc = (torch.linalg.cross(q[:, 1] - q[:, 0], n[:, 1]) * W).sum(dim=1) / L2
        a = q[:, 0] + sc[:, None] * n[:, 0]
        R = sc.abs() * n[:, 0].norm(dim=1)
        ok = (L2 > 0) & torch.isfinite(a).all(dim=1) & torch.isfinite(w).all(dim=1) & torch.isfinite(R) & (pick[:, 0] != pick[:, 1])
        af = torch.where(ok[:, None], a, torch.zeros_like(a)).float()
        wf = torch.where(ok[:, None], w, torch.zeros_like(w)).float()
        Rf = torch.where(ok, R, torch.zeros_like(R)).float()
        cost = torch.empty(B, dtype=torch.float64, device=p.device)
        cnt = torch.empty(B, dtype=torch.int64, device=p.device)
        for b0 in range(0, B, chunk):
            r = _radial(rows, af[b0:b0 + chunk], wf[b0:b0 + chunk], Rf[b0:b0 + chunk])   # [nA, chunk]
            r2 = r * r
            inl = r2 <= t2
            cost[b0:b0 + chunk] = torch.where(inl, r2 * s, torch.full_like(r2, 2.0 ** 20)).sum(dim=0, dtype=torch.float64)
            cnt[b0:b0 + chunk] = inl.sum(dim=0)
        cost = torch.where(ok & (cnt >= 4), cost, torch.full_like(cost, float("inf")))
        best = torch.argmin(cost)
        r = _radial(rows, af[best:best + 1], wf[best:best + 1], Rf[best:best + 1])[:, 0]
        inl = r * r <= t2
        ni = nr[inl].double()                                                 # pass 1: the axis minimises sum (n . w)^2
        ni = ni[torch.isfinite(ni).all(dim=1)]
        ax = torch.linalg.eigh(ni.t() @ ni).eigenvectors[:, 0]
        k = int(torch.argmin(ax.abs()).item())
        u = torch.linalg.cross(ax, torch.eye(3, dtype=torch.float64, device=p.device)[k])
        u = u / u.norm()
        v = torch.linalg.cross(ax, u)
        g = (rows[inl] - q[best, 0].float()).double()                          # pass 2: the circle, (x, y) . a + beta = x^2 + y^2
        xy = torch.stack([g @ u, g @ v], dim=1)
        A = torch.cat([xy, torch.ones_like(xy[:, :1])], dim=1)
        sol = torch.linalg.solve(A.t() @ A, A.t() @ (xy * xy).sum(dim=1))
        c2 = sol[:2] / 2
        R2 = (sol[2] + (c2 * c2).sum()).sqrt()
        centre = q[best, 0] + c2[0] * u + c2[1] * v
        r = _radial(rows, centre.float()[None, :], ax.float()[None, :], R2.float()[None])[:, 0]
        keep = ~(r * r <= t2)
        n_in = int((~keep).sum().item())                                      # the round's one host read
        if not bool(torch.isfinite(cost[best]).item()) or n_in < min_inliers:
            break
        counts.append(n_in)
        rows, nr = rows[keep], nr[keep]
    return counts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--cylinders", default="1,4")
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--rod-rows", type=int, default=2000)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--route", choices=("both", "fit_cylinders"), default="both")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = with_rods(model.astype(np.float32), a.rod_rows)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    rows = mt.t().contiguous()
    pm = PreparedModel(mt)
    nt = pm.normals(12)                                                       # once, outside the timed region
    nrows = nt.t().contiguous()
    torch.cuda.synchronize()
    M, B = pm.M, a.B
    chunk = max(1, min(B, (a.chunk_mb << 20) // (12 * M)))                    # (the cross product's [nA, chunk, 3] is the largest matrix)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    res = {"M": M, "B": B, "max_distance": a.t, "reps": a.reps, "warmup": a.warmup, "chunk_trials": chunk, "rod_rows": a.rod_rows,
           "device": torch.cuda.get_device_name(0), "cylinders": {}}
    for P in [int(x) for x in a.cylinders.split(",")]:
        i32, f64 = torch.int32, torch.float64
        ws = torch.empty(max(int(L.pcreg_dev_model_fit_cylinders_workspace(M, B)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty(M, dtype=i32, device=dev), torch.empty((P, 7), dtype=f64, device=dev), torch.empty((P, 2), dtype=f64, device=dev),
               torch.empty(P, dtype=i32, device=dev), torch.empty(P, dtype=f64, device=dev), torch.empty(P, dtype=i32, device=dev),
               torch.empty(1, dtype=i32, device=dev), torch.empty(P, dtype=i32, device=dev), torch.empty(P, dtype=torch.int64, device=dev),
               torch.empty(P, dtype=i32, device=dev), ws)
        new = lambda: pm.fit_cylinders(a.t, nt, max_cylinders=P, n_trials=B, min_inliers=4, seed=9, out=out)
        comp = {}

        def composed():
            comp["counts"] = composed_cylinders(rows, nrows, a.t, B, P, 4, chunk, gen)

        fns = {"composed": composed, "fit_cylinders": new} if a.route == "both" else {"fit_cylinders": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        entry = {"first_call_ms": first, "n_cylinders": int(out[6].item()), "counts": out[3].cpu().tolist(),
                 "radii": [round(v, 4) for v in out[1][:, 6].cpu().tolist()], "rmse": [round(v, 5) for v in out[4].cpu().tolist()],
                 "refit_used": out[5].cpu().tolist(), "best_count": out[9].cpu().tolist()}
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
            entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["fit_cylinders_ms"]["median"], 2)
            entry["median_below_composed_min"] = bool(entry["fit_cylinders_ms"]["median"] < entry["composed_ms"]["min"])
        res["cylinders"][str(P)] = entry
        del out, ws
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))
    bad = [P for P, e in res["cylinders"].items() if e.get("median_below_composed_min") is False]
    if bad:
        raise SystemExit(f"the call's median is not below the composition's minimum at P = {bad}")


if __name__ == "__main__":
    main()
