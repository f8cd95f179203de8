"""Timing of the FPFH descriptor from radius neighbourhoods on a prepared model: one JSON line.

A sheet of --M rows by this script's own seed (z = 3 sin(x / 5) cos(y / 7) + N(0, 0.05^2) over a square sized for 12.5 rows per
unit area, so that radii 1.13 and 2.26 hold about 50 and about 200 rows), normals from PreparedModel.normals(9) with a viewpoint
ONCE, outside the timed region.  Per radius, timed alternately in one process after warm-up, with a host clock around a stream
synchronise:
  count          PreparedModel.fpfh_radius_count                      (the radius search's count + scan, the rows as the queries)
  fill           PreparedModel.rangesearch_fill into buffers of its own (the radius search's fill + order alone)
  second_call    PreparedModel.fpfh_radius                            (fill + R1 + R2); R1 + R2 = second_call - fill
  lanes_4 / 16   the same call with the counting kernel at 4 and at 16 lanes a row ("fpfh_radius_lanes"); 64 is the default
  fpfh_k32       PreparedModel.fpfh(32), the k-nearest form, for orientation
  torch          a torch formulation of the same contract on the library's own lists (torch has no radius search): the pair
                 features of every (row, neighbour) pair in float64, the counts by index_add_ of one-hot rows, the weighting by
                 index_add_ of (c_j / m_j) / d2 -- floating-point atomics, so its sums are close to, not equal to, the call's; the
                 largest difference is reported.  Skipped above --torch-max-pairs list entries.
The kernel split of second_call (fill's kernels, R1, R2) comes from a kernel trace of `--route radius`, a run of its own.  No time is
fixed in advance.

    python3 scripts/fpfh_radius_bench.py [--reps 15] [--warmup 2] [--M 1000000] [--radii 1.13,2.26] [--max-neighbors 0] [--route all]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402

DENSITY = 12.5
VIEWPOINT = (120.0, 70.0, 4000.0)


def sheet(M: int, seed: int = 41) -> np.ndarray:
    rng = np.random.default_rng(seed)
    side = math.sqrt(M / DENSITY)
    u = rng.uniform(0, side, (M, 2))
    z = 3 * np.sin(u[:, 0] / 5) * np.cos(u[:, 1] / 7) + rng.normal(0, 0.05, M)
    return np.column_stack([u, z]).astype(np.float32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def torch_fpfh(rows, nrm, seg_off, idx, d2, max_neighbors):
    """rows, nrm [M, 3] float32; the library's lists -> out [M, 33] float64 (the contract, with sums in arrival order)"""
    M = rows.shape[0]
    cnt = (seg_off[1:] - seg_off[:-1])
    owner = torch.repeat_interleave(torch.arange(M, device=rows.device), cnt)
    pos = torch.arange(idx.numel(), device=rows.device) - seg_off[:-1][owner]
    nb = (d2 > 0) & torch.isfinite(d2)
    zeros = torch.zeros(M, dtype=torch.int64, device=rows.device).index_add_(0, owner, (~(d2 > 0)).long())
    if max_neighbors > 0:
        nb &= pos - zeros[owner] < max_neighbors
    i, j, w = owner[nb], idx[nb].long(), d2[nb].double()
    p, n = rows.double(), nrm.double()
    d, ni, nj = p[j] - p[i], n[i], n[j]
    ln = _dot(d, d).sqrt()
    ai, aj = _dot(ni, d) / ln, _dot(nj, d) / ln
    swap = ai.abs() < aj.abs()
    ns, nt = torch.where(swap[:, None], nj, ni), torch.where(swap[:, None], ni, nj)
    d = torch.where(swap[:, None], -d, d)
    f3 = torch.where(swap, -aj, ai)
    v = torch.linalg.cross(d, ns)
    vl = _dot(v, v).sqrt()
    v = v / vl[:, None]
    f2 = _dot(v, nt)
    f1 = torch.atan2(_dot(torch.linalg.cross(ns, v), nt), _dot(ns, nt))
    on = (ln > 0) & (vl > 0) & ~(torch.isnan(f1) | torch.isnan(f2) | torch.isnan(f3)) & torch.isfinite(ni).all(dim=1) & torch.isfinite(nj).all(dim=1)
    bins = torch.stack([(f1 + math.pi) / (2 * math.pi), (f2 + 1) * 0.5, (f3 + 1) * 0.5], dim=1)
    bins = torch.nan_to_num(torch.floor(11.0 * bins), nan=0.0).clamp_(0, 10).long() + torch.tensor([0, 11, 22], device=rows.device)
    counts = torch.zeros(M * 33, dtype=torch.float64, device=rows.device)
    counts.index_add_(0, (i[on, None] * 33 + bins[on]).reshape(-1), torch.ones(int(on.sum()) * 3, dtype=torch.float64, device=rows.device))
    counts = counts.view(M, 33)
    m = counts[:, :11].sum(dim=1)
    use = m[j] > 0
    acc = torch.zeros((M, 33), dtype=torch.float64, device=rows.device)
    acc.index_add_(0, i[use], (counts[j[use]] / m[j[use], None]) / w[use, None])
    S = acc.view(M, 3, 11).sum(dim=2, keepdim=True)
    out = torch.where(S > 0, acc.view(M, 3, 11) / torch.where(S > 0, S, torch.ones_like(S)) * 100.0, torch.zeros_like(S)).reshape(M, 33)
    out[~torch.isfinite(rows).all(dim=1)] = float("nan")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--radii", default="1.13,2.26")
    ap.add_argument("--max-neighbors", type=int, default=0)
    ap.add_argument("--torch-max-pairs", type=int, default=80_000_000)
    ap.add_argument("--route", choices=("all", "radius"), default="all")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model = sheet(a.M)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    rows = mt.t().contiguous()
    pm = PreparedModel(mt)
    nt = pm.normals(9, viewpoint=VIEWPOINT)                                   # once, outside the timed region
    nrows = nt.t().contiguous()
    torch.cuda.synchronize()
    M = pm.M
    res = {"M": M, "reps": a.reps, "warmup": a.warmup, "max_neighbors": a.max_neighbors, "device": torch.cuda.get_device_name(0), "radii": {}}
    for radius in [float(x) for x in a.radii.split(",")]:
        r2 = float(np.float32(radius * radius))
        _c, seg = pm.fpfh_radius_count(r2)
        total = int(seg[-1].item())
        need = max(int(L.pcreg_dev_model_fpfh_radius_workspace(M, total)), 256)
        out = (torch.empty((M, 33), dtype=torch.float64, device=dev), None, torch.empty(M, dtype=torch.int32, device=dev),
               torch.empty(need, dtype=torch.uint8, device=dev))
        idx, d2 = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.float32, device=dev)
        second = lambda: pm.fpfh_radius(r2, nt, seg, total, max_neighbors=a.max_neighbors, out=out)

        def with_lanes(n):
            def run():
                check(L.pcreg_debug_set(b"fpfh_radius_lanes", n))
                second()
                check(L.pcreg_debug_set(b"fpfh_radius_lanes", 0))
            return run

        fns = {"count": lambda: pm.fpfh_radius_count(r2), "fill": lambda: pm.rangesearch_fill(mt, r2, seg, idx, d2), "second_call": second}
        if a.route == "all":
            fns.update({"lanes_4": with_lanes(4), "lanes_16": with_lanes(16), "fpfh_k32": lambda: pm.fpfh(32, nt)})
        entry = {"list_entries": total, "list_bytes": 8 * total, "workspace_bytes": need}
        tref = {}
        if a.route == "all" and total <= a.torch_max_pairs:
            def torch_route():
                tref["out"] = torch_fpfh(rows, nrows, seg, idx, d2, a.max_neighbors)
            fns["torch"] = torch_route
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        entry["first_call_ms"] = first
        nn = out[2].cpu().numpy()
        entry["neighbors"] = {"mean": round(float(nn.mean()), 2), "min": int(nn.min()), "max": int(nn.max())}
        if tref:
            diff = (tref["out"] - out[0]).abs()
            entry["torch_max_abs_difference"] = float(diff[~torch.isnan(diff)].max().item())
        times = {name: [] for name in fns}
        for _ in range(a.reps):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.current_stream().synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        entry["r1_r2_ms_median"] = round(entry["second_call_ms"]["median"] - entry["fill_ms"]["median"], 3)
        res["radii"][str(radius)] = entry
        del out, idx, d2, tref
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
