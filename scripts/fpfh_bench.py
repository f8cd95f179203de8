"""Timing of the FPFH descriptors of a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows), k = 8 and k = 16, the normals precomputed (PreparedModel.normals at k = 9 towards a
viewpoint).  Timed, alternately in one process after warm-up, with a host clock around a stream synchronise:
  fpfh       PreparedModel.fpfh (descriptors and SPFH counts), buffers of its own
  composed   what the entry points before it allow: PreparedModel.knn of the model against itself (an [M][k] table), torch gathers
             of the [M][k][6] coordinates and normals, the pair features in torch float64, a binned scatter_add into [M][33]
             counts, a gather of the neighbours' [M][k][33] counts, the weighted sum and the normalisation
Reported per k: median, min, max and interquartile range of each route, the share of rows whose counts agree (torch's atan2 and
its fused kernels round differently: a pair on a bin edge may differ), the largest difference of the outputs over the rows whose
own and whose neighbours' counts agree, and the share of tile visits the walk makes ("knn_stats").  No time is fixed in advance:
the composition is the baseline.  --max-seconds bounds the timed loop of one k.

    python3 scripts/fpfh_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--ks 8,16] [--k-normals 9] [--max-seconds 0]
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

from bench import synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def composed_fpfh(pm, mt, nt, k):
    """the contract through today's entry points; mt, nt: [3, M] float32 -> (out [M, 33] float64, counts [M, 33] int64)"""
    M = mt.shape[1]
    dev = mt.device
    idx, d2 = pm.knn(mt, k)                                                  # [M, k]
    nb = (idx >= 0) & torch.isfinite(d2) & (d2 > 0)
    j = idx.clamp_min(0).long()
    p, n = mt.t().double(), nt.t().double()                                  # [M, 3]
    d = p[j] - p[:, None, :]
    ni, nj = n[:, None, :].expand(M, k, 3), n[j]
    ln = dot(d, d).sqrt()
    ai, aj = dot(ni, d) / ln, dot(nj, d) / ln
    swap = (ai.abs() < aj.abs())[..., None]
    ns, ntg = torch.where(swap, nj, ni), torch.where(swap, ni, nj)
    d = torch.where(swap, -d, d)
    f3 = torch.where(swap[..., 0], -aj, ai)
    v = torch.linalg.cross(d, ns)
    vl = dot(v, v).sqrt()
    v = v / vl[..., None]
    w = torch.linalg.cross(ns, v)
    f2 = dot(v, ntg)
    f1 = torch.atan2(dot(w, ntg), dot(ns, ntg))
    x = torch.stack([(f1 + math.pi) / (2 * math.pi), (f2 + 1) * 0.5, (f3 + 1) * 0.5], dim=-1) * 11
    on = nb & (ln > 0) & (vl > 0) & ~torch.isnan(x).any(dim=-1) & torch.isfinite(ni).all(dim=-1) & torch.isfinite(nj).all(dim=-1)
    b = torch.nan_to_num(x).floor().clamp(0, 10).long() + torch.tensor([0, 11, 22], device=dev)
    counts = torch.zeros((M, 33), dtype=torch.int64, device=dev)
    for f in range(3):                                                       # the binned scatter
        counts.scatter_add_(1, b[..., f], on.long())
    mm = counts[:, :11].sum(dim=1)
    use = nb & (mm[j] > 0)
    wgt = torch.where(use, 1.0 / (mm[j].clamp_min(1).double() * d2.double()), torch.zeros((), dtype=torch.float64, device=dev))
    acc = (counts[j].double() * wgt[..., None]).sum(dim=1)                   # [M, 33]
    S = acc.view(M, 3, 11).sum(dim=2, keepdim=True)
    out = torch.where(S > 0, acc.view(M, 3, 11) / S.clamp_min(1e-300) * 100.0, torch.zeros((), dtype=torch.float64, device=dev)).view(M, 33)
    return out, counts, j, nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--ks", type=str, default="8,16")
    ap.add_argument("--k-normals", type=int, default=9)
    ap.add_argument("--max-seconds", type=float, default=0.0)
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = model.astype(np.float32)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    M = pm.M
    centre = model.astype(np.float64).mean(axis=0)
    nt = pm.normals(a.k_normals, viewpoint=(centre[0], centre[1], centre[2] + 1000.0)).clone()
    res = {"M": M, "k_normals": a.k_normals, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "k": {}}
    for k in [int(x) for x in a.ks.split(",")]:
        ws = torch.empty(max(int(L.pcreg_dev_model_fpfh_workspace(M, k)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty((M, 33), dtype=torch.float64, device=dev), torch.empty((M, 33), dtype=torch.uint8, device=dev), ws)
        new = lambda: pm.fpfh(k, nt, spfh=True, out=out)
        comp = {}

        def composed():
            comp["out"], comp["counts"], comp["j"], comp["nb"] = composed_fpfh(pm, mt, nt, k)

        fns = {"composed": composed, "fpfh": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        same = (out[1].long() == comp["counts"]).all(dim=1)
        clean = same & (same[comp["j"]] | ~comp["nb"]).all(dim=1)
        diff = float((out[0][clean] - comp["out"][clean]).abs().max().item()) if bool(clean.any()) else None
        times = {name: [] for name in fns}
        t_loop = time.perf_counter()
        for _ in range(a.reps):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.current_stream().synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
            if a.max_seconds > 0 and time.perf_counter() - t_loop > a.max_seconds:
                break
        stats = (C.c_longlong * 4)()
        check(L.pcreg_debug_set(b"knn_stats", 1))
        check(L.pcreg_debug_knn_stats(stats, 1))
        new()
        torch.cuda.synchronize()
        check(L.pcreg_debug_knn_stats(stats, 1))
        check(L.pcreg_debug_set(b"knn_stats", 0))
        entry = {"reps_done": len(times["fpfh"]), "first_call_ms": first, "rows_with_equal_counts": float(same.double().mean().item()),
                 "rows_compared": float(clean.double().mean().item()), "max_abs_diff_on_compared_rows": diff,
                 "nan_rows": int(torch.isnan(out[0]).any(dim=1).sum().item()),
                 "visited_tiles": int(stats[1]), "nominal_tiles": int(stats[2]), "visited_share": round(stats[1] / stats[2], 5) if stats[2] else None}
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["fpfh_ms"]["median"], 2)
        res["k"][str(k)] = entry
        del comp, out, ws
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))
    bad = [k for k, e in res["k"].items() if e["rows_with_equal_counts"] < 0.999 or (e["max_abs_diff_on_compared_rows"] or 0.0) > 1e-9]
    if bad:
        raise SystemExit(f"the new call and the composition disagree at k = {bad}")


if __name__ == "__main__":
    main()
