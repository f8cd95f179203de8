"""Timing of the ISS keypoints of a prepared model: one JSON line.

The bench model (bench.synth, 1 M rows) at salient radii that give a median neighbourhood near 30 and near 100 rows (1.6 and 2.4
for the model's 1.79 rows per cubic unit), the nonmax radius two thirds of the salient one, thresholds 0.975, five neighbours.
Timed, alternately in one process after warm-up, with a host clock around a stream synchronise:
  iss        PreparedModel.iss_keypoints, buffers of its own
  composed   what the entry points before it allow: PreparedModel.rangesearch of the model against itself (count and fill, one
             read of the total on the host), a torch gather of the differences, the contract's integers q = rint(dx 2^(18 - e)) as
             float64 (their sums are exact below 2^53, so both routes decide the SAME contract; the centred form of the sums would
             add a gather and a segment sum), index_add segment sums of 1, q and the six products, N = n S2 - S1 S1^T,
             torch.linalg.eigvalsh, the tests; a second rangesearch at the nonmax radius and scatter_reduce segment maxima for
             the suppression with the tie rule
Reported per radius: median, min, max and interquartile range of each route; whether n_neighbors agree on every row; the rows
the reference rule excludes (a ratio test within 1e-9 mu1 of equality, a candidate nonmax neighbour within 1e-9 in saliency that is
no exact tie, or such a neighbour) and whether the keypoint sets agree outside them; the share of tile visits both walks make
("knn_stats").  No time is fixed in advance: the composition is the baseline.  --route iss runs the new call alone (for a kernel
trace).  --max-seconds bounds the timed loop of one radius.

    python3 scripts/iss_bench.py [--reps 25] [--warmup 3] [--M 1000000] [--radii 1.6,2.4] [--route both] [--max-seconds 0]
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
from pcreg_amd.api import iss_args  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402

TOL = 1e-9


def composed_iss(pm, mt, r2s, r2n, g21, g32, mn):
    """the contract through the entry points before it; mt: [3, M] float32 -> dict of device tensors"""
    M, dev = mt.shape[1], mt.device
    _f, e2 = math.frexp(r2s)
    e = -((-e2) // 2)
    scale = 2.0 ** (18 - e)
    seg, idx, _d = pm.rangesearch(mt, r2s)
    n = (seg[1:] - seg[:-1])
    row = torch.repeat_interleave(torch.arange(M, device=dev), n)
    j = idx.long()
    p = mt.t().contiguous()                                                  # [M, 3] float32
    q = torch.round((p[j] - p[row]).double() * scale)                        # fp32 differences, scaled exactly, to nearest even
    S = torch.zeros((M, 9), dtype=torch.float64, device=dev)
    prod = torch.stack([q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1],
                        q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], dim=1)
    S.index_add_(0, row, prod)
    nd = n.double()
    a, b = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)
    N6 = torch.stack([nd * S[:, 3 + k] - S[:, a[k]] * S[:, b[k]] for k in range(6)], dim=1)
    A = torch.stack([N6[:, 0], N6[:, 1], N6[:, 2], N6[:, 1], N6[:, 3], N6[:, 4], N6[:, 2], N6[:, 4], N6[:, 5]], dim=1).view(M, 3, 3)
    mu = torch.linalg.eigvalsh(A).flip(1)                                    # descending
    cand = (n >= mn) & (mu[:, 1] < g21 * mu[:, 0]) & (mu[:, 2] < g32 * mu[:, 1]) & (mu[:, 2] > 0)
    lam3 = (mu[:, 2] / (nd * nd)) * 4.0 ** -(18 - e)
    s = torch.where(cand, lam3, torch.zeros((), dtype=torch.float64, device=dev))
    seg2, idx2, _d2 = pm.rangesearch(mt, r2n)
    n2 = seg2[1:] - seg2[:-1]
    row2 = torch.repeat_interleave(torch.arange(M, device=dev), n2)
    j2 = idx2.long()
    sj = s[j2]
    smax = torch.zeros(M, dtype=torch.float64, device=dev).scatter_reduce_(0, row2, sj, "amax", include_self=True)
    top = sj == smax[row2]
    jmin = torch.full((M,), M, dtype=torch.int64, device=dev).scatter_reduce_(0, row2[top], j2[top], "amin", include_self=True)
    key = (s > 0) & (s == smax) & (jmin == torch.arange(M, device=dev))
    # the reference rule's exclusions
    sens = (n >= mn) & (((mu[:, 1] - g21 * mu[:, 0]).abs() <= TOL * mu[:, 0]) | ((mu[:, 2] - g32 * mu[:, 1]).abs() <= TOL * mu[:, 0])
                        | (mu[:, 2].abs() <= TOL * mu[:, 0]))
    si = s[row2]
    close = cand[row2] & cand[j2] & (row2 != j2) & ((si - sj).abs() <= TOL * torch.maximum(si, sj)) & ~((N6[row2] == N6[j2]).all(dim=1) & (n[row2] == n[j2]))
    sens = sens | torch.zeros(M, dtype=torch.bool, device=dev).index_put_((row2[close],), torch.ones((), dtype=torch.bool, device=dev))
    excl = sens.clone()
    hit = sens[j2]
    excl.index_put_((row2[hit],), torch.ones((), dtype=torch.bool, device=dev))
    return dict(n=n.int(), s=s, key=key, excluded=excl, pairs=int(idx.numel()), pairs_nonmax=int(idx2.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--radii", type=str, default="1.6,2.4")
    ap.add_argument("--route", choices=("both", "iss"), default="both")
    ap.add_argument("--max-seconds", type=float, default=0.0)
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(a.M, 1000)
    model = model.astype(np.float32)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    M = pm.M
    res = {"M": M, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "radius": {}}
    for rs in [float(x) for x in a.radii.split(",")]:
        rn = rs * 2.0 / 3.0
        r2s, r2n, g21, g32, mn = iss_args(rs, rn, 0.975, 0.975, 5)
        ws = torch.empty(max(int(L.pcreg_dev_model_iss_workspace(M)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty(M, dtype=torch.int32, device=dev), torch.empty((M, 3), dtype=torch.float64, device=dev),
               torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.int32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev), ws)
        new = lambda: pm.iss_keypoints(rs, rn, g21, g32, mn, out=out)
        comp = {}

        def composed():
            comp.update(composed_iss(pm, mt, r2s, r2n, g21, g32, mn))

        fns = {"composed": composed, "iss": new} if a.route == "both" else {"iss": new}
        first = {}
        for w in range(a.warmup):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if w == 0:
                    first[name] = round((time.perf_counter() - t0) * 1e3, 3)
        n_kp = int(out[4].item())
        entry = {"nonmax_radius": round(rn, 4), "first_call_ms": first, "keypoints": n_kp, "median_neighbours": float(out[0].float().median().item()),
                 "max_neighbours": int(out[0].max().item())}
        if comp:
            key = torch.zeros(M, dtype=torch.bool, device=dev)
            key[out[3][:n_kp].long()] = True
            keep = ~comp["excluded"]
            entry.update(n_neighbors_equal=bool((out[0] == comp["n"]).all().item()), rows_excluded=int(comp["excluded"].sum().item()),
                         keypoints_equal_outside_excluded=bool((key[keep] == comp["key"][keep]).all().item()),
                         keypoint_rows_that_differ=int((key != comp["key"]).sum().item()),
                         max_rel_saliency_diff=float(((out[2] - comp["s"]).abs() / comp["s"].clamp_min(1e-300)).max().item()),
                         pairs_listed=comp["pairs"], pairs_listed_nonmax=comp["pairs_nonmax"])
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
        entry.update(reps_done=len(times["iss"]), visited_tiles=int(stats[1]), nominal_tiles=int(stats[2]),
                     visited_share=round(stats[1] / stats[2], 5) if stats[2] else None)
        for name, v in times.items():
            v = np.array(v)
            entry[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                   "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
        if comp:
            entry["speedup_median"] = round(entry["composed_ms"]["median"] / entry["iss_ms"]["median"], 2)
        res["radius"][str(rs)] = entry
        comp.clear()
        del out, ws
        torch.cuda.empty_cache()
    pm.close()
    print(json.dumps(res))
    bad = [r for r, e in res["radius"].items() if e.get("n_neighbors_equal") is False or e.get("keypoints_equal_outside_excluded") is False]
    if bad:
        raise SystemExit(f"the new call and the composition disagree at radius {bad}")


if __name__ == "__main__":
    main()
