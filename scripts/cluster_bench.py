"""Timing of clusterPoints against a prepared model: one JSON line.

On the bench model (bench.synth: 1 M rows), for r = 0.5, 0.75, 1, 2, 4: median device-event times of 20 calls after warm-up of
the cluster call, with and without the "same root" early-out ("cluster_noskip"); in the same process, alternating with them,
the yardsticks: (a) the k = 1 search with the model as its own queries, (b) one count + fill radius search with the model as its
own queries at r = 1.  Per r also the clusters found, the share of (tile, tile) pairs visited ("knn_stats") and the hits,
compare-and-swap attempts and failures of the union-find ("cluster_stats").  Then, on a 100 000-row subsample at r = 2: the
cluster call against (c) the frontier loop of clusterPoints.m over PreparedModel.rangesearch (one count + fill and one host read
per breadth-first level), wall-clock, with the two partitions compared.  Exits 1 if the cluster call is not the faster one.

    python3 scripts/cluster_bench.py [--reps 20] [--warmup 5] [--out profiles/cluster_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402

DEV = torch.device("cuda", 0)


def _time_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _medians_ms(fns, reps, warmup):
    """the calls alternate inside every repetition, so that all of them see the same clocks"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(_time_ms(fn))
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def _counters(fn):
    """-> visited share of the (tile, tile) pairs, [hits, compare-and-swaps, failed] of one call"""
    L = lib()
    knn, cl = (C.c_longlong * 4)(), (C.c_longlong * 4)()
    check(L.pcreg_debug_set(b"knn_stats", 1))
    check(L.pcreg_debug_set(b"cluster_stats", 1))
    check(L.pcreg_debug_knn_stats(knn, 1))
    check(L.pcreg_debug_cluster_stats(cl, 1))
    fn()
    torch.cuda.synchronize()
    check(L.pcreg_debug_knn_stats(knn, 1))
    check(L.pcreg_debug_cluster_stats(cl, 1))
    check(L.pcreg_debug_set(b"knn_stats", 0))
    check(L.pcreg_debug_set(b"cluster_stats", 0))
    return (round(knn[1] / knn[2], 4) if knn[2] else None), [int(cl[1]), int(cl[2]), int(cl[3])]


def _cluster_call(pm):
    M = pm.M
    out = tuple(torch.empty(n, dtype=torch.int32, device=DEV) for n in (M, 1, M, M)) + \
        (torch.empty(max(int(lib().pcreg_dev_model_cluster_workspace(M)), 256), dtype=torch.uint8, device=DEV),)
    return out, (lambda r2: pm.cluster(r2, out=out))


def full_model(pm, t, reps, warmup):
    L, M = lib(), pm.M
    res = {"M": M}
    out, cluster = _cluster_call(pm)
    knn_out = (torch.empty((M, 1), dtype=torch.int32, device=DEV), torch.empty((M, 1), dtype=torch.float32, device=DEV),
               torch.empty(int(L.pcreg_dev_model_knn_workspace(M, M, 1)), dtype=torch.uint8, device=DEV))
    ws = torch.empty(int(L.pcreg_dev_model_range_workspace(M, M)), dtype=torch.uint8, device=DEV)
    cnt = (torch.empty(M, dtype=torch.int32, device=DEV), torch.empty(M + 1, dtype=torch.int64, device=DEV), ws)
    pm.rangesearch_count(t, 1.0, out=cnt)
    total = int(cnt[1][-1].item())
    idx, dist = torch.empty(total, dtype=torch.int32, device=DEV), torch.empty(total, dtype=torch.float32, device=DEV)

    def range_pair():
        pm.rangesearch_count(t, 1.0, out=cnt)
        pm.rangesearch_fill(t, 1.0, cnt[1], idx, dist, ws=ws)
    yard = {"knn1_self_ms": lambda: pm.knn(t, 1, out=knn_out), "range_self_r1_ms": range_pair}
    res["range_self_r1_rows"] = total

    def noskip(r2):
        check(L.pcreg_debug_set(b"cluster_noskip", 1))
        cluster(r2)
        check(L.pcreg_debug_set(b"cluster_noskip", 0))
    for r in (0.5, 0.75, 1.0, 2.0, 4.0):
        r2 = float(np.float32(r) ** 2)
        tm = _medians_ms({"cluster_ms": lambda: cluster(r2), "cluster_noskip_ms": lambda: noskip(r2), **yard}, reps, warmup)
        cluster(r2)
        torch.cuda.synchronize()
        nc = int(out[1].item())
        visited, (hits, cas, failed) = _counters(lambda: cluster(r2))
        _, (hits_ns, cas_ns, failed_ns) = _counters(lambda: noskip(r2))
        tm.update(clusters=nc, largest=int(out[3][:nc].max().item()), visited=visited, hits=hits, cas=cas, cas_failed=failed,
                  noskip_cas=cas_ns, noskip_cas_failed=failed_ns,
                  to_knn1=round(tm["cluster_ms"] / tm["knn1_self_ms"], 3), to_range_pair=round(tm["cluster_ms"] / tm["range_self_r1_ms"], 3))
        res[f"r{r:g}"] = tm
    return res


def frontier_loop(pm, t, r2):
    """clusterPoints.m:16-45 over the device tier: -> label [M] (clusters numbered as they are found), the number of levels"""
    M = pm.M
    label = torch.full((M,), -1, dtype=torch.int64, device=DEV)
    unexplored = torch.ones(M, dtype=torch.bool, device=DEV)
    n, levels, start = 0, 0, 0
    while True:
        rest = torch.nonzero(unexplored[start:])[:1]
        if rest.numel() == 0:
            break
        start += int(rest.item())
        frontier = torch.tensor([start], device=DEV)
        unexplored[frontier] = False
        while frontier.numel():
            _, idx, _ = pm.rangesearch(t[:, frontier].contiguous(), r2)
            label[frontier] = n
            cand = torch.unique(idx.long())
            frontier = cand[unexplored[cand]]
            unexplored[frontier] = False
            levels += 1
        n += 1
    return label, n, levels


def subsample(model, reps):
    pts = np.ascontiguousarray(model[np.sort(np.random.default_rng(17).choice(len(model), 100_000, replace=False))])
    t = torch.from_numpy(np.ascontiguousarray(pts.T)).to(DEV)
    pm = PreparedModel(t)
    r2 = 4.0
    out, cluster = _cluster_call(pm)
    cluster(r2)
    frontier_loop(pm, t, r2)                                     # warm-up of both
    torch.cuda.synchronize()
    tc, tf = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        cluster(r2)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        label, n, levels = frontier_loop(pm, t, r2)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tc.append(1e3 * (t1 - t0)); tf.append(1e3 * (t2 - t1))
    same = bool((label.to(torch.int32) == out[0]).all().item()) and n == int(out[1].item())   # both number the clusters by their first row
    pm.close()
    c, f = float(np.median(tc)), float(np.median(tf))
    return {"M": len(pts), "r": 2.0, "cluster_ms": round(c, 4), "frontier_loop_ms": round(f, 3), "speedup": round(f / c, 1), "clusters": n,
            "levels": levels, "same_partition": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frontier-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = synth(1_000_000, 50_000)[0]
    t = torch.from_numpy(np.ascontiguousarray(model.T)).to(DEV)
    pm = PreparedModel(t)
    res = {"bench_model": full_model(pm, t, a.reps, a.warmup)}
    pm.close()
    res["subsample"] = subsample(model, a.frontier_reps)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ok = res["subsample"]["same_partition"] and res["subsample"]["cluster_ms"] < res["subsample"]["frontier_loop_ms"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
