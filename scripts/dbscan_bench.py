"""Timing of DBSCAN against a prepared model: one JSON line.

On the bench model (bench.synth: 1 M rows), for r = 0.5, 1, 2 and minpts = 1, 4, 16: the median device-event time of 20 dbscan
calls after warm-up; in the same process, alternating with them, the yardsticks at the same r2: (a) the cluster call
(DESIGN 4.11), (b) the count-only radius search of the model against itself.  Per setting also the core, border and noise rows and
the clusters found.  The structure says dbscan <= 2 (b) + (a): a full count walk, a half walk with unions, and a border walk that
scores no more pairs than the count walk; "within" records whether the medians say so.

    python3 scripts/dbscan_bench.py [--reps 20] [--warmup 5] [--out profiles/dbscan_bench.json]
    python3 scripts/dbscan_bench.py --calls-only 3 --r 1 --minpts 4      # a few calls and nothing else, for a kernel trace
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import lib  # noqa: E402
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


def _buffers(pm):
    L, M = lib(), pm.M
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=DEV)
    ws = lambda n: torch.empty(max(int(n), 256), dtype=torch.uint8, device=DEV)
    db = (i32(M), i32(1), torch.empty(M, dtype=torch.uint8, device=DEV), i32(M), i32(M), i32(M), ws(L.pcreg_dev_model_dbscan_workspace(M)))
    cl = (i32(M), i32(1), i32(M), i32(M), ws(L.pcreg_dev_model_cluster_workspace(M)))
    rc = (i32(M), torch.empty(M + 1, dtype=torch.int64, device=DEV), ws(L.pcreg_dev_model_range_workspace(M, M)))
    return db, cl, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--r", type=float, default=1.0)
    ap.add_argument("--minpts", type=int, default=4)
    a = ap.parse_args()
    model = synth(1_000_000, 50_000)[0]
    t = torch.from_numpy(np.ascontiguousarray(model.T)).to(DEV)
    pm = PreparedModel(t)
    db, cl, rc = _buffers(pm)
    if a.calls_only:
        r2 = float(np.float32(a.r) ** 2)
        for _ in range(a.calls_only):
            pm.dbscan(r2, a.minpts, out=db)
            pm.cluster(r2, out=cl)
            pm.rangesearch_count(t, r2, out=rc)
        torch.cuda.synchronize()
        pm.close()
        return
    res = {"M": pm.M, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for r in (0.5, 1.0, 2.0):
        r2 = float(np.float32(r) ** 2)
        for minpts in (1, 4, 16):
            tm = _medians_ms({"dbscan_ms": lambda: pm.dbscan(r2, minpts, out=db), "cluster_ms": lambda: pm.cluster(r2, out=cl),
                              "range_count_self_ms": lambda: pm.rangesearch_count(t, r2, out=rc)}, a.reps, a.warmup)
            pm.dbscan(r2, minpts, out=db)
            torch.cuda.synchronize()
            label, nc, core = db[0], int(db[1].item()), db[2]
            n_core = int(core.sum().item())
            n_noise = int((label < 0).sum().item())
            bound = 2.0 * tm["range_count_self_ms"] + tm["cluster_ms"]
            tm.update(core=n_core, border=pm.M - n_core - n_noise, noise=n_noise, clusters=nc, bound_ms=round(bound, 4),
                      within=bool(tm["dbscan_ms"] <= bound))
            res[f"r{r:g}_minpts{minpts}"] = tm
    pm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
