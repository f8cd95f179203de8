"""Timing of the farthest point sampling of a prepared model: one JSON line per case, then one for the run.

The bench model (bench.synth: uniform in the bench's box) at M = 50 k, 200 k and 1 M rows, K = 512 and 4096, start = -1, stop_d2 = 0.
Every case runs in a process of its own under its own `timeout`, and the driver stops at the first case that fails: nothing is
started on a device after a fault or a hang.  Per case, with a host clock around a stream synchronise after warm-up:
  culled     PreparedModel.farthest_points with buffers of its own: median / min / max ms per call, and per step
  head       the same call with K = 1, 8 and 64: what the first steps, which visit every row from one compute unit, cost
  nocull     the same call under the debug key "knn_nocull" (every tile and unit visited), fewer repetitions
  touched    the share of (live row, step) pairs measured, from "knn_stats" (pcreg_debug_fps_stats), culled and not
The culled and the un-culled call must agree in every bit; the script fails if they do not.

    python3 scripts/fps_bench.py [--Ms 50000,200000,1000000] [--Ks 512,4096] [--reps 7] [--nocull-reps 2] [--limit 240]
    python3 scripts/fps_bench.py --case M,K [--reps ..] [--nocull-reps ..]        (one case, in this process)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_case(M: int, K: int, reps: int, nocull_reps: int, warmup: int) -> dict:
    import torch
    from bench import synth
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import PreparedModel
    L, dev = lib(), torch.device("cuda", 0)
    model, _surf, _ = synth(M, 1000)
    mt = torch.from_numpy(np.ascontiguousarray(model.astype(np.float32).T)).to(dev)
    pm = PreparedModel(mt)
    ws = torch.empty(int(L.pcreg_dev_model_fps_workspace(M, K)), dtype=torch.uint8, device=dev)
    mk = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    out = (mk(K, torch.int32), mk(K, torch.float32), mk(1, torch.int32), mk(1, torch.float32), mk(M, torch.float32), mk(M, torch.int32),
           mk(1, torch.int32), ws)

    def timed(k, n):
        v = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pm.farthest_points(k, out=out)
            torch.cuda.current_stream().synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
        v = np.array(v)
        return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "reps": n}

    def counted(k):
        st = (C.c_longlong * 2)()
        check(L.pcreg_debug_set(b"knn_stats", 1))
        check(L.pcreg_debug_fps_stats(st, 1))
        pm.farthest_points(k, out=out)
        torch.cuda.synchronize()
        check(L.pcreg_debug_fps_stats(st, 1))
        check(L.pcreg_debug_set(b"knn_stats", 0))
        return int(st[0]), int(st[1])

    def snapshot():
        torch.cuda.synchronize()
        return [t.clone() for t in out[:6]]

    timed(K, warmup)
    res = {"M": M, "K": K, "device": torch.cuda.get_device_name(0)}
    res["culled_ms"] = timed(K, reps)
    a = snapshot()
    n = int(out[2].item())
    res["n_out"] = n
    res["culled_us_per_step"] = round(res["culled_ms"]["median"] * 1e3 / max(n, 1), 3)
    res["head_ms"] = {str(k): timed(k, reps)["median"] for k in (1, 8, 64)}
    steps, touched = counted(K)
    check(L.pcreg_debug_set(b"knn_nocull", 1))
    res["nocull_ms"] = timed(K, nocull_reps)
    b = snapshot()
    steps_all, touched_all = counted(K)
    check(L.pcreg_debug_set(b"knn_nocull", 0))
    res["nocull_us_per_step"] = round(res["nocull_ms"]["median"] * 1e3 / max(n, 1), 3)
    res.update(steps=steps, rows_touched=touched, rows_touched_nocull=touched_all, touched_share=round(touched / max(touched_all, 1), 5),
               speedup_median=round(res["nocull_ms"]["median"] / res["culled_ms"]["median"], 2))
    same = all(torch.equal(x.view(torch.int32)[:n] if i < 2 else x.view(torch.int32), y.view(torch.int32)[:n] if i < 2 else y.view(torch.int32))
               for i, (x, y) in enumerate(zip(a, b)))
    res["same_bits"] = bool(same) and steps == steps_all == n and touched_all == M * n
    pm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ms", type=str, default="50000,200000,1000000")
    ap.add_argument("--Ks", type=str, default="512,4096")
    ap.add_argument("--case", type=str, default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nocull-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take before it is ended")
    a = ap.parse_args()
    if a.case:
        M, K = (int(x) for x in a.case.split(","))
        res = run_case(M, K, a.reps, a.nocull_reps, a.warmup)
        print(json.dumps(res), flush=True)
        if not res["same_bits"]:
            raise SystemExit("the culled and the un-culled call disagree")
        return
    cases = []
    for M in (int(x) for x in a.Ms.split(",")):
        for K in (int(x) for x in a.Ks.split(",")):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", f"{M},{K}", "--reps", str(a.reps),
                   "--nocull-reps", str(a.nocull_reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            if r.returncode != 0 or not line.startswith("{"):
                print(json.dumps({"M": M, "K": K, "failed": r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
                raise SystemExit(f"case M = {M}, K = {K} ended with status {r.returncode}: nothing more is started")
            print(line, flush=True)
            cases.append(json.loads(line))
    print(json.dumps({"fps_bench": cases}))


if __name__ == "__main__":
    main()
