"""Timing of the voxel-grid average downsampling on resident tensors: one JSON line.

n uniformly random points in a cube (10^6 and 10^7), the step chosen for about 8 points per voxel and once for about 1.
Timed after warm-up with a host clock around a stream synchronise, buffers allocated once:
  downsample   pcreg_amd.device.downsample_grid (out, count and label)
  copy         a plain device copy (Tensor.copy_) of 1 GiB, past the Infinity Cache, and one of the cloud's own 12 n bytes:
               the achieved copy bandwidth of this box, bytes read + bytes written over the time
Beside the time per call stands the time the bytes alone would take at the 1 GiB copy's bandwidth: the cloud read once and a
(key, row) record of 12 bytes read and written once per live sort pass, n * (12 + passes * 2 * 12) bytes.  passes is the number
of 8-bit digit passes that move data: ceil(used key bits / 8), the used bits restated here from the contract (the bits of the
largest cell index per axis; no row of these clouds is dead).  There is no threshold: the figures are a record.

    python3 scripts/downsample_bench.py [--reps 20] [--warmup 3] [--ns 1000000,10000000] [--per-voxel 8,1]
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

from pcreg_amd._lib import lib  # noqa: E402
from pcreg_amd.device import downsample_grid  # noqa: E402

BOX = 100.0


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.current_stream().synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    v = np.array(ts)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4),
            "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 4)}


def copy_gbs(nbytes, dev, reps, warmup):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), reps, warmup)
    return 2.0 * nbytes / (t["median"] * 1e-3) / 1e9, t


def live_passes(pts: torch.Tensor, step: float) -> tuple[int, int]:
    lo, hi = pts.min(dim=1).values.double(), pts.max(dim=1).values.double()
    cmax = torch.floor((hi - lo) / step).long().tolist()
    used = sum(int(c).bit_length() for c in cmax)
    return used, (used + 7) // 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", type=str, default="1000000,10000000")
    ap.add_argument("--per-voxel", type=str, default="8,1")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    big_gbs, big_t = copy_gbs(1 << 30, dev, a.reps, a.warmup)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "copy_1GiB": {"GBps": round(big_gbs, 1), "ms": big_t}, "cases": []}
    for n in [int(x) for x in a.ns.split(",")]:
        g = torch.Generator(device="cpu").manual_seed(n)
        pts = (torch.rand((3, n), generator=g, dtype=torch.float32) * BOX).to(dev)
        own_gbs, own_t = copy_gbs(12 * n, dev, a.reps, a.warmup)
        ws = torch.empty(max(int(L.pcreg_dev_downsample_grid_workspace(n)), 256), dtype=torch.uint8, device=dev)
        out = (torch.empty((3, n), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev), ws)
        for pv in [float(x) for x in a.per_voxel.split(",")]:
            step = BOX / (n / pv) ** (1.0 / 3.0)
            t = timed(lambda: downsample_grid(pts, step, out=out), a.reps, a.warmup)
            n_out, info = int(out[3].item()), int(out[4].item())
            if info != 0 or n_out <= 0 or int(out[1][:n_out].sum().item()) != n:
                raise SystemExit(f"n = {n}, step = {step}: info {info}, n_out {n_out}: not a valid result")
            used, passes = live_passes(pts, step)
            nbytes = n * (12 + passes * 2 * 12)
            bytes_ms = nbytes / (big_gbs * 1e9) * 1e3
            res["cases"].append({"n": n, "per_voxel_target": pv, "step": round(step, 6), "n_out": n_out, "per_voxel": round(n / n_out, 3),
                                 "key_bits": used, "passes": passes, "downsample_ms": t, "bytes": nbytes, "bytes_only_ms": round(bytes_ms, 4),
                                 "ratio": round(t["median"] / bytes_ms, 2), "copy_12n": {"GBps": round(own_gbs, 1), "ms": own_t},
                                 "workspace_bytes": int(ws.numel())})
        del pts, ws, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
