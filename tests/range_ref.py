"""Brute-force fp32 radius-search reference (tests/range_ref.c), compiled on first use with -ffp-contract=off.

rangesearch(query, model, r2) -> (seg_off [Q + 1] int64, idx [total] int32 0-based, dist [total] float32 squared): query i's
rows are seg_off[i] .. seg_off[i + 1], every model row whose chain distance is <= r2 (the SQUARED radius, compared in float32),
ordered by (distance, row) with ties to the lowest row: the contract of pcreg_range_points_f32 and friends, which must match it
bit for bit.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="range_ref_"), "librange_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-pthread",
                               os.path.join(_HERE, "range_ref.c"), "-o", out, "-lm"])
        L = C.CDLL(out)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.range_ref_count.restype = L.range_ref_fill.restype = C.c_int
        L.range_ref_count.argtypes = [vp, i, i, vp, i, i, f, vp, i]
        L.range_ref_fill.argtypes = [vp, i, i, vp, i, i, f, vp, vp, vp, i]
        _lib = L
    return _lib


def rangesearch(query, model, r2, threads: int | None = None):
    q = np.asfortranarray(np.asarray(query, np.float32).reshape(-1, 3))
    m = np.asfortranarray(np.asarray(model, np.float32).reshape(-1, 3))
    Q, M = q.shape[0], m.shape[0]
    r2 = float(np.float32(r2))
    assert r2 >= 0.0, "the squared radius is a number >= 0"
    if threads is None:
        threads = min(len(os.sched_getaffinity(0)), 16)
    qd = q if Q else np.zeros((1, 3), np.float32, order="F")
    md = m if M else np.zeros((1, 3), np.float32, order="F")
    counts = np.zeros(max(Q, 1), np.int32)
    rc = lib().range_ref_count(qd.ctypes.data, Q, max(Q, 1), md.ctypes.data, M, max(M, 1), r2, counts.ctypes.data, int(threads))
    assert rc == 0, rc
    seg_off = np.zeros(Q + 1, np.int64)
    np.cumsum(counts[:Q], dtype=np.int64, out=seg_off[1:])
    total = int(seg_off[Q])
    idx = np.zeros(max(total, 1), np.int32)
    dist = np.zeros(max(total, 1), np.float32)
    rc = lib().range_ref_fill(qd.ctypes.data, Q, max(Q, 1), md.ctypes.data, M, max(M, 1), r2, seg_off.ctypes.data, idx.ctypes.data,
                              dist.ctypes.data, int(threads))
    assert rc == 0, rc
    return seg_off, idx[:total].copy(), dist[:total].copy()
