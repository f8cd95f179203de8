"""Brute-force fp32 k-nearest reference (tests/knn_k_ref.c), compiled on first use with -ffp-contract=off.

knn(query, model, k) -> (idx [Q, k] int32 0-based, -1 past M; dist [Q, k] float32 squared, +inf past M), ordered by
(distance, row) with ties to the lowest row: the contract of pcreg_knn_points_f32 and friends, which must match it bit for bit.
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
        out = os.path.join(tempfile.mkdtemp(prefix="knn_k_ref_"), "libknn_k_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-pthread",
                               os.path.join(_HERE, "knn_k_ref.c"), "-o", out, "-lm"])
        L = C.CDLL(out)
        L.knn_k_ref.restype = C.c_int
        _lib = L
    return _lib


def knn(query, model, k: int, threads: int | None = None):
    q = np.asfortranarray(np.asarray(query, np.float32).reshape(-1, 3))
    m = np.asfortranarray(np.asarray(model, np.float32).reshape(-1, 3))
    Q, M = q.shape[0], m.shape[0]
    idx = np.empty((max(Q, 1), k), np.int32)
    dist = np.empty((max(Q, 1), k), np.float32)
    if threads is None:
        threads = min(len(os.sched_getaffinity(0)), 16)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    qd = q if Q else np.zeros((1, 3), np.float32, order="F")
    md = m if M else np.zeros((1, 3), np.float32, order="F")
    rc = lib().knn_k_ref(qd.ctypes.data_as(f32p), Q, max(Q, 1), md.ctypes.data_as(f32p), M, max(M, 1), int(k),
                         idx.ctypes.data_as(i32p), dist.ctypes.data_as(f32p), int(threads))
    assert rc == 0, rc
    return idx[:Q].copy(), dist[:Q].copy()
