"""Brute-force farthest point sampling reference (tests/fps_ref.c), compiled on first use with -ffp-contract=off.

fps(model, K, start=-1, stop_d2=0.0) -> a dict: idx [n_out] int32 0-based original rows in selection order, dist [n_out] float32
squared, n_out, cover_d2 (numpy float32), min_dist [M] float32, label [M] int32, info -- the contract of pcreg_model_fps_f32 and
friends (include/pcreg.h), which must match it bit for bit.  O(M K), no culling, no ordering.

family(name, M, seed) -> the clouds the tests share: "surface", "cube", "lattice", "clusters", "nonfinite", "overflow".
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
FAMILIES = ("surface", "cube", "lattice", "clusters", "nonfinite", "overflow")


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="fps_ref_"), "libfps_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               os.path.join(_HERE, "fps_ref.c"), "-o", out, "-lm"])
        L = C.CDLL(out)
        L.fps_ref.restype = C.c_int
        vp, i = C.c_void_p, C.c_int
        L.fps_ref.argtypes = [vp, i, i, i, i, C.c_float, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def fps(model, K: int, start: int = -1, stop_d2: float = 0.0) -> dict:
    m = np.asfortranarray(np.asarray(model, np.float32).reshape(-1, 3))
    M = m.shape[0]
    idx = np.full(max(K, 1), -7, np.int32)
    dist = np.full(max(K, 1), -7.0, np.float32)
    n, info = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    cover = np.full(1, -7.0, np.float32)
    md = np.full(max(M, 1), -7.0, np.float32)
    lab = np.full(max(M, 1), -7, np.int32)
    mm = m if M else np.zeros((1, 3), np.float32, order="F")
    rc = lib().fps_ref(mm.ctypes.data, M, max(M, 1), int(K), int(start), float(stop_d2), idx.ctypes.data, dist.ctypes.data, n.ctypes.data,
                       cover.ctypes.data, md.ctypes.data, lab.ctypes.data, info.ctypes.data)
    assert rc == 0, rc
    k = int(n[0])
    return dict(idx=idx[:k].copy(), dist=dist[:k].copy(), n_out=k, cover_d2=cover[0], min_dist=md[:M].copy(), label=lab[:M].copy(),
                info=int(info[0]))


def family(name: str, M: int = 4000, seed: int = 0) -> np.ndarray:
    """[M, 3] float32.  surface: a noisy height field; cube: uniform; lattice: an integer lattice with every point four times over,
    shuffled (massive ties and coincident rows; every distance exact); clusters: two far clusters; nonfinite: NaN / +-inf rows, row 0
    among them; overflow: an extent whose fp32 squares (and some differences) overflow."""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    if name == "surface":
        xy = rng.random((M, 2)) * [100.0, 56.0]
        z = 8.0 * np.sin(xy[:, 0] * 0.07) * np.cos(xy[:, 1] * 0.11) + rng.normal(0.0, 0.05, M)
        return np.column_stack([xy, z]).astype(np.float32)
    if name == "cube":
        return (rng.random((M, 3)) * 10.0 - 5.0).astype(np.float32)
    if name == "lattice":
        n = max(-(-M // 4), 1)
        side = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        pts = np.repeat(g, 4, axis=0)[:M].astype(np.float32)
        return pts[rng.permutation(M)]
    if name == "clusters":
        a = rng.normal(0.0, 1.0, (M // 2, 3))
        b = rng.normal(0.0, 1.0, (M - M // 2, 3)) + [4000.0, -2500.0, 900.0]
        return np.concatenate([a, b])[rng.permutation(M)].astype(np.float32)
    if name == "nonfinite":
        pts = (rng.random((M, 3)) * [50.0, 50.0, 5.0]).astype(np.float32)
        bad = np.unique(np.concatenate([[0], rng.choice(M, max(M // 20, 1), replace=False)])) if M else np.zeros(0, np.int64)
        vals = np.array([np.nan, np.inf, -np.inf], np.float32)
        for t, r in enumerate(bad):
            pts[r, t % 3] = vals[(t // 3) % 3]
        return pts
    if name == "overflow":
        pts = (rng.random((M, 3)) * 2.0 - 1.0).astype(np.float32)
        # about one row in twenty lies where squares (1e19) or differences (1e38) overflow; the rest spans 18 decades below
        scale = np.float32(10.0) ** rng.choice(np.array([0, 5, 10, 18, 19, 38], np.float32), M, p=[0.5, 0.2, 0.15, 0.1, 0.03, 0.02]).astype(np.float32)
        return (pts * scale[:, None] * np.float32(3.0)).astype(np.float32)
    raise ValueError(name)
