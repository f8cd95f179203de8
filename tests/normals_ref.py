"""TEST REFERENCE for the surface normals of a prepared model (pcreg_model_normals_f32's contract in include/pcreg.h).

Neighbours come from knn_k_ref.knn(model, model, k), the fp32 brute force with (distance, row) ties; an entry at a non-finite
distance is no neighbour (a non-finite row is never one, and has none).  The mean and the six sums of centred products are taken
in numpy.longdouble, the eigen-decomposition by numpy.linalg.eigh in float64.  Nothing here restates the library's Jacobi.

normals(model, k, viewpoint=None) -> dict with, per row,
  n        [M]     the neighbours found
  normal   [M, 3]  float64 unit normal UP TO SIGN (eigh's), NaN where there is none
  variation[M]     lambda_min / (lambda_0 + lambda_1 + lambda_2)
  gap      [M]     g = (lambda_1 - lambda_0) / ||C||_F, the relative gap that conditions the direction
  big      [M]     the difference between the two largest |components| of the normal (decides the sign without a viewpoint)
  toward   [M]     n . (v - p) / |v - p| for the viewpoint v (decides the sign with one); NaN without a viewpoint
oriented(ref, viewpoint) applies the contract's sign rule to the reference normals.
families() are the clouds the GPU test and the exclusion-share check use.
"""
from __future__ import annotations

import numpy as np

import knn_k_ref

M_FAMILY = 2048
KS = (3, 4, 5, 8, 9, 16, 17, 32)          # every list size of the kernel (4, 8, 16, 32) and both sides of each boundary
OFFSET = np.array([100.0, 50.0, 90.0])
GAP_MIN = 1e-3                            # rows with a smaller relative gap are not compared in direction
EXCLUDED_CAP = 0.04                       # ... and may be at most this share of any (family, k)


def family(name: str, M: int = M_FAMILY) -> np.ndarray:
    rng = np.random.default_rng(1)
    if name == "sheet":
        u = rng.uniform(0, 40, (M, 2))
        z = 3 * np.sin(u[:, 0] / 5) * np.cos(u[:, 1] / 7) + rng.normal(0, 0.05, M)
        pts = np.column_stack([u, z])
    elif name == "volume":
        pts = rng.uniform(0, 20, (M, 3))
    else:
        raise KeyError(name)
    return (pts + OFFSET).astype(np.float32)


def families():
    return {name: family(name) for name in ("sheet", "volume")}


def normals(model, k: int, viewpoint=None) -> dict:
    m = np.asarray(model, np.float32).reshape(-1, 3)
    M = len(m)
    out = dict(n=np.zeros(M, np.int64), normal=np.full((M, 3), np.nan), variation=np.full(M, np.nan), gap=np.full(M, np.nan),
               big=np.full(M, np.nan), toward=np.full(M, np.nan))
    if M == 0:
        return out
    idx, dist = knn_k_ref.knn(m, m, k)
    finite_row = np.isfinite(m).all(axis=1)
    valid = (idx >= 0) & np.isfinite(dist) & finite_row[:, None]
    valid &= finite_row[np.clip(idx, 0, M - 1)]
    n = valid.sum(axis=1)
    out["n"] = n
    w = valid[:, :, None].astype(np.longdouble)
    pts = np.where(valid[:, :, None], m[np.clip(idx, 0, M - 1)], np.float32(0)).astype(np.longdouble)       # [M, k, 3]
    nn = np.maximum(n, 1).astype(np.longdouble)[:, None]
    mean = pts.sum(axis=1) / nn
    cen = (pts - mean[:, None, :]) * w
    Cm = np.zeros((M, 3, 3), np.longdouble)
    for a in range(3):
        for b in range(3):
            Cm[:, a, b] = (cen[:, :, a] * cen[:, :, b]).sum(axis=1)
    C64 = Cm.astype(np.float64)
    lam, vec = np.linalg.eigh(C64)                                      # ascending
    tr = lam.sum(axis=1)
    ok = (n >= 3) & (np.trace(C64, axis1=1, axis2=2) > 0)
    fro = np.sqrt((C64 * C64).sum(axis=(1, 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["normal"][ok] = vec[ok, :, 0]
        out["variation"][ok] = (lam[:, 0] / tr)[ok]
        out["gap"][ok] = ((lam[:, 1] - lam[:, 0]) / fro)[ok]
        a = np.sort(np.abs(out["normal"]), axis=1)
        out["big"] = a[:, 2] - a[:, 1]
        if viewpoint is not None:
            d = np.asarray(viewpoint, np.float64)[None, :] - m.astype(np.float64)
            out["toward"] = (out["normal"] * d).sum(axis=1) / np.sqrt((d * d).sum(axis=1))
    return out


def oriented(ref: dict, model, viewpoint=None) -> np.ndarray:
    """the reference normals with the contract's sign: towards the viewpoint, or the largest |component| (first of equals) >= 0"""
    nrm = ref["normal"].copy()
    if viewpoint is not None:
        d = np.asarray(viewpoint, np.float64)[None, :] - np.asarray(model, np.float32).reshape(-1, 3).astype(np.float64)
        flip = (nrm * d).sum(axis=1) < 0
    else:
        with np.errstate(invalid="ignore"):
            j = np.argmax(np.abs(np.nan_to_num(nrm)), axis=1)           # (argmax takes the first of equals)
        flip = nrm[np.arange(len(nrm)), j] < 0
    nrm[flip] = -nrm[flip]
    return nrm


def excluded_share(ref: dict) -> float:
    has = np.isfinite(ref["gap"])
    return float((ref["gap"][has] < GAP_MIN).mean()) if has.any() else 0.0
