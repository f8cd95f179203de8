"""TEST REFERENCE for the statistical outlier removal of a prepared model (pcreg_model_denoise_f32's contract in include/pcreg.h).

Neighbours come from knn_k_ref.knn(model, model, k + 1), the fp32 brute force; an entry at a non-finite distance is no neighbour
(a non-finite row is never one, and has none).  The square roots, the row sums, mu, sd and thr are taken in numpy.longdouble, by
numpy's own summation.  Nothing here restates the library's summation tree; inliers_of() alone restates the contract's mask on
RETURNED doubles.

denoise(model, k, t) -> dict with
  n         [M]   the neighbours found, the row itself among them
  mean_dist [M]   longdouble mean distance to the n - 1 others, NaN where n <= 1
  nf, mu, sd, thr the statistic (longdouble; NaN where undefined)
  dmax            the largest finite mean distance
  inliers         the rows with mean_dist <= thr, ascending
  rel_gap         min |mean_dist - thr| / thr over the finite rows: how close any row lies to the threshold
families() are the clouds the GPU test uses: normals_ref's sheet and volume with 24 rows thrown far out, so that real outliers exist.
"""
from __future__ import annotations

import numpy as np

import knn_k_ref
import normals_ref

M_FAMILY = 2048
KS = (1, 3, 4, 7, 8, 15, 16, 31)          # every list size of the kernel (k + 1 <= 4, 8, 16, 32) and both sides of each boundary
TS = (0.0, 1.0, 2.5)
N_OUT = 24
GAP_MIN = 1e-7                            # no row of any case may lie this close (relatively) to the threshold


def family(name: str, M: int = M_FAMILY) -> np.ndarray:
    pts = normals_ref.family(name, M).copy()
    rng = np.random.default_rng(7)
    rows = rng.choice(M, N_OUT, replace=False)
    pts[rows] += rng.normal(0, 6, (N_OUT, 3)).astype(np.float32)
    return pts


def families():
    return {name: family(name) for name in ("sheet", "volume")}


def denoise(model, k: int, t: float) -> dict:
    m = np.asarray(model, np.float32).reshape(-1, 3)
    M = len(m)
    L = np.longdouble
    nan = L("nan")
    out = dict(n=np.zeros(M, np.int64), mean_dist=np.full(M, nan, L), nf=0, mu=nan, sd=nan, thr=nan, dmax=nan,
               inliers=np.zeros(0, np.int64), rel_gap=np.inf)
    if M == 0:
        return out
    idx, dist = knn_k_ref.knn(m, m, k + 1)
    finite_row = np.isfinite(m).all(axis=1)
    valid = (idx >= 0) & np.isfinite(dist) & finite_row[:, None]
    valid &= finite_row[np.clip(idx, 0, M - 1)]
    n = valid.sum(axis=1)
    roots = np.sqrt(np.where(valid, dist, np.float32(0)).astype(L))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(n >= 2, roots.sum(axis=1) / np.maximum(n - 1, 1).astype(L), nan)
    out["n"], out["mean_dist"] = n, d
    fin = np.isfinite(d)
    nf = int(fin.sum())
    out["nf"] = nf
    if nf == 0:
        return out
    mu = d[fin].sum() / L(nf)
    sd = np.sqrt(((d[fin] - mu) ** 2).sum() / L(nf - 1)) if nf > 1 else L(0)
    thr = mu + L(t) * sd
    out.update(mu=mu, sd=sd, thr=thr, dmax=d[fin].max())
    with np.errstate(invalid="ignore"):
        out["inliers"] = np.flatnonzero(d <= thr)
    if thr > 0:
        out["rel_gap"] = float((np.abs(d[fin] - thr) / thr).min())
    return out


def inliers_of(mean_dist, thr) -> np.ndarray:
    """the contract's mask restated on returned doubles: d_i <= thr, NaN on either side no inlier; ascending rows"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(mean_dist, np.float64) <= np.float64(thr))
