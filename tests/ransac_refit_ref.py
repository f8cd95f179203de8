"""Host reference for ONE RANSAC refit: estimateTransform.m's >= 4-point, full-rank path with effectively exact sums.

T = refit_reference(p1, p2, rows) is the transform of the correspondences `rows` (0-based) in the library's convention
[p2, 1] T = [p1, 1], T = [R 0; t 1] (conftest.rigid_case).  The formula is the reference's: centroids cd, cm of the
p1 / p2 rows, H = sum (m - cm) (d - cd)^T = sum m d^T - (sum m)(sum d)^T / K, H = U S V^T, R = V U^T (no reflection
fix, estimateTransform.m:62), t = cd - R cm.

Arithmetic.  Every product m_i d_j is split without error into a rounded product and its rounding error (Veltkamp's
split, Dekker's product).  The sums -- of both halves of the products, and of the coordinates -- are taken with
math.fsum, which rounds the exact sum once; fsum is applied again to the terms and the negated partial results until
the remainder is exactly zero, so the partial results add up to the exact sum.  The centring and the division by K
are done in fractions.Fraction on those fifteen sums.  H and the centroids are rounded to fp64 ONCE; what follows is
numpy's SVD of a 3 x 3 matrix and a 3 x 3 product.  No origin is subtracted anywhere, so the accuracy does not depend
on where any row lies: an outlier of 10^8 times the inlier extent in the input changes nothing, because it is not in `rows`.

The helper serves inlier sets of at least four rows and rank 3 only (the N == 3 branch and the rank decisions have
their own tests); it asserts both.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

_SPLITTER = 134217729.0       # 2^27 + 1 (Veltkamp)


def _split(a: np.ndarray):
    c = _SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a: np.ndarray, b: np.ndarray):
    """p, e with p = fl(a b) and p + e = a b exactly (Dekker), elementwise; no overflow / underflow at the sizes of point clouds."""
    p = a * b
    ah, al = _split(a); bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_sum(*arrays) -> Fraction:
    """The exact sum of all the fp64 values given, as a Fraction: correctly rounded partial sums (math.fsum) until nothing is left."""
    terms = [float(v) for a in arrays for v in np.asarray(a, dtype=np.float64).ravel()]
    assert all(math.isfinite(v) for v in terms)
    total = Fraction(0)
    for _ in range(64):
        s = math.fsum(terms)
        if s == 0.0:              # the correctly rounded sum is zero only if the sum is
            return total
        total += Fraction(s)
        terms.append(-s)
    raise AssertionError("exact_sum did not terminate")


def refit_moments(p1, p2, rows):
    """(H, cd, cm, K): H [3, 3] with H[i, j] = sum (m_i - cm_i)(d_j - cd_j) over `rows` (m = p2, d = p1), and the two
    centroids, each entry the exact value rounded to fp64 once."""
    rows = np.asarray(rows, dtype=np.int64)
    d = np.ascontiguousarray(np.asarray(p1, dtype=np.float64)[rows]); m = np.ascontiguousarray(np.asarray(p2, dtype=np.float64)[rows])
    K = len(rows)
    sd = [exact_sum(d[:, c]) for c in range(3)]
    sm = [exact_sum(m[:, c]) for c in range(3)]
    H = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            p, e = two_prod(m[:, i], d[:, j])
            H[i, j] = float(exact_sum(p, e) - sm[i] * sd[j] / K)
    cd = np.array([float(s / K) for s in sd]); cm = np.array([float(s / K) for s in sm])
    return H, cd, cm, K


def refit_moments_fractions(p1, p2, rows):
    """The same quantities by brute force: every coordinate a Fraction, every operation exact (for small inputs)."""
    rows = [int(r) for r in rows]
    K = len(rows)
    d = [[Fraction(float(p1[r][c])) for c in range(3)] for r in rows]
    m = [[Fraction(float(p2[r][c])) for c in range(3)] for r in rows]
    cd = [sum(x[c] for x in d) / K for c in range(3)]
    cm = [sum(x[c] for x in m) / K for c in range(3)]
    H = np.array([[float(sum((m[k][i] - cm[i]) * (d[k][j] - cd[j]) for k in range(K))) for j in range(3)] for i in range(3)])
    return H, np.array([float(v) for v in cd]), np.array([float(v) for v in cm]), K


def transform_from_moments(H, cd, cm):
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T                                # estimateTransform.m:62
    T = np.eye(4)
    T[:3, :3] = R.T
    T[3, :3] = cd - R @ cm                        # :63
    return T


def refit_reference(p1, p2, rows):
    from oracle import pcreg_oracle as o
    rows = np.asarray(rows, dtype=np.int64)
    assert len(rows) >= 4, "the reference serves the >= 4-point path only"
    assert o.matlab_rank(np.asarray(p1, dtype=np.float64)[rows]) == 3 and o.matlab_rank(np.asarray(p2, dtype=np.float64)[rows]) == 3, \
        "the reference serves rank-3 inlier sets only"
    H, cd, cm, _ = refit_moments(p1, p2, rows)
    s = np.linalg.svd(H, compute_uv=False)
    assert s[2] > 1e-6 * s[0], "H must have three usable singular pairs (no reflection fix in the reference)"
    return transform_from_moments(H, cd, cm)
