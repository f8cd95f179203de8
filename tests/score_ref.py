"""The reference of the transform scoring (pcreg_model_score_f32's contract, include/pcreg.h), from parts that are references
already: numpy float64 for the transformed queries, the brute-force fp32 nearest row of tests/knn_k_ref.py, math.fsum for the sum.

transformed(q, T)      -> [B, Q, 3] float32: ((x*T[0,j] + y*T[1,j]) + z*T[2,j]) + T[3,j] in float64, rounded once; an all-zero
                          transform's queries are NaN (it scores nothing)
score(q, model, T, r2) -> idx [B, Q] int32 (0-based, -1 for none), dist [B, Q] float32 (+inf for none), n_close [B] int32,
                          sum_d2 [B] float64 (math.fsum: the correctly rounded sum)
"""
from __future__ import annotations

import math

import numpy as np

import knn_k_ref


def transformed(q, T):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    x, y, z = (q[:, c].astype(np.float64) for c in range(3))
    out = np.empty((len(T), len(q), 3), np.float32)
    with np.errstate(all="ignore"):
        for b, t in enumerate(T):
            if not t.any():                                    # the empty transform (-0.0 counts as zero, NaN does not)
                out[b] = np.nan
                continue
            for j in range(3):
                out[b, :, j] = (((x * t[0, j] + y * t[1, j]) + z * t[2, j]) + t[3, j]).astype(np.float32)
    return out


def nearest(tq, model, threads=None):
    """tq [N, 3] float32 -> idx [N], dist [N]: knn_k_ref with k = 1, whatever the radius.  A query with a NaN coordinate is not
    searched: all its distances are NaN, and it comes back as (-1, NaN)"""
    tq = np.asarray(tq, np.float32).reshape(-1, 3)
    idx, dist = np.full(len(tq), -1, np.int32), np.full(len(tq), np.nan, np.float32)
    ok = ~np.isnan(tq).any(axis=1)
    if ok.any():
        i, d = knn_k_ref.knn(tq[ok], model, 1, threads=threads)
        idx[ok], dist[ok] = i[:, 0], d[:, 0]
    return idx, dist


def within(idx, dist, r2):
    """the `<= r2` filter on nearest()'s result (NaN never passes): copies with -1 / +inf for none"""
    idx, dist = idx.copy(), dist.copy()
    with np.errstate(invalid="ignore"):
        hit = (idx >= 0) & (dist <= np.float32(r2))
    idx[~hit] = -1
    dist[~hit] = np.inf
    return idx, dist


def sums(idx, dist):
    """idx, dist [B, Q] -> n_close [B] int32, sum_d2 [B] float64"""
    hit = idx >= 0
    n_close = hit.sum(axis=1).astype(np.int32)
    sum_d2 = np.array([math.fsum(dist[b][hit[b]].astype(np.float64).tolist()) for b in range(len(idx))], np.float64).reshape(len(idx))
    return n_close, sum_d2


def score(q, model, T, r2, threads=None):
    tq = transformed(q, T)
    B, Q = tq.shape[:2]
    idx, dist = within(*nearest(tq.reshape(-1, 3), model, threads=threads), r2)
    idx, dist = idx.reshape(B, Q), dist.reshape(B, Q)
    return (idx, dist) + sums(idx, dist)
