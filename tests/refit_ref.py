"""The reference of the transform refit (pcreg_model_refit_f32's contract, include/pcreg.h), from references that exist:
tests/score_ref.py gives the pairs (float64 transformed queries rounded once, the brute-force fp32 nearest row, the `<= r2`
filter), oracle.pcreg_oracle.estimateTransform is applied in double to those pairs in ascending query order, and the
composition T * T_step is restated entry by entry with the contract's parenthesisation.

step(q, model, T, r2) -> dict(T_step [B, 4, 4], T_out [B, 4, 4], empty [B] bool, hit [B, Q] bool, idx [B, Q], tq [B, Q, 3],
                              n_close [B], sum_d2 [B]); matrices as quickTF uses them ([p, 1] @ T), zeros where empty
"""
from __future__ import annotations

import numpy as np

import score_ref
from oracle.pcreg_oracle import estimateTransform


def compose(T, S):
    """T * S, every entry ((T[r,0] S[0,c] + T[r,1] S[1,c]) + T[r,2] S[2,c]) + T[r,3] S[3,c] in float64"""
    T, S = np.asarray(T, np.float64), np.asarray(S, np.float64)
    out = np.empty((4, 4), np.float64)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                out[r, c] = ((T[r, 0] * S[0, c] + T[r, 1] * S[1, c]) + T[r, 2] * S[2, c]) + T[r, 3] * S[3, c]
    return out


def fit(model, idx_b, tq_b):
    """estimateTransform(model rows, moved points) over the hits of one transform in ascending query order, or None"""
    hit = idx_b >= 0
    if hit.sum() < 3:
        return None
    return estimateTransform(np.asarray(model, np.float32)[idx_b[hit]].astype(np.float64), tq_b[hit].astype(np.float64))


def step(q, model, T, r2, threads=None):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tq = score_ref.transformed(q, T)
    B, Q = tq.shape[:2]
    if len(model) and Q:
        idx, dist = score_ref.within(*score_ref.nearest(tq.reshape(-1, 3), model, threads=threads), r2)
    else:
        idx, dist = np.full(B * Q, -1, np.int32), np.full(B * Q, np.inf, np.float32)
    idx, dist = idx.reshape(B, Q), dist.reshape(B, Q)
    n_close, sum_d2 = score_ref.sums(idx, dist)
    T_step, T_out, empty = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.ones(B, bool)
    for b in range(B):
        S = fit(model, idx[b], tq[b]) if T[b].any() else None
        if S is not None:
            T_step[b], T_out[b], empty[b] = S, compose(T[b], S), False
    return dict(T_step=T_step, T_out=T_out, empty=empty, hit=idx >= 0, idx=idx, tq=tq, n_close=n_close, sum_d2=sum_d2)


def cross_covariance_singular_values(model, idx_b, tq_b):
    """the singular values of the centred cross-covariance estimateTransform.m:55-58 forms from the pairs, descending; exactly
    three pairs get the synthetic fourth point of :18-37 first, as the fit does"""
    hit = idx_b >= 0
    d = np.asarray(model, np.float32)[idx_b[hit]].astype(np.float64)
    m = tq_b[hit].astype(np.float64)
    if len(d) == 3:
        def fourth(p):
            n = np.cross(p[2] - p[1], p[2] - p[0])
            return np.vstack([p, p.sum(axis=0) / 3.0 + n / np.linalg.norm(n) * np.median(np.linalg.norm(p - np.roll(p, 1, axis=0), axis=1))])
        d, m = fourth(d), fourth(m)
    return np.linalg.svd((m - m.mean(axis=0)).T @ (d - d.mean(axis=0)), compute_uv=False)
