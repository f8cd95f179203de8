"""TEST REFERENCE of the plane-to-plane (generalized ICP) refit (pcreg_model_refit_gicp_f32's contract, include/pcreg.h).

The pairs come from tests/score_ref.py, as tests/plane_ref.py takes them.  Both sets of normals are inputs.  Per pair S, its
Cholesky factor and W = S^-1 are taken in numpy.longdouble; the 28 sums are NDT's per-pair terms with C := W and no weight, summed
in longdouble (numpy's pairwise summation, not the library's tree); the fit is plane_ref.fit and the product refit_ref.compose.

weights(n, v, a)                   -> (W [P, 3, 3] longdouble, ok [P] bool): S = 2 I - a (n n^T + v v^T) inverted through its Cholesky
                                       factor; ok where the three pivots are finite and above 0
pairs(model, normals, qnormals, idx_b, tq_b) -> (query [P], m, p, n, nq [P, 3] float64): the hits with six finite normal components
sums(model, normals, qnormals, idx_b, tq_b, T_b, o, epsilon) -> (sums [28] longdouble, n_pairs)
step(q, model, normals, qnormals, T, r2, epsilon=1e-3) -> plane_ref.step's dict with n_pairs in n_plane's place
steps(q, model, normals, qnormals, T, r2, n, epsilon=1e-3) -> the list of n steps' dicts, each one's T_out the next one's T
pair64(n, nq, T16, a, want_s=False) -> W [6] (xx xy xz yy yz zz) as a list of floats, or None: the float64 restatement of
                                       pcreg_amd/csrc/gicp_pair.hpp in the header's order, operation by operation
sum_res2_64(model, normals, qnormals, idx_b, tq_b, T_b, epsilon) -> (the contract's 28th sum in float64 by pair64, added in query
                                       order; n_pairs by pair64's own judgement)
surface_normals()                  -> plane_ref.scene()'s surface normals: normals_ref at k = 8 on the surface's own rows, fp32
"""
from __future__ import annotations

import math

import numpy as np

import plane_ref
import refit_ref
import score_ref

LD = np.longdouble
EPSILON = 1e-3


def t16(T):
    """a [4, 4] transform as quickTF uses it ([p, 1] @ T) -> the library's 16 doubles, new_j = x T16[4j] + y T16[4j+1] + z T16[4j+2] + T16[4j+3]"""
    return np.asarray(T, np.float64).reshape(4, 4).T.reshape(16).copy()


def weights(n, v, a):
    n, v = np.asarray(n, LD).reshape(-1, 3), np.asarray(v, LD).reshape(-1, 3)
    P = len(n)
    with np.errstate(all="ignore"):
        S = 2 * np.eye(3, dtype=LD)[None] - LD(a) * (n[:, :, None] * n[:, None, :] + v[:, :, None] * v[:, None, :])
        L = np.zeros((P, 3, 3), LD)
        p0 = S[:, 0, 0]
        L[:, 0, 0] = np.sqrt(p0)
        L[:, 1, 0] = S[:, 0, 1] / L[:, 0, 0]
        L[:, 2, 0] = S[:, 0, 2] / L[:, 0, 0]
        p1 = S[:, 1, 1] - L[:, 1, 0] ** 2
        L[:, 1, 1] = np.sqrt(p1)
        L[:, 2, 1] = (S[:, 1, 2] - L[:, 2, 0] * L[:, 1, 0]) / L[:, 1, 1]
        p2 = S[:, 2, 2] - L[:, 2, 0] ** 2 - L[:, 2, 1] ** 2
        L[:, 2, 2] = np.sqrt(p2)
        ok = np.ones(P, bool)
        for p in (p0, p1, p2):
            ok &= np.isfinite(p) & (p > 0)
        Mi = np.zeros((P, 3, 3), LD)
        Mi[:, 0, 0], Mi[:, 1, 1], Mi[:, 2, 2] = 1 / L[:, 0, 0], 1 / L[:, 1, 1], 1 / L[:, 2, 2]
        Mi[:, 1, 0] = -L[:, 1, 0] * Mi[:, 0, 0] / L[:, 1, 1]
        Mi[:, 2, 1] = -L[:, 2, 1] * Mi[:, 1, 1] / L[:, 2, 2]
        Mi[:, 2, 0] = -(L[:, 2, 0] * Mi[:, 0, 0] + L[:, 2, 1] * Mi[:, 1, 0]) / L[:, 2, 2]
        W = np.einsum("pki,pkj->pij", Mi, Mi)
    return W, ok


def pairs(model, normals, qnormals, idx_b, tq_b):
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    nq = np.asarray(qnormals, np.float32).reshape(-1, 3)
    hit = np.flatnonzero(np.asarray(idx_b) >= 0)
    rows = np.asarray(idx_b)[hit]
    ok = (np.isfinite(nrm[rows]).all(axis=1) & np.isfinite(nq[hit]).all(axis=1)) if len(hit) else np.zeros(0, bool)
    hit, rows = hit[ok], rows[ok]
    return (hit, np.asarray(model, np.float32).reshape(-1, 3)[rows].astype(np.float64), np.asarray(tq_b, np.float32)[hit].astype(np.float64),
            nrm[rows].astype(np.float64), nq[hit].astype(np.float64))


def sums_of_pairs(m, p, n, nq, T_b, o, epsilon):
    """the 28 sums of given candidate pairs (all six normal components finite) under the transform T_b -> (sums, n_pairs, kept [P] bool)"""
    out = np.zeros(28, LD)
    if len(m) == 0:
        return out, 0, np.zeros(0, bool)
    m, p, n, nq = (np.asarray(a, np.float64).reshape(-1, 3).astype(LD) for a in (m, p, n, nq))
    R = np.asarray(T_b, np.float64).reshape(4, 4)[:3, :3].astype(LD)
    with np.errstate(all="ignore"):
        v = nq @ R
    W, ok = weights(n, v, 1.0 - float(epsilon))
    if not ok.any():
        return out, 0, ok
    m, p, W = m[ok], p[ok], W[ok]
    e = p - m
    u = p - np.asarray(o, np.float64).astype(LD)
    y = np.einsum("nab,nb->na", W, e)
    J = np.zeros((len(m), 3, 6), LD)
    for i in range(3):
        ei = np.zeros(3, LD); ei[i] = 1
        J[:, :, i] = np.cross(ei[None, :], u)
        J[:, i, 3 + i] = 1
    A = np.einsum("nai,nab,nbj->ij", J, W, J)
    g = np.einsum("nai,na->i", J, y)
    for i in range(6):
        for j in range(i, 6):
            out[plane_ref.tri(i, j)] = A[i, j]
        out[21 + i] = g[i]
    out[27] = (e * y).sum()
    return out, int(ok.sum()), ok


def sums(model, normals, qnormals, idx_b, tq_b, T_b, o, epsilon):
    _hit, m, p, n, nq = pairs(model, normals, qnormals, idx_b, tq_b)
    s, cnt, _ok = sums_of_pairs(m, p, n, nq, T_b, o, epsilon)
    return s, cnt


def step(q, model, normals, qnormals, T, r2, epsilon=EPSILON, threads=None):
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
    o = plane_ref.origin(model)
    T_step, T_out, empty = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.ones(B, bool)
    n_pairs, sum_res2, pivot = np.zeros(B, np.int32), np.zeros(B), np.full(B, np.nan)
    for b in range(B):
        s, n_pairs[b] = sums(model, normals, qnormals, idx[b], tq[b], T[b], o, epsilon)
        sum_res2[b] = float(s[27])
        S, pivot[b] = plane_ref.fit(s, n_pairs[b], o) if T[b].any() else (None, np.nan)
        if S is not None:
            T_step[b], T_out[b], empty[b] = S, refit_ref.compose(T[b], S), False
    return dict(T_step=T_step, T_out=T_out, empty=empty, hit=idx >= 0, idx=idx, tq=tq, n_close=n_close, sum_d2=sum_d2, n_pairs=n_pairs,
                sum_res2=sum_res2, pivot=pivot)


def steps(q, model, normals, qnormals, T, r2, n, epsilon=EPSILON, threads=None):
    out = []
    for _ in range(n):
        out.append(step(q, model, normals, qnormals, T, r2, epsilon, threads=threads))
        T = out[-1]["T_out"]
    return out


def pair64(n, nq, T16, a, want_s=False):
    """gicp_pair.hpp in float64, one operation per operation (Python floats are IEEE doubles, never contracted); want_s: S (xx xy xz yy
    yz zz) instead of W, before any pivot is judged"""
    fin = lambda x: x - x == 0.0
    div = lambda x, y: float(np.float64(x) / np.float64(y))              # (IEEE division: inf and NaN instead of ZeroDivisionError)
    sqrt = lambda x: float(np.sqrt(np.float64(x)))
    n0, n1, n2 = (float(np.float32(c)) for c in n)
    q0, q1, q2 = (float(np.float32(c)) for c in nq)
    if not all(fin(c) for c in (n0, n1, n2, q0, q1, q2)):
        return None
    T = [float(t) for t in T16]
    a = float(a)
    with np.errstate(all="ignore"):
        v0 = (q0 * T[0] + q1 * T[1]) + q2 * T[2]
        v1 = (q0 * T[4] + q1 * T[5]) + q2 * T[6]
        v2 = (q0 * T[8] + q1 * T[9]) + q2 * T[10]
        sxx = 2.0 - a * (n0 * n0 + v0 * v0); sxy = 0.0 - a * (n0 * n1 + v0 * v1); sxz = 0.0 - a * (n0 * n2 + v0 * v2)
        syy = 2.0 - a * (n1 * n1 + v1 * v1); syz = 0.0 - a * (n1 * n2 + v1 * v2); szz = 2.0 - a * (n2 * n2 + v2 * v2)
        if want_s:
            return [sxx, sxy, sxz, syy, syz, szz]
        p0 = sxx
        if not p0 > 0.0 or not fin(p0):
            return None
        l00 = sqrt(p0); l10 = div(sxy, l00); l20 = div(sxz, l00)
        p1 = syy - l10 * l10
        if not p1 > 0.0 or not fin(p1):
            return None
        l11 = sqrt(p1); l21 = div(syz - l20 * l10, l11)
        p2 = (szz - l20 * l20) - l21 * l21
        if not p2 > 0.0 or not fin(p2):
            return None
        l22 = sqrt(p2)
        m00, m11, m22 = div(1.0, l00), div(1.0, l11), div(1.0, l22)
        m10 = div(-(l10 * m00), l11); m21 = div(-(l21 * m11), l22)
        m20 = div(-(l20 * m00 + l21 * m10), l22)
        return [(m00 * m00 + m10 * m10) + m20 * m20, m10 * m11 + m20 * m21, m20 * m22, m11 * m11 + m21 * m21, m21 * m22, m22 * m22]


def sum_res2_64(model, normals, qnormals, idx_b, tq_b, T_b, epsilon):
    hit, m, p, n, nq = pairs(model, normals, qnormals, idx_b, tq_b)
    T16, a = t16(T_b), 1.0 - float(epsilon)
    total, cnt = 0.0, 0
    for k in range(len(hit)):
        W = pair64(n[k], nq[k], T16, a)
        if W is None:
            continue
        x = [float(p[k][c]) - float(m[k][c]) for c in range(3)]
        y = [(W[0] * x[0] + W[1] * x[1]) + W[2] * x[2], (W[1] * x[0] + W[3] * x[1]) + W[4] * x[2], (W[2] * x[0] + W[4] * x[1]) + W[5] * x[2]]
        total = total + ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2])
        cnt += 1
    return total, cnt


_SURF = {}


def surface_normals():
    if "n" not in _SURF:
        import normals_ref
        sc = plane_ref.scene()
        _SURF["n"] = normals_ref.oriented(normals_ref.normals(sc["surf"], plane_ref.K_NORMALS), sc["surf"]).astype(np.float32)
    return _SURF["n"]


_REF = {}


def scene_ref(r2, epsilon=EPSILON, threads=None):
    sc = plane_ref.scene()
    key = (float(r2), float(epsilon))
    if key not in _REF:
        _REF[key] = step(sc["surf"], sc["model"], sc["normals"], surface_normals(), sc["T"], r2, epsilon, threads=threads)
    return _REF[key]
