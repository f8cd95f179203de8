"""TEST REFERENCE of the normal-distributions transform (pcreg_ndt's contract, include/pcreg.h).

The grid is downsample_ref's: cells and counts are exact integers.  The means are a sequential float64 sum (the contract's own
chain, so the library's must give these bits).  The covariances are taken in numpy.longdouble about the longdouble mean;
numpy.linalg.eigh (float64: LAPACK has no longdouble) gives a first basis, a cyclic Jacobi in longdouble finishes the
decomposition in that basis, and the floor and C = V diag(1 / l) V^T follow in longdouble.  The step takes a TABLE as its input, as
plane_ref takes the normals: the moved points are score_ref.transformed, the pairs are found from exact integer cells, the 28 sums
are taken in longdouble (numpy's pairwise summation, not the library's tree), the fit is plane_ref.fit and the product
refit_ref.compose.

grid(pts, step)                      -> lo [3] float32, live [n] bool, cell [n, 3] int64 (garbage where not live)
table(pts, step, min_points=6)       -> dict: cells [G, 3], counts [G], means [G, 3] float64, C [G, 6] float64 by gauss64, C_ref [G, 6]
                                        longdouble, lo, origin (float32), step, n_voxels, voxel_counts (every voxel's), members
gauss64(rows)                        -> (mean [3], C [6] or None): ndt_gauss.hpp in float64, operation by operation
d2_of(step, outlier_ratio)           -> the contract's d2
pairs(tab, p, neighbors)             -> (query [P], gaussian [P]) in ascending (query, candidate) order
sums(tab, p, neighbors, d2)          -> (sums [28] longdouble, n_pairs)
step(q, tab, T, neighbors=1, outlier_ratio=0.55) -> dict: T_step, T_out, empty, n_pairs, sum_e, pivot, tq
"""
from __future__ import annotations

import math

import numpy as np

import plane_ref
import refit_ref
import score_ref
from cylinders_ref import _div, jacobi64

LD = np.longdouble
FLOOR = 0.01
MAX_CELLS = 1 << 21
NEIGHBORS = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # the contract's candidate order


def grid(pts, step):
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    live = np.isfinite(p).all(axis=1)
    if not live.any():
        return np.zeros(3, np.float32), live, np.zeros((len(p), 3), np.int64)
    lo = p[live].min(axis=0)
    with np.errstate(all="ignore"):
        cell = np.floor((p.astype(np.float64) - lo.astype(np.float64)) / float(step))
    cell[~live] = 0
    return lo, live, cell.astype(np.int64)


def key_of(cell):
    cell = np.asarray(cell, np.int64)
    return (cell[..., 0] << 42) | (cell[..., 1] << 21) | cell[..., 2]


def gauss64(rows):
    """ndt_gauss.hpp in float64, one operation per operation (Python floats are IEEE doubles, never contracted)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    n = len(rows)
    s = [0.0, 0.0, 0.0]
    for r in rows:
        for c in range(3):
            s[c] = s[c] + float(r[c])
    mean = [_div(s[c], float(n)) for c in range(3)]
    m = [0.0] * 6
    for r in rows:
        d = [float(r[c]) - mean[c] for c in range(3)]
        m[0] = m[0] + d[0] * d[0]; m[1] = m[1] + d[0] * d[1]; m[2] = m[2] + d[0] * d[2]
        m[3] = m[3] + d[1] * d[1]; m[4] = m[4] + d[1] * d[2]; m[5] = m[5] + d[2] * d[2]
    a, V = jacobi64([_div(v, float(n - 1)) for v in m])
    l = [a[0], a[3], a[5]]
    if not all(math.isfinite(v) for v in l):
        return np.array(mean), None
    lmax = l[0]
    if l[1] > lmax:
        lmax = l[1]
    if l[2] > lmax:
        lmax = l[2]
    if not lmax > 0.0:
        return np.array(mean), None
    f = FLOOR * lmax
    l = [f if v < f else v for v in l]
    C = [(_div(V[3 * a_] * V[3 * b_], l[0]) + _div(V[3 * a_ + 1] * V[3 * b_ + 1], l[1])) + _div(V[3 * a_ + 2] * V[3 * b_ + 2], l[2])
         for a_, b_ in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.array(mean), np.array(C)


def _jacobi_ld(A):
    """eigen-decomposition of a symmetric 3 x 3 longdouble matrix: eigh's float64 basis, then cyclic Jacobi in longdouble"""
    A = np.asarray(A, LD)
    _w, V0 = np.linalg.eigh(A.astype(np.float64))
    V = V0.astype(LD)
    Bm = V.T @ A @ V
    for _ in range(30):
        off = abs(Bm[0, 1]) + abs(Bm[0, 2]) + abs(Bm[1, 2])
        if off <= LD(1e-30) * (abs(Bm[0, 0]) + abs(Bm[1, 1]) + abs(Bm[2, 2])) or off == 0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if Bm[p, q] == 0:
                continue
            theta = (Bm[q, q] - Bm[p, p]) / (2 * Bm[p, q])
            t = (LD(1) if theta >= 0 else LD(-1)) / (abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            G = np.eye(3, dtype=LD)
            G[p, p] = G[q, q] = c
            G[p, q], G[q, p] = s, -s
            Bm = G.T @ Bm @ G
            V = V @ G
    return np.diag(Bm).copy(), V


def gauss_ld(rows):
    """the longdouble Gaussian of the member rows -> C [6] longdouble (xx xy xz yy yz zz), or None for a void voxel"""
    x = np.asarray(rows, np.float32).reshape(-1, 3).astype(LD)
    d = x - x.mean(axis=0)
    cov = (d.T @ d) / LD(len(x) - 1)
    l, V = _jacobi_ld(cov)
    lmax = l.max()
    if not (np.isfinite(l).all() and lmax > 0):
        return None
    l = np.maximum(l, LD(FLOOR) * lmax)
    Cm = (V / l) @ V.T
    return np.array([Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]], LD)


def table(pts, step, min_points=6):
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    lo, live, cell = grid(p, step)
    tab = dict(step=float(step), min_points=int(min_points), lo=lo, origin=np.zeros(3, np.float32), n_voxels=0, cells=np.zeros((0, 3), np.int32),
               counts=np.zeros(0, np.int32), means=np.zeros((0, 3)), C=np.zeros((0, 6)), C_ref=np.zeros((0, 6), LD), members=[],
               voxel_counts=np.zeros(0, np.int64), voxel_cells=np.zeros((0, 3), np.int64))
    if not live.any():
        return tab
    hi = p[live].max(axis=0)
    tab["origin"] = np.float32(0.5) * lo + np.float32(0.5) * hi
    rows = np.flatnonzero(live)
    if cell[rows].max() >= MAX_CELLS:
        raise ValueError("the cloud spans 2^21 or more cells along an axis")
    keys = key_of(cell[rows])
    order = np.argsort(keys, kind="stable")                 # ascending key, ascending original row inside a voxel
    uk, start, cnt = np.unique(keys[order], return_index=True, return_counts=True)
    tab["n_voxels"], tab["voxel_counts"] = len(uk), cnt
    tab["voxel_cells"] = cell[rows[order[start]]]
    cells, counts, means, C64, Cref, members = [], [], [], [], [], []
    for s, c in zip(start, cnt):
        if c < min_points:
            continue
        mem = rows[order[s:s + c]]
        mean, C = gauss64(p[mem])
        if C is None:
            continue
        seq = np.cumsum(p[mem].astype(np.float64), axis=0)[-1] / float(c)            # the sequential float64 sum
        assert seq.tolist() == mean.tolist()
        cells.append(cell[mem[0]]); counts.append(c); means.append(mean); C64.append(C); Cref.append(gauss_ld(p[mem])); members.append(mem)
    if cells:
        tab.update(cells=np.array(cells, np.int32), counts=np.array(counts, np.int32), means=np.array(means), C=np.array(C64),
                   C_ref=np.array(Cref, LD), members=members)
    return tab


def d2_of(step, outlier_ratio):
    if outlier_ratio == 0:
        return 1.0
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / ((step * step) * step)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    return -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)


def pairs(tab, p, neighbors):
    """p [Q, 3] float32 moved points -> (query [P], gaussian [P]) in ascending (query, candidate) order"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    G = len(tab["cells"])
    if G == 0 or len(p) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    keys = key_of(tab["cells"].astype(np.int64))
    assert (np.diff(keys) > 0).all()
    with np.errstate(all="ignore"):
        cell = np.floor((p.astype(np.float64) - tab["lo"].astype(np.float64)) / tab["step"])
    qi, ci, gi = [], [], []
    for k, off in enumerate(NEIGHBORS[:neighbors]):
        c = cell + np.array(off, np.float64)
        ok = ((c >= 0) & (c < MAX_CELLS)).all(axis=1)               # (NaN and inf fail)
        idx = np.flatnonzero(ok)
        kk = key_of(c[idx].astype(np.int64))
        at = np.searchsorted(keys, kk)
        hit = (at < G) & (keys[np.minimum(at, G - 1)] == kk)
        qi.append(idx[hit]); ci.append(np.full(hit.sum(), k)); gi.append(at[hit])
    qi, ci, gi = np.concatenate(qi), np.concatenate(ci), np.concatenate(gi)
    order = np.lexsort((ci, qi))
    return qi[order], gi[order]


def full(C6):
    C6 = np.asarray(C6)
    return np.stack([np.stack([C6[..., 0], C6[..., 1], C6[..., 2]], -1), np.stack([C6[..., 1], C6[..., 3], C6[..., 4]], -1),
                     np.stack([C6[..., 2], C6[..., 4], C6[..., 5]], -1)], -2)


def sums(tab, p, neighbors, d2):
    qi, gi = pairs(tab, p, neighbors)
    out = np.zeros(28, LD)
    if len(qi) == 0:
        return out, 0
    pp = np.asarray(p, np.float32).reshape(-1, 3)[qi].astype(LD)
    x = pp - tab["means"][gi].astype(LD)
    u = pp - tab["origin"].astype(np.float64).astype(LD)
    Cm = full(tab["C"][gi].astype(LD))
    y = np.einsum("nab,nb->na", Cm, x)
    qq = (x * y).sum(axis=1)
    e = np.exp(-(LD(d2) / 2) * qq)
    J = np.zeros((len(qi), 3, 6), LD)
    for i in range(3):
        ei = np.zeros(3, LD); ei[i] = 1
        J[:, :, i] = np.cross(ei[None, :], u)
        J[:, i, 3 + i] = 1
    A = np.einsum("n,nai,nab,nbj->ij", e, J, Cm, J)
    g = np.einsum("n,nai,na->i", e, J, y)
    for i in range(6):
        for j in range(i, 6):
            out[plane_ref.tri(i, j)] = A[i, j]
        out[21 + i] = g[i]
    out[27] = e.sum()
    return out, len(qi)


def info_pair64(C, x, u, e, acc0, weighted):
    """info_pair.hpp in float64, one operation per operation, in its order: the 27 sums from acc0 after one pair (C [6] xx xy xz yy
    yz zz, x [3], u [3]), y = C x and qq = x . y.  Products and differences are plain float64; weighted: each add is the correctly
    rounded fma(e, term, sum) for a finite e > 0, formed exactly in rationals and rounded once; otherwise sum + term and e is not
    read."""
    from fractions import Fraction
    C, x, u = (np.asarray(v, np.float64) for v in (C, x, u))
    acc = [np.float64(v) for v in acc0]
    e = float(e)

    def add(k, term):
        if not weighted:
            acc[k] = acc[k] + term
            return
        exact = Fraction(e) * Fraction(float(term)) + Fraction(float(acc[k]))
        # (an exact zero is -0.0 only as the sum of two negative zeros; e > 0, so the product has the term's sign)
        acc[k] = np.float64(float(exact)) if exact else np.float64(-0.0 if term == 0 and np.signbit(term) and np.signbit(acc[k]) else 0.0)

    def cross(a, b0, b1, b2):
        return [a[1] * b2 - a[2] * b1, a[2] * b0 - a[0] * b2, a[0] * b1 - a[1] * b0]
    y = [(C[0] * x[0] + C[1] * x[1]) + C[2] * x[2], (C[1] * x[0] + C[3] * x[1]) + C[4] * x[2], (C[2] * x[0] + C[4] * x[1]) + C[5] * x[2]]
    qq = (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    W = [cross(u, C[0], C[1], C[2]), cross(u, C[1], C[3], C[4]), cross(u, C[2], C[4], C[5])]
    for j in range(3):
        M = cross(u, W[0][j], W[1][j], W[2][j])
        for i in range(j + 1):
            add(plane_ref.tri(i, j), M[i])
        for i in range(3):
            add(plane_ref.tri(i, 3 + j), W[j][i])
    for k, (a, b) in enumerate(((3, 3), (3, 4), (3, 5), (4, 4), (4, 5), (5, 5))):
        add(plane_ref.tri(a, b), C[k])
    gy = cross(u, y[0], y[1], y[2])
    for i in range(3):
        add(21 + i, gy[i])
        add(24 + i, y[i])
    return np.array(acc, np.float64), np.array(y, np.float64), np.float64(qq)


def step(q, tab, T, neighbors=1, outlier_ratio=0.55):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tq = score_ref.transformed(q, T)
    B = len(T)
    d2 = d2_of(tab["step"], outlier_ratio)
    o = tab["origin"].astype(np.float64)
    T_step, T_out, empty = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.ones(B, bool)
    n_pairs, sum_e, pivot = np.zeros(B, np.int32), np.zeros(B), np.full(B, np.nan)
    for b in range(B):
        s, n_pairs[b] = sums(tab, tq[b], neighbors, d2)
        sum_e[b] = float(s[27])
        S, pivot[b] = plane_ref.fit(s, n_pairs[b], o) if T[b].any() else (None, np.nan)
        if S is not None:
            T_step[b], T_out[b], empty[b] = S, refit_ref.compose(T[b], S), False
    return dict(T_step=T_step, T_out=T_out, empty=empty, n_pairs=n_pairs, sum_e=sum_e, pivot=pivot, tq=tq, d2=d2)


def steps(q, tab, T, n, neighbors=1, outlier_ratio=0.55):
    """n steps, each one's T_out the next one's T -> the list of the steps' dicts"""
    out = []
    for _ in range(n):
        out.append(step(q, tab, T, neighbors, outlier_ratio))
        T = out[-1]["T_out"]
    return out
