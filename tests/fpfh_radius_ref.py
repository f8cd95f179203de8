"""TEST REFERENCE for the FPFH descriptor from radius neighbourhoods (pcreg_model_fpfh_radius_f32's contract in include/pcreg.h).

Neighbour lists come from range_ref.rangesearch(model, model, r2): the fp32 chain, inclusive radius, (distance, row) order.  The
NEIGHBOURS of a row are its entries with a finite squared distance > 0, and with max_neighbors = n > 0 only the first n of them
count.  The pair mathematics, TOL and the sensitivity / exclusion rule are fpfh_ref.py's, restated here over padded [M, n_max]
lists (fpfh_ref.fpfh is tied to the k-nearest lists and to counts <= 31); the helpers are imported from it.

fpfh(model, normals, r2, max_neighbors=0) -> dict with, per row,
  idx, d2, nb  [M, n_max]  the counted window: rows (clipped), fp32 squared distances, and which places are filled
  n         [M]     int64    the neighbours counted (0 for a non-finite row)
  counts    [M, 33] int64    the SPFH counts, f1's eleven bins, then f2's, then f3's
  m         [M]     int64    the contributing pairs
  out       [M, 33] longdouble the FPFH, NaN for a non-finite row
  sensitive [M]     bool     fpfh_ref's rule: some contributing pair within TOL of a bin edge or of the swap tie
  excluded  [M]     bool     the row or one of its counted neighbours is sensitive: the row is not compared
plain_double(model, normals, r2, max_neighbors=0) restates the contract in Python floats, pair by pair, with nothing shared but
the neighbour lists.  case(family, radius, max_neighbors) are the cached inputs and results of the GPU test and of the
exclusion-share check: fpfh_ref's families and normals (M = 2048, normals_ref at K_NORMALS = 9, oriented, rounded to fp32).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import fpfh_ref
import range_ref
from fpfh_ref import EPS, EXCLUDED_CAP, TOL, _cross, _dot, family_inputs

CASES = (("sheet", 4.0), ("sheet", 8.0), ("volume", 4.0), ("volume", 16.0))       # counts on both sides of 31 and 64, past a byte
MAX_NEIGHBORS = (0, 50)
_CHUNK = 128                                   # rows evaluated at a time (bounds the long-double temporaries)


def out_tol(n_max: int) -> float:
    """|x - x_ref| on the output for a case whose longest counted neighbourhood is n_max: every term of acc is positive; n
    sequential double adds of terms carrying two roundings each, ten adds for S_f, a division and a product bound the relative
    error by about (n + 8) eps; the factor 2 covers second-order terms and the reference's own rounding; the output is <= 100."""
    return 2 * (n_max + 8) * EPS * 100


def r2_of(radius) -> np.float32:
    """the squared radius as the wrappers form it: squared in double, rounded once to float32"""
    return np.float32(float(radius) * float(radius))


def lists(model, r2, max_neighbors: int = 0):
    """-> idx [M, n_max] int64, d2 [M, n_max] float32, nb [M, n_max] bool, n [M] int64: the counted window of every row, padded"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    M = len(m)
    seg, ridx, rd2 = range_ref.rangesearch(m, m, r2)
    finite_row = np.isfinite(m).all(axis=1)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(rd2) & (rd2 > 0)
    keep &= finite_row[ridx] if len(ridx) else keep
    keep &= np.repeat(finite_row, np.diff(seg))
    owner = np.repeat(np.arange(M), np.diff(seg))[keep]
    kidx, kd2 = ridx[keep].astype(np.int64), rd2[keep]
    n = np.bincount(owner, minlength=M).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    pos = np.arange(len(owner)) - first[owner] if len(owner) else np.zeros(0, np.int64)
    if max_neighbors > 0:
        sel = pos < max_neighbors
        owner, kidx, kd2, pos = owner[sel], kidx[sel], kd2[sel], pos[sel]
        n = np.minimum(n, max_neighbors)
    n_max = int(n.max(initial=0))
    idx = np.zeros((M, n_max), np.int64)
    d2 = np.full((M, n_max), np.inf, np.float32)
    nb = np.zeros((M, n_max), bool)
    idx[owner, pos], d2[owner, pos], nb[owner, pos] = kidx, kd2, True
    return idx, d2, nb, n


def _pairs(m, n32, idx, nb):
    """fpfh_ref's pair mathematics over padded lists -> b [M, n, 3] int64 bins, on [M, n] contributes, sens [M, n] sensitive pair"""
    T = np.longdouble
    M, n_max = idx.shape
    b = np.zeros((M, n_max, 3), np.int64)
    on = np.zeros((M, n_max), bool)
    sens = np.zeros((M, n_max), bool)
    p, n = m.astype(T), n32.astype(T)
    fin_n = np.isfinite(n32).all(axis=1)
    bits = np.ascontiguousarray(n32).view(np.uint32)
    pi = T(np.pi)
    for lo in range(0, M, _CHUNK):
        sl = slice(lo, min(lo + _CHUNK, M))
        ix, nbx = idx[sl], nb[sl]
        with np.errstate(all="ignore"):
            d = p[ix] - p[sl, None, :]
            ni = np.broadcast_to(n[sl, None, :], d.shape)
            nj = n[ix]
            ln = np.sqrt(_dot(d, d))
            ai, aj = _dot(ni, d) / ln, _dot(nj, d) / ln
            swap = np.abs(ai) < np.abs(aj)
            ns = np.where(swap[..., None], nj, ni)
            nt = np.where(swap[..., None], ni, nj)
            d = np.where(swap[..., None], -d, d)
            f3 = np.where(swap, -aj, ai)
            v = _cross(d, ns)
            vl = np.sqrt(_dot(v, v))
            v = v / vl[..., None]
            w = _cross(ns, v)
            f2 = _dot(v, nt)
            f1 = np.arctan2(_dot(w, nt), _dot(ns, nt))
            x = np.stack([T(11) * ((f1 + pi) / (T(2) * pi)), T(11) * ((f2 + T(1)) * T(0.5)), T(11) * ((f3 + T(1)) * T(0.5))], axis=-1)
            o = nbx & (ln > 0) & (vl > 0) & ~np.isnan(x).any(axis=-1) & fin_n[sl, None] & fin_n[ix]
            b[sl] = np.clip(np.floor(np.where(np.isnan(x), T(0), x)), 0, 10).astype(np.int64)
            edge = np.abs(x - np.round(x))
            r = np.round(np.where(np.isnan(x), T(0.5), x))
            near = (edge < TOL) & (r >= 1) & (r <= 10)
            near[..., 0] |= (edge[..., 0] < TOL) & ((r[..., 0] == 0) | (r[..., 0] == 11))
            bi, bj = bits[sl, None, :], bits[ix]
            same = (bi == bj).all(axis=-1) | (bi == (bj ^ np.uint32(0x80000000))).all(axis=-1)
            tie = (np.abs(np.abs(ai) - np.abs(aj)) < TOL) & ~same
        on[sl] = o
        sens[sl] = o & (near.any(axis=-1) | tie)
    return b, on, sens


def fpfh(model, normals, r2, max_neighbors: int = 0) -> dict:
    T = np.longdouble
    m = np.asarray(model, np.float32).reshape(-1, 3)
    n32 = np.asarray(normals, np.float32).reshape(-1, 3)
    M = len(m)
    idx, d2, nb, n = lists(m, r2, max_neighbors)
    res = dict(idx=idx, d2=d2, nb=nb, n=n, counts=np.zeros((M, 33), np.int64), m=np.zeros(M, np.int64), out=np.zeros((M, 33), T),
               sensitive=np.zeros(M, bool), excluded=np.zeros(M, bool))
    if M == 0:
        return res
    finite_row = np.isfinite(m).all(axis=1)
    n_max = idx.shape[1]
    b, on, sens = _pairs(m, n32, idx, nb)
    res["sensitive"] = sens.any(axis=1)
    res["excluded"] = res["sensitive"] | (nb & res["sensitive"][idx]).any(axis=1)
    counts = res["counts"]
    rows = np.broadcast_to(np.arange(M)[:, None], on.shape)
    for f in range(3):
        np.add.at(counts, (rows[on], 11 * f + b[..., f][on]), 1)
    mm = counts[:, :11].sum(axis=1)
    res["m"] = mm
    assert (counts[:, 11:22].sum(axis=1) == mm).all() and (counts[:, 22:].sum(axis=1) == mm).all() and (mm <= n).all()
    acc = np.zeros((M, 33), T)
    with np.errstate(all="ignore"):
        for s in range(n_max):                                               # list order
            live = np.flatnonzero(nb[:, s])
            j = idx[live, s]
            use = mm[j] > 0
            live, j = live[use], j[use]
            acc[live] = acc[live] + (counts[j].astype(T) / mm[j].astype(T)[:, None]) / d2[live, s].astype(T)[:, None]
        out = np.zeros((M, 33), T)
        for f in range(3):
            a = acc[:, 11 * f:11 * f + 11]
            S = a[:, 0].copy()
            for bb in range(1, 11):
                S = S + a[:, bb]
            out[:, 11 * f:11 * f + 11] = np.where((S > 0)[:, None], (a / np.where(S > 0, S, T(1))[:, None]) * T(100), T(0))
    out[~finite_row] = np.nan
    res["out"] = out
    return res


def plain_double(model, normals, r2, max_neighbors: int = 0):
    """the contract in Python floats, one pair at a time -> (counts [M, 33] int64, out [M, 33] float64)"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    n32 = np.asarray(normals, np.float32).reshape(-1, 3)
    M = len(m)
    counts = np.zeros((M, 33), np.int64)
    out = np.zeros((M, 33), np.float64)
    if M == 0:
        return counts, out
    idx, d2, nb, n = lists(m, r2, max_neighbors)
    P, N = m.astype(np.float64).tolist(), n32.astype(np.float64).tolist()
    fin = [all(math.isfinite(c) for c in row) for row in N]
    sqrt, atan2, floor, pi = math.sqrt, math.atan2, math.floor, math.pi

    def bin_of(x):
        return int(min(max(floor(11.0 * x), 0.0), 10.0))

    for i in range(M):
        pi_, ni = P[i], N[i]
        for s in range(int(n[i])):
            j = int(idx[i, s])
            pj, nj = P[j], N[j]
            if not (fin[i] and fin[j]):
                continue
            dx, dy, dz = pj[0] - pi_[0], pj[1] - pi_[1], pj[2] - pi_[2]
            ln = sqrt((dx * dx + dy * dy) + dz * dz)
            if not ln > 0.0:
                continue
            ai = ((ni[0] * dx + ni[1] * dy) + ni[2] * dz) / ln
            aj = ((nj[0] * dx + nj[1] * dy) + nj[2] * dz) / ln
            if abs(ai) < abs(aj):
                ns, nt, dx, dy, dz, f3 = nj, ni, -dx, -dy, -dz, -aj
            else:
                ns, nt, f3 = ni, nj, ai
            vx, vy, vz = dy * ns[2] - dz * ns[1], dz * ns[0] - dx * ns[2], dx * ns[1] - dy * ns[0]
            vl = sqrt((vx * vx + vy * vy) + vz * vz)
            if not vl > 0.0:
                continue
            vx, vy, vz = vx / vl, vy / vl, vz / vl
            wx, wy, wz = ns[1] * vz - ns[2] * vy, ns[2] * vx - ns[0] * vz, ns[0] * vy - ns[1] * vx
            f2 = (vx * nt[0] + vy * nt[1]) + vz * nt[2]
            f1 = atan2((wx * nt[0] + wy * nt[1]) + wz * nt[2], (ns[0] * nt[0] + ns[1] * nt[1]) + ns[2] * nt[2])
            if f1 != f1 or f2 != f2 or f3 != f3:
                continue
            counts[i, bin_of((f1 + pi) / (2.0 * pi))] += 1
            counts[i, 11 + bin_of((f2 + 1.0) * 0.5)] += 1
            counts[i, 22 + bin_of((f3 + 1.0) * 0.5)] += 1
    mm = counts[:, :11].sum(axis=1)
    finite_row = np.isfinite(m).all(axis=1)
    for i in range(M):
        if not finite_row[i]:
            out[i] = np.nan
            continue
        acc = [0.0] * 33
        for s in range(int(n[i])):
            j = int(idx[i, s])
            if mm[j] > 0:
                mj, w = float(mm[j]), float(d2[i, s])
                cj = counts[j].tolist()
                for b in range(33):
                    acc[b] = acc[b] + (float(cj[b]) / mj) / w
        for f in range(3):
            S = acc[11 * f]
            for b in range(1, 11):
                S = S + acc[11 * f + b]
            if S > 0.0:
                for b in range(11):
                    out[i, 11 * f + b] = (acc[11 * f + b] / S) * 100.0
    return counts, out


@functools.lru_cache(maxsize=None)
def case(name: str, radius: float, max_neighbors: int = 0):
    model, nrm = family_inputs(name)
    r = fpfh(model, nrm, r2_of(radius), max_neighbors)
    for a in r.values():
        a.setflags(write=False)
    return r


def excluded_share(r: dict) -> float:
    return fpfh_ref.excluded_share(r)
