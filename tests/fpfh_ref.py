"""TEST REFERENCE for the FPFH descriptor of a prepared model (pcreg_model_fpfh_f32's contract in include/pcreg.h).

Neighbours come from knn_k_ref.knn(model, model, k), the fp32 brute force with (distance, row) ties; the NEIGHBOURS of a row are
its list entries with a row and a finite squared distance > 0.  The contract is evaluated in numpy.longdouble, vectorised over
the [M, k] pairs.

fpfh(model, normals, k) -> dict with, per row,
  counts    [M, 33] int64    the SPFH counts, f1's eleven bins, then f2's, then f3's
  m         [M]     int64    the contributing pairs
  out       [M, 33] longdouble the FPFH, NaN for a non-finite row
  sensitive [M]     bool     some pair of the row has a value 11 (...) within TOL of a bin edge 1 .. 10 (or of 0 or 11 for f1, where
                             the histogram wraps), or | |a_i| - |a_j| | < TOL with normals neither bitwise equal nor exact negatives
  excluded  [M]     bool     the row or one of its neighbours is sensitive: the row is not compared
plain_double(model, normals, k) restates the contract in Python floats, pair by pair, with nothing shared but the neighbour lists.
case(family, k) are the cached inputs and results of the GPU test and the exclusion-share check: normals_ref's families, normals
from normals_ref at K_NORMALS = 9 for EVERY k, oriented to VIEWPOINT and rounded to fp32 (normals from three-point
neighbourhoods lie in their neighbours' plane and make a tenth of the rows sensitive).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import knn_k_ref
import normals_ref

KS = (3, 4, 5, 8, 9, 16, 17, 32)          # every list size of the kernel (4, 8, 16, 32) and both sides of each boundary
K_NORMALS = 9
VIEWPOINT = (120.0, 70.0, 400.0)
M_FAMILY = 2048
TOL = 1e-9
EXCLUDED_CAP = 0.01
EPS = float(np.finfo(np.float64).eps)
OUT_TOL = 64 * EPS * 100                  # |x - x_ref| on the output


def neighbours(model, k):
    """-> idx [M, k] int64 (clipped into the model), d2 [M, k] float32, nb [M, k] bool: the entry is a NEIGHBOUR"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    M = len(m)
    idx, dist = knn_k_ref.knn(m, m, k)
    finite_row = np.isfinite(m).all(axis=1)
    cl = np.clip(idx, 0, max(M - 1, 0)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        nb = (idx >= 0) & np.isfinite(dist) & (dist > 0) & finite_row[:, None] & finite_row[cl]
    return cl, dist, nb


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def fpfh(model, normals, k: int) -> dict:
    T = np.longdouble
    m = np.asarray(model, np.float32).reshape(-1, 3)
    n32 = np.asarray(normals, np.float32).reshape(-1, 3)
    M = len(m)
    res = dict(counts=np.zeros((M, 33), np.int64), m=np.zeros(M, np.int64), out=np.zeros((M, 33), T), sensitive=np.zeros(M, bool),
               excluded=np.zeros(M, bool))
    if M == 0:
        return res
    idx, d2, nb = neighbours(m, k)
    finite_row = np.isfinite(m).all(axis=1)
    with np.errstate(all="ignore"):
        p, n = m.astype(T), n32.astype(T)
        d = p[idx] - p[:, None, :]
        ni = np.broadcast_to(n[:, None, :], d.shape)
        nj = n[idx]
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
        pi = T(np.pi)
        x = np.stack([T(11) * ((f1 + pi) / (T(2) * pi)), T(11) * ((f2 + T(1)) * T(0.5)), T(11) * ((f3 + T(1)) * T(0.5))], axis=-1)     # [M, k, 3]
        fin_n = np.isfinite(n32).all(axis=1)
        on = nb & (ln > 0) & (vl > 0) & ~np.isnan(x).any(axis=-1) & fin_n[:, None] & fin_n[idx]
        b = np.clip(np.floor(np.where(np.isnan(x), T(0), x)), 0, 10).astype(np.int64)
        # sensitivity
        edge = np.abs(x - np.round(x))
        r = np.round(np.where(np.isnan(x), T(0.5), x))
        near = (edge < TOL) & (r >= 1) & (r <= 10)
        near[..., 0] |= (edge[..., 0] < TOL) & ((r[..., 0] == 0) | (r[..., 0] == 11))
        bits = np.ascontiguousarray(n32).view(np.uint32)
        bi, bj = bits[:, None, :], bits[idx]
        same = (bi == bj).all(axis=-1) | (bi == (bj ^ np.uint32(0x80000000))).all(axis=-1)
        tie = (np.abs(np.abs(ai) - np.abs(aj)) < TOL) & ~same
        sens_pair = on & (near.any(axis=-1) | tie)
    res["sensitive"] = sens_pair.any(axis=1)
    res["excluded"] = res["sensitive"] | (nb & res["sensitive"][idx]).any(axis=1)
    counts = res["counts"]
    rows = np.broadcast_to(np.arange(M)[:, None], on.shape)
    for f in range(3):
        np.add.at(counts, (rows[on], 11 * f + b[..., f][on]), 1)
    mm = counts[:, :11].sum(axis=1)
    res["m"] = mm
    assert (counts[:, 11:22].sum(axis=1) == mm).all() and (counts[:, 22:].sum(axis=1) == mm).all() and counts.max(initial=0) <= 31
    acc = np.zeros((M, 33), T)
    with np.errstate(all="ignore"):
        for s in range(k):                                                   # list order
            j = idx[:, s]
            use = nb[:, s] & (mm[j] > 0)
            term = (counts[j].astype(T) / np.maximum(mm[j], 1).astype(T)[:, None]) / d2[:, s].astype(T)[:, None]
            acc = np.where(use[:, None], acc + term, acc)
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


def plain_double(model, normals, k: int):
    """the contract in Python floats, one pair at a time -> (counts [M, 33] int64, out [M, 33] float64)"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    n32 = np.asarray(normals, np.float32).reshape(-1, 3)
    M = len(m)
    counts = np.zeros((M, 33), np.int64)
    out = np.zeros((M, 33), np.float64)
    if M == 0:
        return counts, out
    idx, d2, nb = neighbours(m, k)
    P, N = m.astype(np.float64).tolist(), n32.astype(np.float64).tolist()
    fin = [all(math.isfinite(c) for c in row) for row in N]
    sqrt, atan2, floor, pi = math.sqrt, math.atan2, math.floor, math.pi

    def bin_of(x):
        return int(min(max(floor(11.0 * x), 0.0), 10.0))

    for i in range(M):
        pi_, ni = P[i], N[i]
        for s in range(k):
            if not nb[i, s]:
                continue
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
        for s in range(k):
            j = int(idx[i, s])
            if nb[i, s] and mm[j] > 0:
                mj, w = float(mm[j]), float(d2[i, s])
                cj = counts[j]
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
def family_inputs(name: str, M: int = M_FAMILY):
    """-> (model [M, 3] float32, normals [M, 3] float32): normals_ref's at K_NORMALS, oriented to VIEWPOINT, rounded to fp32"""
    model = normals_ref.family(name, M)
    r = normals_ref.normals(model, K_NORMALS, viewpoint=VIEWPOINT)
    nrm = normals_ref.oriented(r, model, VIEWPOINT).astype(np.float32)
    assert np.isfinite(nrm).all()
    model.setflags(write=False)
    nrm.setflags(write=False)
    return model, nrm


@functools.lru_cache(maxsize=None)
def case(name: str, k: int):
    model, nrm = family_inputs(name)
    r = fpfh(model, nrm, k)
    for a in r.values():
        a.setflags(write=False)
    return r


def excluded_share(r: dict) -> float:
    return float(r["excluded"].mean()) if len(r["excluded"]) else 0.0
