"""DBSCAN's contract (include/pcreg.h) restated by brute force in numpy.

Rows i and j (j may be i) are neighbours iff both are finite and fmaf(dz,dz,fmaf(dy,dy,dx*dx)) <= r2, every step rounded to
float32 once -- the predicate of tests/cluster_ref.c, formed here without a compiler: a product of two float32 is exact in float64,
and the sum behind it is brought to float32 with ONE rounding by rounding the float64 sum to odd first (TwoSum gives its error).
count[i] = the neighbours of i, itself included; core = count >= minpts; the clusters are the connected components of the core
rows under the neighbour relation, numbered in ascending order of their smallest core row; a row that is not core and has a core
neighbour takes the smallest NUMBER among its core neighbours' clusters; every other row is noise, -1.

dbscan(points, r2, minpts) -> dict(label, core, count, n_clusters, first, sizes, cl_off, members).  neighbours() compares every
pair; neighbours_grid() takes its candidates from a grid of cells a little wider than the radius and decides them by the same
formula, for the one larger cloud.  Both return the neighbour lists in CSR form, which a test may compute once per (cloud, r2) and
hand to dbscan_from(...) for every minpts.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def _fmaf_sq(a, c):
    """float32(a * a + c) with one rounding, for float32 a and float32 c >= 0 (finite)"""
    p = a.astype(F64) * a.astype(F64)                       # exact: 48 bits
    c = c.astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                           # TwoSum: p + c = s + e exactly
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    inexact = e != 0
    bits[inexact & (e < 0)] -= 1                            # (s > 0 here) the sum cut off towards zero ...
    bits[inexact] |= 1                                      # ... and made odd: the float32 rounding behind it is the one rounding
    with np.errstate(over="ignore"):
        return bits.view(F64).astype(F32)


def chain_d2(a, b):
    """fmaf(dz,dz,fmaf(dy,dy,dx*dx)) of float32 rows a [.., 3] and b [.., 3] (broadcast), float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (np.asarray(a[..., c] - b[..., c], F32) for c in range(3))
        return _fmaf_sq(dz, _fmaf_sq(dy, np.asarray(dx * dx, F32)))


def _points(points):
    return np.ascontiguousarray(np.asarray(points, F32).reshape(-1, 3))


def d2_matrix(points):
    """the chain distance of every pair of FINITE rows, [F, F] float32: what neighbours() compares with r2, for a caller that tries
    several radii on one small cloud"""
    m = _points(points)
    mf = m[np.isfinite(m).all(axis=1)]
    out = np.empty((len(mf), len(mf)), F32)
    step = max(1, 4_000_000 // max(len(mf), 1))
    for a0 in range(0, len(mf), step):
        out[a0:a0 + step] = chain_d2(mf[a0:a0 + step, None, :], mf[None, :, :])
    return out


def neighbours(points, r2, d2=None):
    """-> (indptr [M + 1], indices): row i's neighbours, itself included, ascending; none for a non-finite row.  d2: d2_matrix(points)"""
    m = _points(points)
    M = len(m)
    r2 = F32(r2)
    fin = np.isfinite(m).all(axis=1)
    rows = np.flatnonzero(fin)
    mf = m[rows]
    src, dst = [], []
    step = max(1, 4_000_000 // max(len(mf), 1))
    for a0 in range(0, len(mf), step):
        hit = (chain_d2(mf[a0:a0 + step, None, :], mf[None, :, :]) if d2 is None else d2[a0:a0 + step]) <= r2
        s, d = np.nonzero(hit)
        src.append(rows[a0 + s]); dst.append(rows[d])
    return _csr(M, np.concatenate(src) if src else np.zeros(0, np.int64), np.concatenate(dst) if dst else np.zeros(0, np.int64))


def _csr(M, src, dst):
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    indptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=M), out=indptr[1:])
    return indptr, dst.astype(np.int64)


def neighbours_grid(points, r2):
    """neighbours() with the candidates of a cell grid: cells of 1.001 * sqrt(r2), a row against the 27 cells around its own"""
    m = _points(points)
    M = len(m)
    r2 = F32(r2)
    assert 0 < r2 < np.inf
    fin = np.isfinite(m).all(axis=1)
    rows = np.flatnonzero(fin)
    mf = m[rows].astype(F64)
    cell = np.floor((mf - mf.min(axis=0)) / (1.001 * np.sqrt(F64(r2)))).astype(np.int64) + 1
    n = cell.max(axis=0) + 2
    key = (cell[:, 0] * n[1] + cell[:, 1]) * n[2] + cell[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    src, dst = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                k = key + (ox * n[1] + oy) * n[2] + oz
                lo, hi = np.searchsorted(skey, k, "left"), np.searchsorted(skey, k, "right")
                cnt = hi - lo
                s = np.repeat(np.arange(len(mf)), cnt)
                d = order[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
                hit = chain_d2(m[rows[s]], m[rows[d]]) <= r2
                src.append(rows[s[hit]]); dst.append(rows[d[hit]])
    return _csr(M, np.concatenate(src), np.concatenate(dst))


def dbscan_from(adj, minpts):
    indptr, indices = adj
    M = len(indptr) - 1
    minpts = int(minpts)
    assert minpts >= 1
    count = np.diff(indptr).astype(np.int32)
    core = count >= minpts
    src = np.repeat(np.arange(M), count)
    # the components of the core rows: every core row takes the smallest row number among its core neighbours (itself one of them)
    # and then that row's, until nothing changes; comp[i] ends as the smallest core row of i's component
    cc = core[src] & core[indices]
    s, d = src[cc], indices[cc]
    crow = np.flatnonzero(core)
    starts = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=M)[crow])[:-1]]).astype(np.int64)
    comp = np.arange(M)
    while len(crow):
        new = comp.copy()
        new[crow] = np.minimum.reduceat(comp[d], starts)
        new = new[new]
        if np.array_equal(new, comp):
            break
        comp = new
    first = np.unique(comp[core]).astype(np.int32)             # ascending: cluster c's smallest core row
    label = np.full(M, -1, np.int32)
    label[core] = np.searchsorted(first, comp[core])
    # border rows: the smallest cluster NUMBER among the core neighbours
    bc = ~core[src] & core[indices]
    best = np.full(M, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(best, src[bc], label[indices[bc]])
    border = ~core & (best < np.iinfo(np.int32).max)
    label[border] = best[border]
    nc = len(first)
    sizes = np.bincount(label[label >= 0], minlength=nc).astype(np.int32)
    cl_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = np.argsort(np.where(label >= 0, label, nc), kind="stable")[:cl_off[-1]].astype(np.int32)
    return dict(label=label, core=core, count=count, n_clusters=nc, first=first, sizes=sizes, cl_off=cl_off, members=members,
                border=border, noise=label < 0)


def lattice_cloud(seed, M):
    """M rows with integer coordinates in [0, 12)^3: a few dense blobs, a sparse background, coincident rows"""
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(1, 5))
    centres = rng.integers(2, 10, (nb, 3))
    blob = centres[rng.integers(0, nb, M)] + np.rint(rng.normal(0.0, 1.2, (M, 3))).astype(np.int64)
    back = rng.integers(0, 12, (M, 3))
    pts = np.where(rng.random((M, 1)) < 0.6, blob, back)
    return np.clip(pts, 0, 11).astype(np.float32)


def dbscan(points, r2, minpts, grid=False):
    return dbscan_from((neighbours_grid if grid else neighbours)(points, r2), minpts)
