"""The direct-answer rule of the two-nearest search (pcreg_amd/csrc/direct_rule.hpp, DESIGN 4.1 "Direct answers") restated in
numpy: float64 for the radius, np.float32 for everything the device does in fp32.

A seeded query q with seed distance dk is answered from the ordering-grid cells [cell(lo_c), cell(hi_c)] per axis, where
rho = sqrt(dk (1 + 4u) + 2^-149) (1 + 4u) in float64, lo_c the largest float32 <= q_c - rho, hi_c the smallest float32 >=
q_c + rho and cell() the ordering grid's per-axis expression.  It is eligible when dk and its coordinates are finite, the
range holds at most CELLS cells and those cells at most ROWS rows."""
import numpy as np

U = 2.0 ** -24
CELLS = 27                       # direct_rule.hpp: kDirectCells
ROWS = 512                       # direct_rule.hpp: kDirectRows
TOP = 63                         # knn_fast_common.hpp: 2^kSortBits - 1
F32 = np.float32


def radius(dk):
    dk = np.asarray(dk, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.sqrt(dk * (1.0 + 4.0 * U) + 2.0 ** -149) * (1.0 + 4.0 * U)


def float_below(t):
    """the largest float32 <= t (t float64, no NaN)"""
    with np.errstate(over="ignore"):
        f = np.asarray(t, np.float64).astype(F32)
        return np.where(f.astype(np.float64) > t, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def float_above(t):
    with np.errstate(over="ignore"):
        f = np.asarray(t, np.float64).astype(F32)
        return np.where(f.astype(np.float64) < t, np.nextafter(f, F32(np.inf)), f).astype(F32)


def cell(v, s0, inv_s, top=TOP):
    """the ordering grid's cell of coordinate v on one axis, as sort_key forms it (fp32; NaN -> 0)"""
    v, s0, inv_s = np.asarray(v, F32), np.asarray(s0, F32), F32(inv_s)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(((v - s0).astype(F32) * inv_s).astype(F32))
    return np.fmin(np.fmax(c, F32(0)), F32(top)).astype(np.int64)


def bounds(q, dk):
    """(lo, hi) [Q, 3] float32: the coordinates whose cells bound the range"""
    q = np.asarray(q, F32).reshape(-1, 3)
    rho = radius(dk).reshape(-1, 1)
    q64 = q.astype(np.float64)
    return float_below(q64 - rho), float_above(q64 + rho)


def cell_range(q, dk, s0, inv_s, top=TOP):
    """(finite [Q] bool, lo [Q, 3], hi [Q, 3] int64); a query that is not finite has the range 0 .. 0"""
    q = np.asarray(q, F32).reshape(-1, 3)
    dk = np.asarray(dk, F32).reshape(-1)
    fin = np.isfinite(dk) & (dk >= 0) & np.isfinite(q).all(axis=1)
    qq, dd = np.where(fin[:, None], q, F32(0)), np.where(fin, dk, F32(0))
    lo_f, hi_f = bounds(qq, dd)
    s0 = np.asarray(s0, F32)
    lo, hi = cell(lo_f, s0, inv_s, top), cell(hi_f, s0, inv_s, top)
    lo[~fin] = 0
    hi[~fin] = 0
    return fin, lo, hi


def spread(v):
    v = np.asarray(v).astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton(c):
    c = np.asarray(c)
    return (spread(c[..., 0]) | (spread(c[..., 1]) << np.uint32(1)) | (spread(c[..., 2]) << np.uint32(2))).astype(np.int64)


def eligible(q, dk, sorted_rows, s0, inv_s, top=TOP):
    """-> dict: finite, lo, hi, cells [Q], rows [Q] (rows of the range's cells; -1 where the query is not finite or the range is over CELLS), ok [Q].
    sorted_rows: the prepared model's rows (any order: only their cells count)."""
    fin, lo, hi = cell_range(q, dk, s0, inv_s, top)
    n = (hi - lo + 1).prod(axis=1)
    keys = morton(np.stack([cell(np.asarray(sorted_rows, F32)[:, c], np.asarray(s0, F32)[c], inv_s, top) for c in range(3)], axis=1))
    count = np.bincount(keys, minlength=(top + 1) ** 3)
    rows = np.full(len(n), -1, np.int64)
    for i in np.flatnonzero(fin & (n <= CELLS)):
        g = np.stack(np.meshgrid(*[np.arange(lo[i, c], hi[i, c] + 1) for c in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
        rows[i] = count[morton(g)].sum()
    ok = fin & (n <= CELLS) & (rows >= 0) & (rows <= ROWS)
    return dict(finite=fin, lo=lo, hi=hi, cells=n, rows=rows, ok=ok)
