"""Host reference of the point search's tile-culling rule, in plain numpy.

Written from the rule as DESIGN 4.1 states it, not from the kernel: the queries of a search call sit in slots
(`qperm[slot] = query`, the call's spatial order), 512 slots make a query block.  A block only looks at its SCORED queries,
those whose scaled offset `fp32(sigma * (p - c))` stays within 16384 on every axis, and none at all when sigma^2 or
1/sigma^2 is not a normal fp32 number.  Over them it forms a box B and the
largest seed distance D, where any +inf seed distance turns culling off for the block.  A model tile with box T is skipped
when the gaps g_c = max(0, T.lo_c - B.hi_c, B.lo_c - T.hi_c), formed in float64, give G2 = g_x^2 + g_y^2 + g_z^2 with
G2 > 1e-30 and G2 (1 - 32u) > D, u = 2^-24.  A block without a scored query visits no tile.

The preparation record `prep` is the 24-word array pcreg_debug_dev_model_export returns; only its centre (words 0-2) and
scale sigma (word 4) matter here.  tests/test_knn_cull_ref.py pins the rule on hand-made boxes; tests/test_gpu_knn_cull.py
compares the device's visited count with it.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
BLOCK = 512                      # query slots per block
TILE = 512                       # sorted model rows per tile
QUERY_SCALED_MAX = np.float32(16384.0)
PREP_CX, PREP_SIGMA = 0, 4       # word offsets in the exported preparation record


def make_prep(sigma: float, centre) -> np.ndarray:
    """A 24-word preparation record with only the fields the rule reads (for hand-made cases)."""
    p = np.zeros(24, np.float32)
    p[PREP_CX:PREP_CX + 3] = np.asarray(centre, np.float32)
    p[PREP_SIGMA] = np.float32(sigma)
    return p


def scale_usable(prep: np.ndarray) -> bool:
    """sigma^2 and 1/sigma^2 are both normal fp32 numbers (the model's half extent lies in [2^-58, 2^69))"""
    sg = np.float32(prep[PREP_SIGMA])
    tiny = np.finfo(np.float32).tiny
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        s2 = sg * sg
        inv = np.float32(1.0) / s2
    return bool(tiny <= s2 < np.inf and tiny <= inv < np.inf)


def scored(q: np.ndarray, prep: np.ndarray) -> np.ndarray:
    """[Q] bool: the model's scale is usable and the query's fp32 scaled offset from the model's centre is within 16384 on
    every axis (NaN is not)."""
    q = np.asarray(q, np.float32)
    if not scale_usable(prep):
        return np.zeros(len(q), bool)
    c = np.asarray(prep[PREP_CX:PREP_CX + 3], np.float32)
    sg = np.float32(prep[PREP_SIGMA])
    with np.errstate(invalid="ignore", over="ignore"):
        s = sg * (q - c)                                      # float32 throughout, as the search forms it
        return np.all(np.abs(s) <= QUERY_SCALED_MAX, axis=1)


def block_bounds(q, qperm, dk, prep):
    """Per query block: (lo [nb, 3], hi [nb, 3], D [nb], any_scored [nb]) over the block's scored queries.  lo / hi are the
    float32 box, D the largest seed distance as float64 (+inf when one of them is not finite)."""
    q = np.asarray(q, np.float32)
    qperm = np.asarray(qperm, np.int64)
    dk = np.asarray(dk, np.float32)
    Q = len(qperm)
    nb = (Q + BLOCK - 1) // BLOCK
    ok = scored(q, prep)
    lo = np.full((nb, 3), np.inf, np.float32)
    hi = np.full((nb, 3), -np.inf, np.float32)
    D = np.zeros(nb, np.float64)
    has = np.zeros(nb, bool)
    for b in range(nb):
        rows = qperm[b * BLOCK:(b + 1) * BLOCK]
        rows = rows[ok[rows]]
        if len(rows) == 0:
            continue
        has[b] = True
        lo[b] = q[rows].min(axis=0)
        hi[b] = q[rows].max(axis=0)
        d = dk[rows].astype(np.float64)
        D[b] = np.inf if not np.all(d < np.inf) else max(0.0, float(d.max()))
    return lo, hi, D, has


def gap2(lo, hi, tile_box) -> np.ndarray:
    """[nb, nt] float64 G2 between every block box and every tile box (tile_box [nt, 6]: lo xyz, hi xyz)."""
    lo = np.asarray(lo, np.float64)[:, None, :]
    hi = np.asarray(hi, np.float64)[:, None, :]
    tb = np.asarray(tile_box, np.float32).reshape(-1, 6).astype(np.float64)
    tlo, thi = tb[None, :, :3], tb[None, :, 3:]
    with np.errstate(invalid="ignore"):
        g = np.maximum(0.0, np.maximum(tlo - hi, lo - thi))
    g = np.where(np.isnan(g), np.inf, g)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def skip(G2, D) -> np.ndarray:
    """The rule itself: skip when G2 > 1e-30 and G2 (1 - 32u) > D (D broadcast over tiles)."""
    G2 = np.asarray(G2, np.float64)
    D = np.asarray(D, np.float64)
    if D.ndim == 1 and G2.ndim == 2:
        D = D[:, None]
    return (G2 > 1e-30) & (G2 * (1.0 - 32.0 * U) > D)


def visited_pairs(q, qperm, dk, tile_box, prep) -> np.ndarray:
    """[n_blocks, n_tiles] bool: the (query block, tile) pairs the candidate kernel must visit."""
    lo, hi, D, has = block_bounds(q, qperm, dk, prep)
    vis = ~skip(gap2(lo, hi, tile_box), D)
    vis[~has] = False
    return vis


def visited_count(q, qperm, dk, tile_box, prep) -> int:
    return int(visited_pairs(q, qperm, dk, tile_box, prep).sum())


def query_blocks(qperm) -> np.ndarray:
    """[Q] the block of every query (inverse of the slot order, divided by 512)."""
    qperm = np.asarray(qperm, np.int64)
    slot = np.empty_like(qperm)
    slot[qperm] = np.arange(len(qperm))
    return slot // BLOCK


def row_tiles(perm) -> np.ndarray:
    """[M] the tile of every ORIGINAL model row (perm[sorted row] = original row)."""
    perm = np.asarray(perm, np.int64)
    pos = np.empty_like(perm)
    pos[perm] = np.arange(len(perm))
    return pos // TILE
