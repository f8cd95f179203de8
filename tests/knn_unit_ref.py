"""Host reference of the point search's UNIT rule ("units"), in plain numpy float64.

Written from the rule as DESIGN 4.1 states it, not from the kernels.  Inside a tile that a query block visits (the block rule,
tests/knn_cull_ref.py) the candidate kernel scores 64-row UNITS per WAVE: wave v of a block holds the query slots
[128 v, 128 v + 128) of the block's 512, unit s of a tile its sorted rows [64 s, 64 s + 64).  For every listed (block, tile)
pair there is one 32-bit mask, byte v for wave v, bit s of the byte for unit s.  A bit is set unless the block rule's test
skips the pair (B, D, T) with

    B = the float32 box of the wave's SCORED queries,  D = their largest seed distance,  T = the unit's box,

i.e. the gaps in float64 give G2 > 1e-30 and G2 (1 - 32u) > D.  A unit's box covers the rows it has; a unit whose rows all lie
at or past M is empty and is never kept by the test (its box is (+inf, -inf): G2 = +inf).  Three cases come before the test:
culling switched off keeps every unit of every tile; a wave holding a scored query whose seed distance is +inf keeps every unit
of every listed tile; a wave without a scored query keeps none.  A pair the block does not list has no mask (0 here).

The sub-boxes are taken from the exported sorted copy (`ms` [M, 3], pcreg_debug_dev_model_export), the query order and seed
distances from pcreg_debug_search_export.  tests/test_knn_unit_ref.py pins this file on hand-made boxes;
tests/test_gpu_knn_units.py compares the device's unit counter with it.
"""
from __future__ import annotations

import numpy as np

import knn_cull_ref as cull

WAVE = 128                       # query slots per candidate wave
WAVES = cull.BLOCK // WAVE       # 4
UNIT = 64                        # sorted model rows per unit
UNITS = cull.TILE // UNIT        # 8


def unit_boxes(ms) -> np.ndarray:
    """[n_tiles * 8, 6] float32 (lo xyz, hi xyz) of every unit of the sorted copy ms [M, 3]; empty units (+inf, -inf)."""
    ms = np.asarray(ms, np.float32).reshape(-1, 3)
    M = len(ms)
    nt = max((M + cull.TILE - 1) // cull.TILE, 1)
    out = np.empty((nt * UNITS, 6), np.float32)
    out[:, :3] = np.inf
    out[:, 3:] = -np.inf
    for s in range((M + UNIT - 1) // UNIT):
        rows = ms[s * UNIT:(s + 1) * UNIT]
        out[s, :3] = rows.min(axis=0)
        out[s, 3:] = rows.max(axis=0)
    return out


def wave_bounds(q, qperm, dk, prep):
    """Per (block, wave): lo [nb, 4, 3], hi [nb, 4, 3] float32, D [nb, 4] float64 (+inf when a scored query's seed distance is not
    finite), has [nb, 4] -- over the wave's scored queries."""
    q = np.asarray(q, np.float32)
    qperm = np.asarray(qperm, np.int64)
    dk = np.asarray(dk, np.float32)
    nb = (len(qperm) + cull.BLOCK - 1) // cull.BLOCK
    ok = cull.scored(q, prep)
    lo = np.full((nb, WAVES, 3), np.inf, np.float32)
    hi = np.full((nb, WAVES, 3), -np.inf, np.float32)
    D = np.zeros((nb, WAVES), np.float64)
    has = np.zeros((nb, WAVES), bool)
    for b in range(nb):
        for v in range(WAVES):
            rows = qperm[b * cull.BLOCK + v * WAVE:b * cull.BLOCK + (v + 1) * WAVE]
            rows = rows[ok[rows]]
            if len(rows) == 0:
                continue
            has[b, v] = True
            lo[b, v] = q[rows].min(axis=0)
            hi[b, v] = q[rows].max(axis=0)
            d = dk[rows].astype(np.float64)
            D[b, v] = np.inf if not np.all(d < np.inf) else max(0.0, float(d.max()))
    return lo, hi, D, has


def unit_keep(lo, hi, D, has, ubox) -> np.ndarray:
    """[nb, 4, n_units] bool: what the unit rule alone keeps, whatever the block lists (culling on)."""
    nb = lo.shape[0]
    G2 = cull.gap2(lo.reshape(nb * WAVES, 3), hi.reshape(nb * WAVES, 3), ubox).reshape(nb, WAVES, -1)
    keep = ~cull.skip(G2, D[:, :, None])
    keep |= np.isinf(D)[:, :, None]                       # an unseeded query meets every point
    keep &= has[:, :, None]
    return keep


def listed_pairs(q, qperm, dk, tile_box, prep, cull_on=True) -> np.ndarray:
    """[nb, nt] bool: the block-level list (every pair when culling is off)."""
    vis = cull.visited_pairs(q, qperm, dk, tile_box, prep)
    return vis if cull_on else np.ones_like(vis)


def unit_masks(q, qperm, dk, tile_box, ubox, prep, cull_on=True) -> np.ndarray:
    """[nb, nt] uint32: the mask of every (block, tile) pair, 0 where the block does not list the tile."""
    listed = listed_pairs(q, qperm, dk, tile_box, prep, cull_on)
    nb, nt = listed.shape
    if not cull_on:
        return np.full((nb, nt), 0xFFFFFFFF, np.uint32)
    keep = unit_keep(*wave_bounds(q, qperm, dk, prep), ubox).reshape(nb, WAVES, nt, UNITS)
    weight = (np.uint64(1) << (np.arange(WAVES, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(UNITS, dtype=np.uint64)[None, :]))
    mask = (keep.transpose(0, 2, 1, 3).astype(np.uint64) * weight[None, None]).sum(axis=(2, 3)).astype(np.uint32)
    return np.where(listed, mask, np.uint32(0))


def popcount(mask) -> np.ndarray:
    m = np.asarray(mask, np.uint32)
    return np.unpackbits(m.reshape(-1, 1).view(np.uint8), axis=1).sum(axis=1).reshape(m.shape)


def unit_stats(q, qperm, dk, tile_box, ubox, prep, cull_on=True):
    """(units scored, 32 x listed tiles): what pcreg_debug_knn_unit_stats counts for one search."""
    listed = listed_pairs(q, qperm, dk, tile_box, prep, cull_on)
    return int(popcount(unit_masks(q, qperm, dk, tile_box, ubox, prep, cull_on)).sum()), 32 * int(listed.sum())


def row_units(perm) -> np.ndarray:
    """[M] the global unit (tile * 8 + unit) of every ORIGINAL model row."""
    perm = np.asarray(perm, np.int64)
    pos = np.empty_like(perm)
    pos[perm] = np.arange(len(perm))
    return pos // UNIT


def query_waves(qperm):
    """([Q] block, [Q] wave) of every query."""
    qperm = np.asarray(qperm, np.int64)
    slot = np.empty_like(qperm)
    slot[qperm] = np.arange(len(qperm))
    return slot // cull.BLOCK, (slot % cull.BLOCK) // WAVE


def answers_in_visited_units(mask, perm, qperm, idx, ok) -> np.ndarray:
    """[Q, 2] bool: each answer's unit is set in its query's wave byte (True for queries outside `ok`)."""
    blk, wav = query_waves(qperm)
    gu = row_units(perm)
    out = np.ones(idx.shape, bool)
    for k in range(idx.shape[1]):
        u = gu[idx[:, k]]
        bit = (mask[blk, u // UNITS] >> (8 * wav + u % UNITS).astype(np.uint32)) & np.uint32(1)
        out[:, k] = np.where(ok, bit == 1, True)
    return out
