"""The unit rule of the point search (knn_mfma16.hip, DESIGN 4.1 "units") against tests/knn_unit_ref.py.

Inside a visited tile a candidate wave scores only the 64-row units that the culling rule cannot rule out for its own 128
queries.  Results alone would not show a unit that was scored for nothing, and the exact tail would hide one that was skipped
wrongly whenever the certificate happens to fail.  So every case here compares idx and dist bit for bit with the C oracle AND
the device's unit counter ("knn_stats", pcreg_debug_knn_unit_stats) exactly with the float64 reference evaluated on what the
library exports (sorted copy, tile boxes, query order, seed distances).  The shapes are small: M between 20 000 and 40 000 rows
(above the seeding threshold of 16 384), Q between 600 and 1 600 (single queries in the lattice cases).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import knn_cull_ref as cull
import knn_unit_ref as uref
from test_gpu_knn_cull import BOX, CORES, U, Model, _bits, _crop, _seed_cells, _stats

pytestmark = pytest.mark.gpu


def _unit_stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 2)()
    check(lib().pcreg_debug_knn_unit_stats(out, 1 if reset else 0))
    return int(out[0]), int(out[1])


@pytest.fixture
def stats_on(debug_set):
    debug_set("knn_stats", 1)
    _stats(reset=True)
    _unit_stats(reset=True)
    return debug_set


class Run:
    """One search with everything the checks need: results, the exported order and seed distances, both counters, the reference's
    masks."""

    def __init__(self, pm, surf, stats_on, nocull=False):
        self.surf = np.asarray(surf, np.float32)
        _unit_stats(reset=True)
        self.idx, self.dist, self.qperm, self.dk, self.st = pm.search(self.surf, nocull=nocull, debug_set=stats_on)
        self.units = _unit_stats(reset=True)
        self.ubox = uref.unit_boxes(pm.ms)
        self.masks = uref.unit_masks(self.surf, self.qperm, self.dk, pm.tbox, self.ubox, pm.prep, cull_on=not nocull)
        self.listed = uref.listed_pairs(self.surf, self.qperm, self.dk, pm.tbox, pm.prep, cull_on=not nocull)
        self.expected = uref.unit_stats(self.surf, self.qperm, self.dk, pm.tbox, self.ubox, pm.prep, cull_on=not nocull)


def _check(pm, run, oracle_c, model):
    """the checks every case shares: the counters against the reference, the answers against the oracle and inside visited units"""
    print(f"units {run.units[0]} of {run.units[1]} (reference {run.expected[0]} of {run.expected[1]}); tail {run.st[3]}")
    assert run.units == run.expected
    assert run.units[1] == 32 * run.st[1]
    ri, rd = oracle_c.knn2_points_f32(run.surf, model, nthreads=CORES)
    np.testing.assert_array_equal(run.idx, ri)
    np.testing.assert_array_equal(_bits(run.dist), _bits(rd))
    ok = cull.scored(run.surf, pm.prep)
    inside = uref.answers_in_visited_units(run.masks, pm.perm, run.qperm, ri, ok)
    assert inside.all(), f"{int((~inside).sum())} answers lie in units their wave does not visit"
    return ri, rd


@pytest.fixture(scope="module")
def uniform_model():
    rng = np.random.default_rng(61)
    return (rng.random((30_000, 3)) * BOX).astype(np.float32)


def test_crop_like_surface_and_nocull(uniform_model, stats_on, oracle_c):
    model = uniform_model
    surf = _crop(model, 1500, BOX * 0.4, 62)
    pm = Model(model)
    try:
        run = Run(pm, surf, stats_on)
        assert run.expected[0] < run.expected[1], "premise: the unit rule culls inside visited tiles"
        assert np.any(run.listed & (run.masks == 0)), "premise: a listed tile no wave needs a unit of"
        _check(pm, run, oracle_c, model)
        # culling off: every unit of every tile, the same bits
        off = Run(pm, surf, stats_on, nocull=True)
        nb = (len(surf) + cull.BLOCK - 1) // cull.BLOCK
        assert off.units == off.expected == (32 * nb * pm.n_tiles, 32 * nb * pm.n_tiles)
        np.testing.assert_array_equal(off.idx, run.idx)
        np.testing.assert_array_equal(_bits(off.dist), _bits(run.dist))
    finally:
        pm.close()


def test_one_unseeded_query_keeps_every_unit_for_its_wave_only(stats_on, oracle_c):
    """The model's corner x > 80, y > 50, z > 50 is empty; one scored query at (95, 95, 95) finds its 27 seeding cells empty
    (dk = +inf).  Its block lists every tile and its wave scores every unit of them; the block's other waves still cull."""
    rng = np.random.default_rng(41)
    model = (rng.random((38_000, 3)) * 100.0).astype(np.float32)
    model = model[~((model[:, 0] > 80) & (model[:, 1] > 50) & (model[:, 2] > 50))]
    assert 20_000 <= len(model) <= 40_000
    crop = _crop(model, 700, np.array([90.0, 90.0, 20.0]), 42, noise=0.02)
    corner = np.array([[95.0, 95.0, 95.0]], np.float32)
    surf = np.vstack([crop, corner]).astype(np.float32)
    pm = Model(model)
    try:
        run = Run(pm, surf, stats_on)
        assert run.dk[-1] == np.inf and np.all(np.isfinite(run.dk[:-1])), "premise: only the corner query is unseeded"
        assert cull.scored(corner, pm.prep).all()
        blk, wav = uref.query_waves(run.qperm)
        b, v = int(blk[-1]), int(wav[-1])
        assert run.listed[b].all()
        byte = (run.masks[b] >> np.uint32(8 * v)) & np.uint32(0xFF)
        assert np.all(byte == 0xFF)
        _, _, _, has = uref.wave_bounds(surf, run.qperm, run.dk, pm.prep)
        others = [w for w in range(uref.WAVES) if w != v and has[b, w]]
        assert others, "premise: the corner query's block holds other scored waves"
        for w in others:
            ob = (run.masks[b] >> np.uint32(8 * w)) & np.uint32(0xFF)
            assert np.any(ob != 0xFF), "premise: the other waves of the block still cull"
        _check(pm, run, oracle_c, model)
    finally:
        pm.close()


def test_a_wave_of_unscored_queries_next_to_scored_waves(uniform_model, stats_on, oracle_c):
    """300 copies of one query far outside kQueryScaledMax share an ordering cell, so they fill a run of 300 slots: one whole wave
    of 128 at least, in a block whose other waves hold scored queries.  That wave's byte is 0 on every listed tile."""
    model = uniform_model
    crop = _crop(model, 900, BOX * 0.5, 63)
    far = np.tile(np.array([[50.0, -7e8, 50.0]], np.float32), (300, 1))
    rng = np.random.default_rng(64)
    surf = np.vstack([crop, far])[rng.permutation(1200)].astype(np.float32)
    pm = Model(model)
    try:
        run = Run(pm, surf, stats_on)
        assert not cull.scored(far[:1], pm.prep).any()
        _, _, _, has = uref.wave_bounds(surf, run.qperm, run.dk, pm.prep)
        pairs = [(b, v) for b in range(has.shape[0]) for v in range(uref.WAVES) if not has[b, v] and has[b].any()
                 and (b * cull.BLOCK + (v + 1) * uref.WAVE) <= len(surf)]
        assert pairs, "premise: a full wave without a scored query inside a block that scores"
        for b, v in pairs:
            assert run.listed[b].any()
            assert np.all(((run.masks[b] >> np.uint32(8 * v)) & np.uint32(0xFF)) == 0)
        assert run.st[3] >= 300, "the unscored queries go to the exact tail"
        _check(pm, run, oracle_c, model)
    finally:
        pm.close()


def test_ragged_model_and_ragged_last_wave(stats_on, oracle_c):
    """M = 30 037: the last tile holds 341 rows -- five full units, one of 21 rows, two empty.  Q = 1228: the last block holds one
    full wave and one of 76 queries.  Queries near rows all over the model, the last tile's among them."""
    rng = np.random.default_rng(65)
    M, Q = 30_037, 1228
    assert M % 512 == 341 and M % 64 == 21 and Q % 512 == 128 + 76
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    try:
        last = pm.perm[(pm.n_tiles - 1) * cull.TILE:]                       # original rows of the last tile
        near = np.concatenate([last[rng.choice(len(last), 200, replace=False)], rng.choice(M, Q - 200, replace=False)])
        surf = (model[near] + rng.normal(0, 0.05, (Q, 3))).astype(np.float32)
        run = Run(pm, surf, stats_on)
        lt = pm.n_tiles - 1
        assert np.all(np.isinf(run.ubox[lt * 8 + 6:, 0])) and np.isfinite(run.ubox[lt * 8 + 5, 0]), "premise: units 6, 7 of the last tile are empty"
        assert run.listed[:, lt].any(), "premise: the last tile is visited"
        fin = np.isfinite(run.dk)
        assert fin.all(), "premise: every query is seeded (no wave keeps the empty units)"
        for v in range(uref.WAVES):
            assert np.all(((run.masks[:, lt] >> np.uint32(8 * v)) & np.uint32(0xC0)) == 0), "an empty unit is scored"
        assert np.any(run.masks[:, lt] & np.uint32(0x20202020)), "premise: the partly filled unit is scored by some wave"
        _check(pm, run, oracle_c, model)
    finally:
        pm.close()


# ---- the two tie cases of test_gpu_knn_cull.py, one level down --------------------------------------------------------
def _unit_lattice_case(a, stats_on, oracle_c, n=32):
    """An n^3 lattice of spacing a (coordinates i * a exact in fp32); every ordering cell holds one node, so the sorted order is
    fixed.  A query sits on a node q whose +-axis neighbour m lies in the SAME tile but in another unit W, whose box is exactly a
    away on that axis only: G2(q, W) = a^2 in float64 while dk = fl32(a^2).  The block visits the tile anyway (it holds q), so
    only the unit rule decides whether m is scored.  m gets the lowest original row of the model, so it is the second answer.
    Whether the certificate passes or the exact tail answers instead (_check prints the tail's count), the unit counter must equal
    the reference's, which keeps W, and W must be set in the reference's mask of the query's wave."""
    g = np.arange(n, dtype=np.float32) * np.float32(a)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    base = Model(nodes)
    try:
        pos = np.empty(len(nodes), np.int64)
        pos[base.perm] = np.arange(len(nodes))
        tile_of, unit_of = pos // cull.TILE, pos // uref.UNIT
        seed_cell = _seed_cells(nodes, base.prep)
        seed_cnt = np.bincount(seed_cell[seed_cell >= 0])
        ub = uref.unit_boxes(base.ms).astype(np.float64)
        lut = {tuple(np.round(p / np.float32(a)).astype(int)): i for i, p in enumerate(nodes)}
        picks, used = [], np.zeros(len(nodes), bool)
        for qi in np.random.default_rng(3).permutation(len(nodes)):
            if len(picks) >= 6:
                break
            ijk = np.round(nodes[qi] / np.float32(a)).astype(int)
            if np.any(ijk < 2) or np.any(ijk > n - 3) or used[qi]:
                continue
            nb = [lut[tuple(ijk + d)] for d in np.vstack([np.eye(3, dtype=int), -np.eye(3, dtype=int)])]
            q64 = nodes[qi].astype(np.float64)
            far = []
            for m in nb:
                w = unit_of[m]
                if tile_of[m] != tile_of[qi] or w == unit_of[qi]:
                    continue
                gap = np.maximum(0.0, np.maximum(ub[w, :3] - q64, q64 - ub[w, 3:]))
                if float((gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2]) == float(a) * float(a):
                    far.append(m)
            if not far:
                continue
            grp = {(pos[m] // 32, (pos[m] % 8) // 4) for m in [qi] + nb if tile_of[m] == tile_of[qi]}
            if len(grp) > 3:
                continue
            if max(seed_cnt[seed_cell[qi]], max(seed_cnt[seed_cell[m]] for m in far)) > 4:
                continue
            cube = [lut[tuple(ijk + np.array(d))] for d in itertools.product(range(-2, 3), repeat=3)]
            if used[cube].any():
                continue
            used[cube] = True
            picks.append((qi, far))
        assert len(picks) >= 3, f"only {len(picks)} query nodes meet the premise"
        base_ms = base.ms.copy()
        base_perm = base.perm.copy()
    finally:
        base.close()
    first = [m for _, far in picks for m in far]
    rest = np.setdiff1d(np.arange(len(nodes)), first)
    order = np.concatenate([np.array(first, np.int64), rest])
    model = nodes[order]                                   # the far neighbours get the lowest rows
    new_row = np.empty(len(nodes), np.int64)
    new_row[order] = np.arange(len(nodes))
    d_a = float(np.float32(a) * np.float32(a))
    pm = Model(model)
    try:
        np.testing.assert_array_equal(_bits(pm.ms), _bits(nodes[base_perm]))      # same sorted coordinates: same tiles and units
        np.testing.assert_array_equal(_bits(pm.ms), _bits(base_ms))
        gu = uref.row_units(pm.perm)
        for qi, far in picks:
            q = nodes[qi:qi + 1]
            run = Run(pm, q, stats_on)
            assert float(run.dk[0]) == d_a, "premise: dk = fl32(a^2)"
            G2 = cull.gap2(q, q, run.ubox)[0]
            assert np.all(G2[gu[new_row[far]]] == float(a) * float(a))
            assert np.all(gu[new_row[far]] // uref.UNITS == gu[new_row[qi]] // uref.UNITS), "premise: the same tile"
            ri, rd = _check(pm, run, oracle_c, model)
            assert ri[0, 0] == new_row[qi] and ri[0, 1] == min(new_row[far]), "premise: the far neighbour is the answer"
            blk, wav = uref.query_waves(run.qperm)
            for m in far:
                w = gu[new_row[m]]
                assert (run.masks[blk[0], w // uref.UNITS] >> np.uint32(8 * wav[0] + w % uref.UNITS)) & np.uint32(1), "the tied unit is not kept"
        return d_a
    finally:
        pm.close()


def test_strict_tie_unit_gap_equal_to_dk(stats_on, oracle_c):
    """spacing 0.5: squares are exact, G2 == dk == 0.25 for the far neighbour's unit"""
    assert _unit_lattice_case(0.5, stats_on, oracle_c) == 0.25


def test_tie_inside_the_margin_window_of_a_unit(stats_on, oracle_c):
    """spacing a = 32769/65536: fl32(a^2) = 0.2500152587890625 < a^2 = G2, and G2 (1 - 32u) <= dk; a unit rule without the margin
    skips the unit of the tied neighbour"""
    a = 32769 / 65536
    d = _unit_lattice_case(a, stats_on, oracle_c)
    assert d == 0.2500152587890625 < a * a and a * a * (1 - 32 * U) <= d


def test_coincident_rows_across_a_unit_boundary(stats_on, oracle_c):
    """Every query coincides with three model rows (dk = 0: every unit with G2 > 1e-30 is skipped) that straddle a UNIT boundary
    inside one tile; both units have G2 = 0 and stay, and the lowest original rows win."""
    rng = np.random.default_rng(51)
    g = np.arange(32, dtype=np.float32) * np.float32(0.5)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nodes = nodes[rng.permutation(len(nodes))]
    probe = Model(nodes)
    try:
        pos = np.empty(len(nodes), np.int64)
        pos[probe.perm] = np.arange(len(nodes))
    finally:
        probe.close()
    # sorted position of a node after adding two copies of every chosen node before it: choose nodes whose triple starts at 62
    # or 63 mod 64 and not at the end of a tile (one cell per node: the order of cells is fixed)
    chosen, shift = [], 0
    for r in np.argsort(pos):
        p = pos[r] + shift
        if p % uref.UNIT in (62, 63) and p % cull.TILE < 500 and len(chosen) < 24:
            chosen.append(r)
            shift += 2
    chosen = np.array(chosen)
    Mc, N = len(chosen), len(nodes)
    assert Mc == 24
    model = np.vstack([nodes[chosen], nodes, nodes[chosen]]).astype(np.float32)     # three copies; the lowest rows first
    surf = nodes[chosen]
    pm = Model(model)
    try:
        gu = uref.row_units(pm.perm)
        for k in range(Mc):
            rows = [k, Mc + chosen[k], Mc + N + k]
            assert len({gu[r] for r in rows}) == 2 and len({gu[r] // uref.UNITS for r in rows}) == 1, \
                "premise: the coincident rows span two units of one tile"
        run = Run(pm, surf, stats_on)
        ri, rd = _check(pm, run, oracle_c, model)
        assert np.all(rd == 0) and np.array_equal(ri[:, 0], np.arange(Mc)) and np.array_equal(ri[:, 1], Mc + chosen)
        assert (run.dk == 0).sum() >= Mc // 2, "premise: most queries are seeded at dk = 0"
    finally:
        pm.close()
