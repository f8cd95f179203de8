"""The point search's visit plan (knn_plan_kernel), the candidate kernel sized by it and the culled exact tail
(DESIGN 4.1).

Every GPU case compares idx and dist bit for bit with the plain-C oracle (or the direct-form search, "knn_exact", where
Q is large) and, where the case is about culling, the visited (query block, tile) pairs with tests/knn_cull_ref.py.  The
partition of a plan over the workgroups of a block is restated in tests/knn_plan_ref.py and checked without a GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import knn_cull_ref as ref
import knn_plan_ref as plan
from test_gpu_knn_cull import BOX, CORES, U, Model, _bits, _crop, _seed_cells, _shape, stats_on  # noqa: F401  (stats_on: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
K_FEW = 1024                     # knn_fast.hip: more unproven queries than this take the tail's tiled all-pairs form


# ---- the partition (no GPU) -----------------------------------------------------------------------------------------
def test_plan_constant_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "pcreg_amd", "csrc", "knn_mfma16.hip")).read()
    m = re.search(r"#define PCREG_PLAN_C (\d+)", src)
    assert m and int(m.group(1)) == plan.PLAN_C
    assert "(n_vis + kPlanC - 1) / kPlanC" in src and "return we < W ? we : W;" in src


@pytest.mark.parametrize("C", [1, 4, 8, 16])
def test_partition_is_disjoint_and_covers_the_plan(C):
    n_list = sorted(set(list(range(0, 70)) + [C * k + d for k in (1, 2, 5, 47, 48, 49, 80, 81) for d in (-1, 0, 1)]
                        + [255, 256, 257, 511, 512, 513, 1954, 4000]))
    for W, n_vis in itertools.product([1, 2, 5, 6, 8, 16, 48, 80], n_list):
        w_eff = plan.live_workgroups(n_vis, W, C)
        assert w_eff == (0 if n_vis == 0 else min(max(-(-n_vis // C), 1), W))
        seen = np.zeros(n_vis, np.int32)
        for w in range(W):
            p = plan.positions(n_vis, W, w, C)
            assert (len(p) > 0) == (w < w_eff), "a live workgroup without work, or a dead one with some"
            assert list(p) == sorted(p)
            for k in p:
                seen[k] += 1
        assert np.all(seen == 1), f"n_vis={n_vis} W={W} C={C}: positions not covered exactly once"
        if n_vis >= C * W:                                  # nothing culled at a full-size shape: position = tile, W_eff = W
            assert w_eff == W
        if w_eff:
            per = [len(plan.positions(n_vis, W, w, C)) for w in range(w_eff)]
            assert max(per) - min(per) <= 1
            assert max(per) <= C or w_eff == W


# ---- helpers --------------------------------------------------------------------------------------------------------
def _check(pm, surf, model, oracle_c, stats_on, nocull=False, exact=None):
    """one search: results against the oracle, visited pairs against the reference; returns what the search exported"""
    idx, dist, qperm, dk, st = pm.search(surf, nocull=nocull, debug_set=stats_on)
    nb = (len(surf) + ref.BLOCK - 1) // ref.BLOCK
    assert st[0] == 1 and st[2] == nb * pm.n_tiles
    if nocull:
        assert st[1] == st[2]
    else:
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep)
    if exact is None:
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    else:
        ri, rd = exact
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(_bits(dist), _bits(rd))
    return idx, dist, qperm, dk, st


def _block_counts(pm, surf, qperm, dk):
    return ref.visited_pairs(surf, qperm, dk, pm.tbox, pm.prep).sum(axis=1)


# ---- A. the plan and the candidate kernel ---------------------------------------------------------------------------
@gpu
def test_blocks_below_and_well_above_the_tile_target(stats_on, oracle_c):
    """Five tight clusters of 1536 queries each (whole blocks that see a handful of tiles: a few live workgroups;
    test_a_block_without_a_tile_and_blocks_with_exactly_one has the smallest plans) next to queries scattered over
    the whole model (blocks that see hundreds)."""
    rng = np.random.default_rng(101)
    model = (rng.random((300_000, 3)) * BOX).astype(np.float32)
    spots = model[rng.choice(len(model), 5, replace=False)]
    tight = np.vstack([s + rng.normal(0, 0.01, (1536, 3)) for s in spots])
    surf = np.vstack([tight, rng.random((4000, 3)) * BOX]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        n = _block_counts(pm, surf, qperm, dk)
        print("visited tiles per block:", sorted(n.tolist()))
        qb, W, nt = _shape(len(surf), len(model))
        live = [plan.live_workgroups(int(v), W) for v in n]
        assert 1 <= min(live) <= 3 and max(live) == W, "premise: blocks with a few live workgroups and blocks with all of them"
        _check(pm, surf, model, oracle_c, stats_on, nocull=True)
    finally:
        pm.close()


def _blob_model(rng):
    """48 blobs of exactly 512 rows, each inside one ordering-grid cell (cube of +-0.01 around a lattice of spacing 10):
    the sorted order keeps a blob together and every tile is one blob"""
    centres = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3) * 10.0 + 0.01
    model = np.vstack([c + rng.uniform(-0.01, 0.01, (512, 3)) for c in centres]).astype(np.float32)
    return centres, model[rng.permutation(len(model))]


@gpu
def test_a_block_without_a_tile_and_blocks_with_exactly_one(stats_on, oracle_c):
    """Blocks of 512 queries on one blob each see exactly that blob's tile; a block of 512 queries far outside
    kQueryScaledMax scores nothing, visits nothing, and the tail answers it (no seed: every tile scanned)."""
    rng = np.random.default_rng(102)
    centres, model = _blob_model(rng)
    a, b = centres[5], centres[30]
    far = rng.uniform(-1, 1, (512, 3)) * 100.0 + 3e6
    surf = np.vstack([a + rng.uniform(-0.005, 0.005, (512, 3)), b + rng.uniform(-0.005, 0.005, (512, 3)), far]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    pm = Model(model)
    try:
        assert pm.n_tiles == 48 and np.all(pm.tbox[:, 3:] - pm.tbox[:, :3] <= 0.03), "premise: one blob per tile"
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        n = _block_counts(pm, surf, qperm, dk)
        assert sorted(n.tolist()) == [0, 1, 1], f"premise: blocks with 0, 1 and 1 tiles, got {n.tolist()}"
        assert st[1] == 2 and st[3] >= 512            # (the blobs are so tight that their own queries stay unproven too)
        assert not ref.scored(surf, pm.prep)[np.all(surf > 1e6, axis=1)].any()
        _check(pm, surf, model, oracle_c, stats_on, nocull=True)
    finally:
        pm.close()


@gpu
def test_a_block_with_more_than_256_tiles_and_nocull(stats_on, oracle_c):
    """One block of 512 queries scattered over the whole model: its box rules out next to nothing of 782 tiles."""
    rng = np.random.default_rng(103)
    model = (rng.random((400_000, 3)) * BOX).astype(np.float32)
    surf = (rng.random((512, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert st[1] > 256, f"premise: more than 256 visited tiles, got {st[1]}"
        _check(pm, surf, model, oracle_c, stats_on, nocull=True)
    finally:
        pm.close()


@gpu
def test_unseeded_model_walks_every_tile(stats_on, oracle_c):
    """M < kSeedMinM: dk = +inf everywhere, the plan lists every tile and the tail (queries outside kQueryScaledMax) scans
    every tile."""
    rng = np.random.default_rng(104)
    model = (rng.random((9000, 3)) * BOX).astype(np.float32)
    far = (rng.uniform(-1, 1, (40, 3)) * 50.0 + [4e6, -2e6, 3e6])
    surf = np.vstack([rng.random((1500, 3)) * BOX, far]).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert np.all(dk == np.inf)
        n = _block_counts(pm, surf, qperm, dk)
        assert st[1] == n.sum() and set(n.tolist()) <= {0, pm.n_tiles} and st[3] >= 40
    finally:
        pm.close()


# ---- B. unproven queries: the culled tail ---------------------------------------------------------------------------
@gpu
def test_unscored_queries_with_a_seed_distance_reach_the_culled_tail(stats_on, oracle_c):
    """Queries pushed outside kQueryScaledMax along one axis still find seeds in the grid's border cells: the tail culls
    with a huge but finite dk."""
    rng = np.random.default_rng(105)
    model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
    crop = _crop(model, 3000, BOX * 0.3, 13)
    huge = crop[:200].copy()
    huge[:, 1] = np.float32(-7e8)
    mid = crop[200:260].copy()
    mid[:, 0] += np.float32(40000.0)
    surf = np.vstack([crop, huge, mid]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        un = ~ref.scored(surf, pm.prep)
        assert 260 <= un.sum() and un.sum() <= st[3] <= K_FEW
        assert np.isfinite(dk[un]).sum() >= 100, "premise: unscored queries with a finite seed distance"
    finally:
        pm.close()


@gpu
def test_sub_2_pow_minus_58_model_goes_to_the_tail_whole(stats_on, oracle_c):
    """sigma^2 overflows fp32: no query is scored, all 600 (<= kFew) are answered by the tail; no gap reaches 1e-30."""
    s = np.float32(2.0 ** -62)
    g = np.arange(28, dtype=np.float32) * s
    model = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(106)
    model = model[rng.permutation(len(model))]
    base = model[rng.choice(len(model), 600, replace=False)]
    surf = np.vstack([base[:300], base[300:] + rng.integers(-1, 2, (300, 3)).astype(np.float32) * (s / 2)]).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert st[1] == 0 and st[3] == len(surf)
    finally:
        pm.close()


@gpu
def test_tail_ranks_coincident_rows_across_two_tiles_by_original_row(stats_on, oracle_c):
    """Each query coincides with 151 model rows that straddle a tile boundary: more tied groups than a list holds, so the
    certificate fails and the tail decides, seeded at dk = 0 (both tiles have G2 = 0 and stay).  The two lowest ORIGINAL
    rows must win whichever side of the boundary the sort put them."""
    rng = np.random.default_rng(107)
    g = np.arange(32, dtype=np.float32) * np.float32(0.5)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nodes = nodes[rng.permutation(len(nodes))]
    probe = Model(nodes)
    try:
        pos = np.empty(len(nodes), np.int64)
        pos[probe.perm] = np.arange(len(nodes))
    finally:
        probe.close()
    extra = 150
    chosen, shift = [], 0
    for r in np.argsort(pos):                              # one cell per node: the order of the cells is fixed
        if 400 <= (pos[r] + shift) % ref.TILE <= 500 and len(chosen) < 8:
            chosen.append(r)
            shift += extra
    chosen = np.array(chosen)
    Mc, N = len(chosen), len(nodes)
    assert Mc == 8
    model = np.vstack([nodes[chosen], nodes, np.repeat(nodes[chosen], extra - 1, axis=0)]).astype(np.float32)
    surf = nodes[chosen]
    pm = Model(model)
    try:
        tiles = ref.row_tiles(pm.perm)
        for k in range(Mc):
            same = np.flatnonzero(np.all(model == surf[k], axis=1))
            assert len(same) == extra + 1 and len(set(tiles[same])) == 2, "premise: the coincident rows span two tiles"
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert st[3] == Mc, f"premise: every query is unproven, got {st[3]} of {Mc}"
        assert (dk == 0).sum() >= Mc // 2, "premise: most queries are seeded at dk = 0"
        assert np.all(dist == 0) and np.array_equal(idx[:, 0], np.arange(Mc)) and np.array_equal(idx[:, 1], Mc + chosen)
    finally:
        pm.close()


@gpu
def test_more_than_kfew_unproven_queries_take_the_many_form(stats_on, oracle_c):
    rng = np.random.default_rng(108)
    model = (rng.random((100_000, 3)) * BOX).astype(np.float32)
    far = rng.uniform(-1, 1, (1500, 3)) * 200.0 + [0.0, 5e6, 0.0]
    surf = np.vstack([_crop(model, 2000, BOX * 0.6, 14), far]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert st[3] > K_FEW
    finally:
        pm.close()


def _tail_lattice_case(a, stats_on, oracle_c, n=32):
    """test_gpu_knn_cull.py's lattice case turned towards the tail.  An n^3 lattice of spacing a, one node per ordering cell,
    so the sorted order is fixed.  The query sits on a node q; a +-axis neighbour m lies in another tile T whose box is
    exactly a away from q on that axis only (G2 = a^2 in float64 with the point box [q, q]); dk = fl32(a^2).  Here q and
    its six neighbours are spread over five of the 16-row groups a lane scores together, so the fourth best
    group of the query's list is itself within a^2, the certificate cannot hold and the tail answers.  m has the lowest
    original row of the model: it is the second answer, and only the rule's margin keeps T."""
    g = np.arange(n, dtype=np.float32) * np.float32(a)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    base = Model(nodes)
    try:
        tile_of = ref.row_tiles(base.perm)
        pos = np.empty(len(nodes), np.int64)
        pos[base.perm] = np.arange(len(nodes))
        seed_cell = _seed_cells(nodes, base.prep)
        seed_cnt = np.bincount(seed_cell[seed_cell >= 0])
        tb = base.tbox.astype(np.float64)
        lut = {tuple(np.round(p / np.float32(a)).astype(int)): i for i, p in enumerate(nodes)}
        d_a = float(np.float32(a) * np.float32(a))
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
                t = tile_of[m]
                if t == tile_of[qi]:
                    continue
                gap = np.maximum(0.0, np.maximum(tb[t, :3] - q64, q64 - tb[t, 3:]))
                if float((gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2]) == float(a) * float(a):
                    far.append(m)
            if not far:
                continue
            grp = {(pos[m] // 32, (pos[m] % 8) // 4) for m in [qi] + nb}
            if len(grp) < 5:
                continue
            if max(seed_cnt[seed_cell[qi]], max(seed_cnt[seed_cell[m]] for m in far)) > 4:
                continue                                   # every point of those seeding cells is seeded
            cube = [lut[tuple(ijk + np.array(d))] for d in itertools.product(range(-2, 3), repeat=3)]
            if used[cube].any():
                continue
            used[cube] = True
            picks.append((qi, far))
        assert len(picks) >= 3, f"only {len(picks)} query nodes meet the premise"
    finally:
        base.close()
    first = [m for _, far in picks for m in far]
    rest = np.setdiff1d(np.arange(len(nodes)), first)
    order = np.concatenate([np.array(first, np.int64), rest])
    model = nodes[order]                                   # the far neighbours get the lowest rows
    new_row = np.empty(len(nodes), np.int64)
    new_row[order] = np.arange(len(nodes))
    pm = Model(model)
    try:
        np.testing.assert_array_equal(_bits(pm.ms), _bits(nodes[base.perm]))      # same sorted coordinates: same tiles
        for qi, far in picks:
            q = nodes[qi:qi + 1]
            idx, dist, qperm, dk, st = _check(pm, q, model, oracle_c, stats_on)
            assert float(dk[0]) == d_a, "premise: dk = fl32(a^2)"
            assert st[3] == 1, "premise: the query is unproven and the tail answers it"
            G2 = ref.gap2(q, q, pm.tbox)[0]
            t_far = ref.row_tiles(pm.perm)[new_row[far]]
            assert np.all(G2[t_far] == float(a) * float(a))
            assert idx[0, 0] == new_row[qi] and idx[0, 1] == min(new_row[far]), "premise: the far neighbour is the answer"
        return d_a
    finally:
        pm.close()


@gpu
def test_tail_tie_inside_the_margin_window(stats_on, oracle_c):
    """spacing a = 32769/65536: fl32(a^2) = dk < a^2 = G2 and G2 (1 - 32u) <= dk: a point-form rule without the margin
    culls the tile of the tied neighbour, which holds the second answer"""
    a = 32769 / 65536
    d = _tail_lattice_case(a, stats_on, oracle_c)
    assert d == 0.2500152587890625 < a * a and a * a * (1 - 32 * U) <= d


@gpu
def test_tail_strict_tie_gap_equal_to_dk(stats_on, oracle_c):
    assert _tail_lattice_case(0.5, stats_on, oracle_c) == 0.25
