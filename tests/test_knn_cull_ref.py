"""The host reference of the tile-culling rule (tests/knn_cull_ref.py) pinned on hand-made boxes, one edge of the rule
each: the strict '>', the 32u margin, the 1e-30 guard, an unseeded query, a block without a scored query."""
import numpy as np

import knn_cull_ref as ref

U = 2.0 ** -24
PREP = ref.make_prep(1.0, (0.0, 0.0, 0.0))


def _tile(lo, hi):
    return np.array([list(lo) + list(hi)], np.float32)


def _one(q, dk, tile_box, prep=PREP):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    return ref.visited_pairs(q, np.arange(len(q)), np.asarray(dk, np.float32), tile_box, prep)[0, 0]


def test_gap_equal_to_dk_is_kept():
    # one query at the origin, a tile whose face is 0.5 away on x: G2 = 0.25 exactly
    assert _one([0, 0, 0], [0.25], _tile((0.5, -1, -1), (1, 1, 1)))
    assert ref.gap2(np.zeros((1, 3)), np.zeros((1, 3)), _tile((0.5, -1, -1), (1, 1, 1)))[0, 0] == 0.25


def test_dk_inside_the_margin_window_is_kept():
    # G2 = a^2 (exact in float64), dk = fl32(a^2) < G2 but >= G2 (1 - 32u): kept; the same pair without a margin would go
    a = 32769 / 65536
    G2 = a * a
    dk = np.float32(G2)
    assert float(dk) < G2 and G2 * (1 - 32 * U) <= float(dk)
    assert _one([0, 0, 0], [dk], _tile((a, 0, 0), (2, 1, 1)))
    assert G2 > float(dk)                                        # what a rule without the margin would cull


def test_dk_just_below_the_window_is_culled():
    G2 = 0.25
    dk = np.nextafter(np.float32(G2 * (1 - 32 * U)), np.float32(0))
    assert not _one([0, 0, 0], [dk], _tile((0.5, 0, 0), (1, 1, 1)))
    edge = np.float32(G2 * (1 - 32 * U))                         # exactly on the window's lower end: not strictly below
    assert float(edge) == G2 * (1 - 32 * U)
    assert _one([0, 0, 0], [edge], _tile((0.5, 0, 0), (1, 1, 1)))


def test_an_unseeded_query_keeps_every_tile_of_its_block():
    tiles = np.array([[10, 10, 10, 11, 11, 11], [-50, 0, 0, -40, 1, 1], [0, 0, 0, 1, 1, 1]], np.float32)
    q = np.array([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.4, 0.4, 0.4]], np.float32)
    dk = np.array([0.01, 0.02, 0.03], np.float32)
    assert ref.visited_pairs(q, np.arange(3), dk, tiles, PREP).tolist() == [[False, False, True]]
    dk[1] = np.inf
    assert ref.visited_pairs(q, np.arange(3), dk, tiles, PREP).all()


def test_a_block_without_a_scored_query_visits_nothing():
    tiles = np.array([[0, 0, 0, 1, 1, 1], [1e6, 1e6, 1e6, 2e6, 2e6, 2e6]], np.float32)
    prep = ref.make_prep(2.0 ** -10, (0.5, 0.5, 0.5))
    far = np.array([[0.5, 0.5, 4e7], [np.nan, 0, 0], [0.5, -9e7, 0.5]], np.float32)       # sigma * offset > 16384, or NaN
    assert not ref.scored(far, prep).any()
    assert not ref.visited_pairs(far, np.arange(3), np.full(3, np.inf, np.float32), tiles, prep).any()
    # the same block with one scored query: its tile is kept, the far one culled
    q = np.vstack([far, [[0.5, 0.5, 0.5]]]).astype(np.float32)
    vis = ref.visited_pairs(q, np.arange(4), np.array([np.inf, np.inf, np.inf, 0.1], np.float32), tiles, prep)
    assert vis.tolist() == [[True, False]]


def test_a_gap_below_1e_30_is_kept():
    g = 5e-16                                                     # G2 = 2.5e-31 <= 1e-30: no bound, kept even with dk = 0
    assert _one([0, 0, 0], [0.0], _tile((g, 0, 0), (1, 1, 1)))
    assert not _one([0, 0, 0], [0.0], _tile((2e-15, 0, 0), (1, 1, 1)))


def test_blocks_follow_the_slot_order():
    # 1030 queries in three blocks (512, 512, 6), slots reversed: block 0 holds the LAST 512 queries
    rng = np.random.default_rng(0)
    Q = 1030
    q = rng.random((Q, 3)).astype(np.float32)
    q[:300] += 100.0
    qperm = np.arange(Q)[::-1].copy()
    tiles = np.array([[0, 0, 0, 1, 1, 1], [100, 100, 100, 101, 101, 101]], np.float32)
    vis = ref.visited_pairs(q, qperm, np.full(Q, 0.01, np.float32), tiles, PREP)
    assert vis.tolist() == [[True, False], [True, True], [False, True]]
    assert ref.visited_count(q, qperm, np.full(Q, 0.01, np.float32), tiles, PREP) == 4
    blk = ref.query_blocks(qperm)
    assert blk[Q - 1] == 0 and blk[0] == 2 and np.bincount(blk).tolist() == [512, 512, 6]
    assert ref.row_tiles(np.arange(1025)[::-1]).tolist()[:2] == [2, 1]


def test_no_query_is_scored_when_the_scale_leaves_fp32():
    q = np.zeros((2, 3), np.float32)
    assert ref.scored(q, ref.make_prep(2.0 ** 63, (0, 0, 0))).all()            # sigma^2 = 2^126: the smallest normal 1/sigma^2
    assert not ref.scored(q, ref.make_prep(2.0 ** 64, (0, 0, 0))).any()        # sigma^2 overflows
    assert ref.scored(q, ref.make_prep(2.0 ** -63, (0, 0, 0))).all()
    assert not ref.scored(q, ref.make_prep(2.0 ** -64, (0, 0, 0))).any()       # sigma^2 subnormal, 1/sigma^2 overflows
    tiles = np.array([[0, 0, 0, 1, 1, 1]], np.float32)
    assert not ref.visited_pairs(q, np.arange(2), np.zeros(2, np.float32), tiles, ref.make_prep(2.0 ** 64, (0, 0, 0))).any()
