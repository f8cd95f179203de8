"""tests/knn_unit_ref.py pinned on hand-made boxes (no GPU): the unit rule of the point search, DESIGN 4.1."""
import numpy as np

import knn_cull_ref as cull
import knn_unit_ref as ref

PREP = cull.make_prep(1.0, [0.0, 0.0, 0.0])


def _rows_x(xs):
    """sorted rows on the x axis"""
    xs = np.asarray(xs, np.float32)
    return np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)


def _tile_boxes(ms):
    starts = np.arange(0, len(ms), cull.TILE)
    return np.hstack([np.minimum.reduceat(ms, starts, axis=0), np.maximum.reduceat(ms, starts, axis=0)]).astype(np.float32)


def test_unit_boxes_partial_and_empty_units():
    ms = _rows_x(np.arange(512 + 70, dtype=np.float32))              # tile 1: one full unit, one of 6 rows, six empty
    ub = ref.unit_boxes(ms)
    assert ub.shape == (16, 6)
    assert ub[0, 0] == 0 and ub[0, 3] == 63 and ub[7, 0] == 448 and ub[7, 3] == 511
    assert ub[8, 0] == 512 and ub[8, 3] == 575
    assert ub[9, 0] == 576 and ub[9, 3] == 581, "a partly filled unit's box covers its existing rows only"
    assert np.all(ub[10:, :3] == np.inf) and np.all(ub[10:, 3:] == -np.inf)
    assert ref.unit_boxes(np.zeros((0, 3), np.float32)).shape == (8, 6)


def _one_block(wave_x, wave_dk, n_per_wave=128):
    """a block whose wave v sits at x = wave_x[v] with seed distance wave_dk[v]; None: the wave's queries are not scored"""
    q, dk = [], []
    for x, d in zip(wave_x, wave_dk):
        if x is None:
            q.append(np.tile(np.array([[3e8, 0.0, 0.0]], np.float32), (n_per_wave, 1)))     # outside kQueryScaledMax
            dk.append(np.full(n_per_wave, 1.0, np.float32))
        else:
            q.append(np.tile(np.array([[x, 0.0, 0.0]], np.float32), (n_per_wave, 1)))
            dk.append(np.full(n_per_wave, d, np.float32))
    q, dk = np.vstack(q), np.concatenate(dk)
    return q, np.arange(len(q)), dk


def test_bits_bytes_and_the_three_special_cases():
    # one tile: unit s covers x in [100 s, 100 s + 63]
    ms = _rows_x(np.concatenate([100.0 * s + np.arange(64) for s in range(8)]))
    tb, ub = _tile_boxes(ms), ref.unit_boxes(ms)
    # wave 0 at x = 0 with dk 4 (reaches 2): unit 0 only.  wave 1 at x = 431.5 with dk 64 (reaches 8): units 3 (gap 68.5: no) ..
    # unit 4 covers [400, 463]: inside.  wave 2 unseeded.  wave 3 not scored.
    q, qperm, dk = _one_block([0.0, 431.5, 250.0, None], [4.0, 64.0, np.inf, 1.0])
    m = ref.unit_masks(q, qperm, dk, tb, ub, PREP)
    assert m.shape == (1, 1)
    assert m[0, 0] == (0x01 | (0x10 << 8) | (0xFF << 16) | (0x00 << 24))
    assert ref.unit_stats(q, qperm, dk, tb, ub, PREP) == (1 + 1 + 8, 32)
    assert ref.unit_masks(q, qperm, dk, tb, ub, PREP, cull_on=False)[0, 0] == 0xFFFFFFFF
    assert ref.unit_stats(q, qperm, dk, tb, ub, PREP, cull_on=False) == (32, 32)


def test_strictness_margin_and_the_tiny_gap_guard():
    ms = _rows_x(np.concatenate([100.0 * s + np.arange(64) for s in range(8)]))
    tb, ub = _tile_boxes(ms), ref.unit_boxes(ms)
    # a wave at x = 65: unit 0 ends at 63 (gap 2, G2 = 4), unit 1 starts at 100 (gap 35)
    for d, bit0 in ((4.0, True), (4.0 * (1 - 32 * cull.U), True), (np.float32(3.9999), False)):
        q, qperm, dk = _one_block([65.0], [d])
        m = ref.unit_masks(q, qperm, dk, tb, ub, PREP)
        assert bool(m[0, 0] & 1) == bit0, d
    # gaps below 1e-15 (G2 < 1e-30) are never skipped, even at dk = 0
    ms2 = _rows_x(np.concatenate([np.float32(1e-16) * s + np.zeros(64) for s in range(8)]))
    q, qperm, dk = _one_block([0.0], [0.0])
    assert ref.unit_masks(q, qperm, dk, _tile_boxes(ms2), ref.unit_boxes(ms2), PREP)[0, 0] == 0xFF


def test_empty_units_are_never_kept_by_the_test_and_ragged_last_wave():
    ms = _rows_x(np.arange(100, dtype=np.float32))                    # one tile: unit 0 full, unit 1 has 36 rows, 2..7 empty
    tb, ub = _tile_boxes(ms), ref.unit_boxes(ms)
    q, qperm, dk = _one_block([50.0, 80.0], [1e6, 1e6], n_per_wave=128)
    q, qperm, dk = q[:130], qperm[:130], dk[:130]                     # the second wave holds two queries
    m = ref.unit_masks(q, qperm, dk, tb, ub, PREP)
    assert m[0, 0] == (0x03 | (0x03 << 8)), hex(int(m[0, 0]))
    dk[129] = np.inf                                                  # ... one of them unseeded: every unit, empty ones included
    assert ref.unit_masks(q, qperm, dk, tb, ub, PREP)[0, 0] == (0x03 | (0xFF << 8))


def test_a_listed_tile_may_have_an_empty_mask():
    """Two waves far apart on x and a tile whose rows lie between them: the block's box spans the tile (listed), no wave's box
    comes near any of its units."""
    xs = np.concatenate([1000.0 + 10.0 * s + np.arange(64) * 0.1 for s in range(8)])
    ms = _rows_x(xs)
    tb, ub = _tile_boxes(ms), ref.unit_boxes(ms)
    q, qperm, dk = _one_block([0.0, 2000.0], [1.0, 1.0])
    assert cull.visited_pairs(q, qperm, dk, tb, PREP)[0, 0]
    assert ref.unit_masks(q, qperm, dk, tb, ub, PREP)[0, 0] == 0
    assert ref.unit_stats(q, qperm, dk, tb, ub, PREP) == (0, 32)


def test_the_units_never_reach_a_tile_the_block_rule_skips():
    """The unit rule alone (unit_keep, which does not look at the list) keeps nothing of a tile that the block rule skips while
    every seed distance is finite: the wave's box lies inside the block's, the unit's inside the tile's, D_wave <= D_block."""
    rng = np.random.default_rng(5)
    skipped_pairs = 0
    for trial in range(20):
        M = int(rng.integers(600, 4000))
        ms = (rng.random((M, 3)) * [2000.0, 50.0, 20.0]).astype(np.float32)
        ms = ms[np.argsort(ms[:, 0], kind="stable")]                  # tiles compact in x
        Q = int(rng.integers(300, 1500))
        q = (rng.random((Q, 3)) * [2000.0, 50.0, 20.0]).astype(np.float32)
        q = q[np.argsort(q[:, 0], kind="stable")]
        if trial % 4 == 0:
            q[rng.integers(0, Q, 5), 1] = 3e8                         # a few unscored queries
        dk = (rng.random(Q) * 30.0).astype(np.float32)
        qperm = np.arange(Q)
        tb, ub = _tile_boxes(ms), ref.unit_boxes(ms)
        listed = cull.visited_pairs(q, qperm, dk, tb, PREP)
        keep = ref.unit_keep(*ref.wave_bounds(q, qperm, dk, PREP), ub)               # [nb, 4, nt * 8]
        by_tile = keep.reshape(keep.shape[0], ref.WAVES, -1, ref.UNITS).any(axis=(1, 3))
        assert not np.any(by_tile & ~listed), "a unit kept in a tile the block skips"
        skipped_pairs += int((~listed).sum())
        masks = ref.unit_masks(q, qperm, dk, tb, ub, PREP)
        assert np.all(masks[~listed] == 0)
        assert ref.unit_stats(q, qperm, dk, tb, ub, PREP)[0] == int(keep.sum())
    assert skipped_pairs > 20, "premise: the block rule skips tiles in these trials"


def test_answers_in_visited_units_helper():
    perm = np.arange(1024)[::-1].copy()                              # sorted row r is original row 1023 - r
    qperm = np.arange(130)
    mask = np.zeros((1, 2), np.uint32)
    mask[0, 1] = 1 << 3                                               # wave 0, unit 3 of tile 1: sorted rows 704..767
    mask[0, 0] = 1 << (8 + 0)                                         # wave 1, unit 0 of tile 0: sorted rows 0..63
    idx = np.zeros((130, 2), np.int64)
    idx[:, 0] = 1023 - 704
    idx[:, 1] = 1023 - 767
    idx[128:] = [[1023 - 0, 1023 - 63]]
    ok = np.ones(130, bool)
    assert ref.answers_in_visited_units(mask, perm, qperm, idx, ok).all()
    idx[5, 1] = 1023 - 768
    got = ref.answers_in_visited_units(mask, perm, qperm, idx, ok)
    assert not got[5, 1] and got.sum() == 259
    ok[5] = False
    assert ref.answers_in_visited_units(mask, perm, qperm, idx, ok).all()
