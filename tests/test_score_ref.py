"""tests/score_ref.py itself, on a case made by hand: a tie between two rows, a distance equal to r2, an empty transform and a NaN
entry.  No GPU."""
import numpy as np

import score_ref as ref


def test_the_reference_on_a_hand_made_case():
    model = np.array([[2, 0, 0], [0, 0, 0], [0, 0, 0], [10, 0, 0], [0.5, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [1, 0, 0], [7, 0, 0], [0.25, 0, 0]], np.float32)
    ident = np.eye(4)
    shift = np.eye(4); shift[3, 0] = 1.0                      # [q, 1] * T: x + 1
    empty = np.zeros((4, 4)); empty[2, 1] = -0.0
    nan = np.eye(4); nan[3, 1] = np.nan
    T = np.stack([ident, shift, empty, nan])
    tq = ref.transformed(q, T)
    assert tq.dtype == np.float32 and tq.shape == (4, 4, 3)
    np.testing.assert_array_equal(tq[0], q)
    np.testing.assert_array_equal(tq[1], q + np.float32([1, 0, 0]))
    assert np.isnan(tq[2]).all()
    assert np.isnan(tq[3][:, 1]).all() and not np.isnan(tq[3][:, [0, 2]]).any()
    idx, dist, n_close, sum_d2 = ref.score(q, model, T, 1.0)
    # identity: q0 on rows 1 and 2 (a tie: the lowest row); q1 is 1 from rows 0 (d = 1 = r2: inclusive), 1 and 2, and 0.25 from
    # row 4; q2 is 9 from row 3: none; q3 is 0.0625 from rows 1, 2 and row 4 alike (a tie over three rows)
    assert idx[0].tolist() == [1, 4, -1, 1]
    assert dist[0].tolist() == [0.0, 0.25, np.inf, 0.0625]
    # x + 1: q0 -> 1 (row 4 at 0.25), q1 -> 2 (row 0, d = 0), q2 -> 8 (row 3 at 4: none), q3 -> 1.25 (rows 0 and 4 at 0.5625: a tie)
    assert idx[1].tolist() == [4, 0, -1, 0]
    assert dist[1].tolist() == [0.25, 0.0, np.inf, 0.5625]
    assert (idx[2:] == -1).all() and np.isposinf(dist[2:]).all()
    assert n_close.tolist() == [3, 3, 0, 0] and n_close.dtype == np.int32
    assert sum_d2.tolist() == [0.3125, 0.8125, 0.0, 0.0] and sum_d2.dtype == np.float64
    # a distance equal to r2 passes, the next float below it does not
    i1, d1, n1, _ = ref.score(q[1:2], model[:1], ident[None], 1.0)
    i2, d2, n2, _ = ref.score(q[1:2], model[:1], ident[None], np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert (i1.tolist(), d1.tolist(), n1.tolist()) == ([[0]], [[1.0]], [1])
    assert (i2.tolist(), d2.tolist(), n2.tolist()) == ([[-1]], [[np.inf]], [0])
    # no model, no queries, no transforms
    i0, d0, n0, s0 = ref.score(q, model[:0], T, 1.0)
    assert (i0 == -1).all() and np.isposinf(d0).all() and n0.tolist() == [0] * 4 and s0.tolist() == [0.0] * 4
    i0, d0, n0, s0 = ref.score(q[:0], model, T, 1.0)
    assert i0.shape == (4, 0) and n0.tolist() == [0] * 4 and s0.tolist() == [0.0] * 4
    i0, d0, n0, s0 = ref.score(q, model, T[:0], 1.0)
    assert i0.shape == (0, 4) and n0.shape == (0,) and s0.shape == (0,)


def test_the_sum_is_correctly_rounded():
    """fsum, not a running sum: 2^24 + 1 + 1 + ... in float64 terms that a float32 accumulator would lose"""
    dist = np.array([[1e16, 1.0, 1.0, np.inf]], np.float32)
    idx = np.array([[0, 1, 2, -1]], np.int32)
    n, s = ref.sums(idx, dist)
    assert n.tolist() == [3] and s[0] == float(np.float32(1e16)) + 2.0
