"""Pins the brute-force radius-search reference (tests/range_ref.c) on hand-made cases, so that the GPU tests compare against
the contract and not against a second copy of the kernel: the inclusive float comparison at d == r2, (distance, row) order,
r2 = 0, non-finite queries, r2 = +inf with overflowing distances, empty inputs -- and an independent cross-check against the
brute-force k-nearest reference (tests/knn_k_ref.c)."""
import numpy as np
import pytest

import knn_k_ref
import range_ref as ref


def _segs(res):
    so, idx, dist = res
    return [(idx[a:b].tolist(), dist[a:b].tolist()) for a, b in zip(so[:-1], so[1:])]


def test_the_bound_is_inclusive_and_the_next_float_is_out():
    m = np.array([[3, 0, 0], [0, 4, 0], [0, 0, 5]], np.float32)
    so, idx, dist = ref.rangesearch([[0, 0, 0]], m, 16.0)
    assert so.tolist() == [0, 2] and idx.tolist() == [0, 1] and dist.tolist() == [9, 16]          # d == r2 is in
    so, idx, dist = ref.rangesearch([[0, 0, 0]], m, np.nextafter(np.float32(16), np.float32(0)))
    assert so.tolist() == [0, 1] and idx.tolist() == [0]                                           # r2 one float below d: out
    # a distance that is not a round number: 0.1^2 + 0.2^2 + 0.3^2 by the chain
    p = np.array([[0.1, 0.2, 0.3]], np.float32)
    d = np.float32(np.float64(p[0, 2]) * p[0, 2] + np.float32(np.float64(p[0, 1]) * p[0, 1] + np.float32(p[0, 0] * p[0, 0])))
    assert _segs(ref.rangesearch([[0, 0, 0]], p, d)) == [([0], [float(d)])]
    assert _segs(ref.rangesearch([[0, 0, 0]], p, np.nextafter(d, np.float32(0)))) == [([], [])]
    assert _segs(ref.rangesearch([[0, 0, 0]], p, np.nextafter(d, np.float32(1)))) == [([0], [float(d)])]


def test_equal_distances_are_ordered_by_row():
    m = np.array([[3, 0, 0], [1, 0, 0], [0, 2, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [5, 5, 5]], np.float32)
    assert _segs(ref.rangesearch([[0, 0, 0]], m, 4.0)) == [([1, 3, 4, 5, 2], [1, 1, 1, 1, 4])]
    assert _segs(ref.rangesearch([[0, 0, 0], [5, 5, 5]], m, 1.0)) == [([1, 3, 4, 5], [1, 1, 1, 1]), ([6], [0])]


def test_zero_radius_returns_the_coincident_rows_only():
    m = np.tile(np.array([[2, 2, 2], [1, 1, 1]], np.float32), (4, 1))
    assert _segs(ref.rangesearch([[1, 1, 1], [2, 2, 2], [0, 0, 0]], m, 0.0)) == [([1, 3, 5, 7], [0] * 4), ([0, 2, 4, 6], [0] * 4), ([], [])]


def test_non_finite_queries_are_empty_at_a_finite_radius():
    m = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    q = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, 0]], np.float32)
    so, idx, dist = ref.rangesearch(q, m, 1e30)
    assert so.tolist() == [0, 0, 0, 0, 2] and idx.tolist() == [0, 1]


def test_infinite_radius_returns_every_row_overflowed_distances_included():
    big = np.float32(3e38)
    m = np.array([[big, 0, 0], [-big, 0, 0], [1e19, 0, 0], [0, -big, 0], [0, 0, 2e19]], np.float32)
    so, idx, dist = ref.rangesearch([[-big, 0, 0], [0, 0, 0]], m, np.inf)
    assert so.tolist() == [0, 5, 10]
    assert idx[:5].tolist() == [1, 0, 2, 3, 4] and dist[0] == 0 and np.all(np.isposinf(dist[1:5]))
    assert idx[5:].tolist() == [2, 0, 1, 3, 4] and dist[5] == np.float32(1e19) ** 2 and np.all(np.isposinf(dist[6:]))
    so, idx, dist = ref.rangesearch([[-big, 0, 0], [0, 0, 0]], m, 3e38)                # finite: the overflowed ones are out
    assert so.tolist() == [0, 1, 2] and idx.tolist() == [1, 2]
    so, _, _ = ref.rangesearch([[np.nan, 0, 0]], m, np.inf)                            # a NaN distance never passes
    assert so.tolist() == [0, 0]


def test_empty_inputs():
    m = np.array([[1, 0, 0], [0, 0, 0]], np.float32)
    so, idx, dist = ref.rangesearch([[0, 0, 0], [1, 0, 0]], np.zeros((0, 3), np.float32), 5.0)
    assert so.tolist() == [0, 0, 0] and idx.shape == (0,) and dist.shape == (0,)
    so, idx, dist = ref.rangesearch(np.zeros((0, 3), np.float32), m, 5.0)
    assert so.tolist() == [0] and idx.shape == (0,) and dist.dtype == np.float32 and idx.dtype == np.int32 and so.dtype == np.int64


@pytest.mark.parametrize("seed, M, Q, r", [(1, 4000, 300, 1.2), (2, 20_000, 200, 0.9), (3, 500, 100, 3.0), (4, 3000, 150, 0.0)])
def test_agrees_with_the_k_nearest_reference(seed, M, Q, r):
    """Below 32 rows a result is the k = 32 list cut at r2, bit for bit; above, its first 32 rows are that list."""
    rng = np.random.default_rng(seed)
    m = (rng.random((M, 3)) * 10).astype(np.float32)
    m[::7] = m[3]                                                        # coincident rows: ties to the lowest row
    q = np.vstack([(rng.random((Q - 20, 3)) * 12 - 1).astype(np.float32), m[:20]])
    r2 = np.float32(r) ** 2
    so, idx, dist = ref.rangesearch(q, m, r2)
    ki, kd = knn_k_ref.knn(q, m, 32)
    n = np.diff(so)
    assert (n == 0).any() and (n > 0).any(), "premise: empty and non-empty segments"
    if r > 1:
        assert (n >= 32).any() and (n < 32).any(), "premise: both sides of 32"
    for i in range(len(q)):
        a, b = int(so[i]), int(so[i + 1])
        if b - a < 32:
            keep = kd[i] <= r2
            assert keep.sum() == b - a
            assert idx[a:b].tolist() == ki[i][keep].tolist()
            assert dist[a:b].view(np.uint32).tolist() == kd[i][keep].view(np.uint32).tolist()
        else:
            assert idx[a:a + 32].tolist() == ki[i].tolist()
            assert dist[a:a + 32].view(np.uint32).tolist() == kd[i].view(np.uint32).tolist()
            assert np.all(dist[a:b] <= r2) and np.all(np.diff(dist[a:b]) >= 0)
