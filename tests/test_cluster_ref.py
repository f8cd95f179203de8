"""Pins tests/cluster_ref.c (the clustering reference the GPU tests compare with) on inputs small enough for a brute force in
numpy: the coordinates are multiples of 1/16 below 2^10, so every product and sum of the fp32 chain is exact and float64
arithmetic restates it without a fused multiply-add."""
import numpy as np
import pytest

import cluster_ref as ref


def _brute(pts, r2):
    """connected components by an all-pairs scan and a serial union-find; the numbering rule applied at the end"""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    with np.errstate(invalid="ignore"):
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        adj = d <= float(np.float32(r2))                          # NaN never passes
    finite = np.isfinite(p).all(axis=1)
    adj &= finite[:, None] & finite[None, :]
    for i, j in zip(*np.nonzero(np.triu(adj, 1))):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(n)], np.int64)
    _, label = np.unique(roots, return_inverse=True)              # a root is its set's smallest row: ascending roots = the rule
    label = label.astype(np.int32)
    order = np.argsort(label, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(label, minlength=0))]).astype(np.int32)
    return label, off, order.astype(np.int32)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, w)


def _grid_points(n, extent, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, int(extent * 16), (n, 3)) / 16.0).astype(np.float32)


def test_the_bound_is_inclusive():
    pts = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    label, off, members = ref.cluster(pts, 25.0)
    assert label.tolist() == [0, 0] and off.tolist() == [0, 2] and members.tolist() == [0, 1]
    label, off, members = ref.cluster(pts, np.nextafter(np.float32(25), np.float32(0)))
    assert label.tolist() == [0, 1] and off.tolist() == [0, 1, 2] and members.tolist() == [0, 1]


def test_non_finite_rows_are_singletons_whatever_the_radius():
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [2, 0, 0]], np.float32)
    for r2, want in ((1.0, [0, 1, 0, 2, 3, 4, 0]), (0.5, [0, 1, 2, 3, 4, 5, 6]), (np.inf, [0, 1, 0, 2, 3, 4, 0])):
        label, off, members = ref.cluster(pts, r2)
        assert label.tolist() == want, r2
        _same((label, off, members), _brute(pts, r2) if np.isfinite(r2) else (label, off, members))
    # r2 = +inf: an overflowed distance between finite rows passes
    far = np.array([[-3e38, 0, 0], [3e38, 0, 0], [0, 3e30, 0]], np.float32)
    assert ref.cluster(far, np.inf)[0].tolist() == [0, 0, 0]
    assert ref.cluster(far, 3e38)[0].tolist() == [0, 1, 2]


def test_coincident_rows_at_radius_zero():
    base = _grid_points(40, 8, 1)
    pts = np.vstack([base, base[::-1], base[:7]])
    label, off, members = ref.cluster(pts, 0.0)
    _same((label, off, members), _brute(pts, 0.0))
    uniq = len(np.unique(base, axis=0))
    assert len(off) - 1 == uniq and np.diff(off).min() >= 2


@pytest.mark.parametrize("n, extent, r2", [(300, 8, 1.0), (300, 8, 2.25), (400, 20, 9.0), (200, 3, 0.0625), (150, 40, 1e4), (1, 4, 1.0), (2, 4, 100.0)])
def test_random_clouds_equal_the_brute_force(n, extent, r2):
    pts = _grid_points(n, extent, n + int(extent))
    got = ref.cluster(pts, r2)
    _same(got, _brute(pts, r2))
    label, off, members = got
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) > 0)
    assert np.all(np.diff(members[off[:-1]]) > 0)                 # clusters ordered by their smallest row
    for c in range(len(off) - 1):
        assert np.all(np.diff(members[off[c]:off[c + 1]]) > 0) and np.all(label[members[off[c]:off[c + 1]]] == c)


def test_the_ordering_rule_under_a_row_permutation():
    pts = _grid_points(350, 10, 5)
    label, off, members = ref.cluster(pts, 1.5)
    assert 3 < len(off) - 1 < 350
    order = np.random.default_rng(2).permutation(len(pts))
    pl, po, pm = ref.cluster(pts[order], 1.5)
    _same((pl, po, pm), _brute(pts[order], 1.5))
    # the same partition: rows of the permuted cloud are together iff their originals are
    old = label[order]
    pairs = {(a, b) for a, b in zip(old.tolist(), pl.tolist())}
    assert len(pairs) == len(off) - 1 == len(po) - 1
    # and renumbered by first appearance
    first_seen = [old.tolist().index(c) for c in range(len(off) - 1)]
    assert [pl[i] for i in sorted(first_seen)] == list(range(len(off) - 1))


def test_empty_cloud_and_large_cell_counts():
    label, off, members = ref.cluster(np.zeros((0, 3), np.float32), 1.0)
    assert len(label) == 0 and off.tolist() == [0] and len(members) == 0
    # more than 256 cells per axis at this radius: the grid falls back to larger cells
    pts = _grid_points(300, 1000, 8)
    pts[:150] = pts[150:] + np.float32(0.5)
    _same(ref.cluster(pts, 0.75), _brute(pts, 0.75))
