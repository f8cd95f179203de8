"""Pins the brute-force k-nearest reference (tests/knn_k_ref.c) on hand-made cases, so that the GPU tests compare against
the contract and not against a second copy of the kernel: the fmaf chain, (distance, row) order, ties and duplicates to the
lowest row, M < k, and squared distances that overflow to +inf."""
import numpy as np

import knn_k_ref as ref


def _chain(q, m):
    q, m = np.float32(q), np.asarray(m, np.float32)
    dx, dy, dz = q[0] - m[:, 0], q[1] - m[:, 1], q[2] - m[:, 2]
    with np.errstate(over="ignore"):
        # fmaf(dz, dz, fmaf(dy, dy, dx*dx)) through float64: each fma is exact in double before the single rounding
        # (the products of two floats are exact in double and the sums here stay far from double's rounding)
        a = (dx * dx).astype(np.float32)
        b = (dy.astype(np.float64) * dy + a).astype(np.float32)
        return (dz.astype(np.float64) * dz + b).astype(np.float32)


def test_order_and_ties_go_to_the_lowest_row():
    m = np.array([[3, 0, 0], [1, 0, 0], [0, 2, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [5, 5, 5]], np.float32)
    idx, dist = ref.knn([[0, 0, 0]], m, 5)
    assert idx.tolist() == [[1, 3, 4, 5, 2]]
    assert dist.tolist() == [[1, 1, 1, 1, 4]]
    idx, dist = ref.knn([[0, 0, 0]], m, 1)
    assert idx.tolist() == [[1]] and dist.tolist() == [[1]]


def test_duplicated_rows_keep_their_row_order():
    m = np.tile(np.array([[2, 2, 2], [1, 1, 1]], np.float32), (4, 1))          # rows 1, 3, 5, 7 coincide, then 0, 2, 4, 6
    idx, dist = ref.knn([[0, 0, 0]], m, 6)
    assert idx.tolist() == [[1, 3, 5, 7, 0, 2]]
    assert dist.tolist() == [[3, 3, 3, 3, 12, 12]]


def test_fewer_rows_than_k_and_no_rows():
    m = np.array([[1, 0, 0], [0, 0, 0]], np.float32)
    idx, dist = ref.knn([[0, 0, 0], [2, 0, 0]], m, 4)
    assert idx.tolist() == [[1, 0, -1, -1], [0, 1, -1, -1]]
    assert dist[:, :2].tolist() == [[0, 1], [1, 4]] and np.all(np.isposinf(dist[:, 2:]))
    idx, dist = ref.knn([[0, 0, 0]], np.zeros((0, 3), np.float32), 3)
    assert idx.tolist() == [[-1, -1, -1]] and np.all(np.isposinf(dist))
    idx, dist = ref.knn(np.zeros((0, 3), np.float32), m, 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3)


def test_overflowing_distances_are_inf_and_ordered_by_row():
    big = np.float32(3e38)
    m = np.array([[big, 0, 0], [-big, 0, 0], [1e19, 0, 0], [0, -big, 0], [0, 0, 2e19]], np.float32)
    idx, dist = ref.knn([[-big, 0, 0]], m, 5)
    # row 1 coincides; rows 2 and 4 are at ~3e38 (squares overflow); rows 0 (dx = inf) and 3 overflow too
    assert idx[0, 0] == 1 and dist[0, 0] == 0
    assert idx[0, 1:].tolist() == [0, 2, 3, 4] and np.all(np.isposinf(dist[0, 1:]))
    idx, dist = ref.knn([[0, 0, 0]], m, 3)          # only row 2 stays finite: (2e19)^2 overflows like 3e38^2
    assert idx.tolist() == [[2, 0, 1]] and dist[0, 0] == np.float32(1e19) ** 2 and np.isposinf(dist[0, 1]) and np.isposinf(dist[0, 2])


def test_agrees_with_a_numpy_sort_on_a_random_cloud():
    rng = np.random.default_rng(5)
    m = (rng.random((3000, 3)) * 10).astype(np.float32)
    m[1500:1600] = m[100:200]                                              # duplicates far apart in row order
    q = (rng.random((200, 3)) * 10).astype(np.float32)
    q[:20] = m[110:130]
    for k in (1, 2, 7, 32):
        idx, dist = ref.knn(q, m, k, threads=3)
        for i in range(len(q)):
            d = _chain(q[i], m)
            order = np.lexsort((np.arange(len(m)), d))[:k]
            assert idx[i].tolist() == order.tolist()
            assert np.array_equal(dist[i], d[order])
