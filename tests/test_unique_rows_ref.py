"""tests/unique_rows_ref.py, the reference every unique_rows / aggregate_matches test is held against, checked on its own: against
numpy's unique, against hand-written answers of MATLAB's [C, ia] = unique(A, 'rows') (first occurrence), with signed zeros, and
the two-step aggregation of completeExperiment.m:440-443 on a case where the second unique removes a row."""
import numpy as np

from unique_rows_ref import aggregate_ref, unique_rows_ref


def test_the_reference_equals_numpys_unique():
    rng = np.random.default_rng(0)
    for n, pool in ((1, 2), (50, 3), (500, 4), (3000, 6)):
        A = rng.integers(1, pool + 1, (n, 3)).astype(np.float64) * 0.25 - 0.625      # both signs, never a zero of either sign
        assert (A != 0).all()
        ia, nu = unique_rows_ref(A)
        C, first = np.unique(A, axis=0, return_index=True)
        assert nu == len(C)
        np.testing.assert_array_equal(ia, first)
        np.testing.assert_array_equal(A[ia], C)
    ia, nu = unique_rows_ref(np.zeros((0, 3)))
    assert nu == 0 and len(ia) == 0


def test_a_known_answer_with_repeated_rows():
    # A = [3 1 2; 1 5 5; 3 1 2; 1 5 4; 1 5 5; -2 9 9; 3 0 7];  [C, ia] = unique(A, 'rows')
    #   C = [-2 9 9; 1 5 4; 1 5 5; 3 0 7; 3 1 2],  ia = [6; 4; 2; 7; 1]   (1-based, first occurrences)
    A = np.array([[3, 1, 2], [1, 5, 5], [3, 1, 2], [1, 5, 4], [1, 5, 5], [-2, 9, 9], [3, 0, 7]], np.float64)
    ia, nu = unique_rows_ref(A)
    assert nu == 5
    np.testing.assert_array_equal(ia + 1, [6, 4, 2, 7, 1])
    np.testing.assert_array_equal(A[ia], [[-2, 9, 9], [1, 5, 4], [1, 5, 5], [3, 0, 7], [3, 1, 2]])


def test_signed_zeros_are_one_value_and_the_first_keeps_its_bits():
    A = np.array([[0.0, 1, 1], [-0.0, 1, 1], [-0.0, 0, 5], [0.0, -0.0, 5], [-1, 0, 0]], np.float64)
    ia, nu = unique_rows_ref(A)
    assert nu == 3
    np.testing.assert_array_equal(ia, [4, 2, 0])                     # [-1 0 0], [-0 0 5] (row 2 before row 3), [0 1 1] (row 0 before row 1)
    assert np.signbit(A[ia][1, 0]) and not np.signbit(A[ia][2, 0])   # C carries the representative's bits
    # infinities order as numbers
    B = np.array([[np.inf, 0, 0], [-np.inf, 0, 0], [1e308, 0, 0], [-np.inf, 0, 0]], np.float64)
    ib, nb = unique_rows_ref(B)
    assert nb == 3
    np.testing.assert_array_equal(ib, [1, 2, 0])


def test_aggregate_where_the_second_unique_removes_a_row():
    # pairs (surface point, model point): surface a twice (second copy dropped by the first unique), surfaces b and c both matched
    # to model point Y (c dropped by the second unique: b comes first after the sort by pts1)
    a, b, c, d = [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0], [0.5, 0, 0]
    X, Y, Z, W = [9.0, 9, 9], [4.0, 4, 4], [7.0, 7, 7], [8.0, 0, 0]
    pts1 = np.array([c, a, b, a, d], np.float64)
    pts2 = np.array([Y, X, Y, Z, W], np.float64)
    p1, p2, ia = aggregate_ref(pts1, pts2)
    # first unique: sorted pts1 = d(4), a(1), b(2), c(0) -> pts2 = W, X, Y, Y; second unique over that: Y (first: b), W, X
    np.testing.assert_array_equal(ia, [2, 4, 1])
    np.testing.assert_array_equal(p2, [Y, W, X])
    np.testing.assert_array_equal(p1, [b, d, a])
    assert (np.lexsort((p2[:, 2], p2[:, 1], p2[:, 0])) == np.arange(3)).all()       # sorted by the model point
