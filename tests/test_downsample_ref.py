"""tests/downsample_ref.py against a brute-force triple loop (voxels, members, coordinates) on hand-made clouds whose answers are
written out here: the oracle of the GPU tests is itself held to the contract of pcreg_downsample_grid_f32."""
import math

import numpy as np
import pytest

import downsample_ref as ref

NAN, INF = float("nan"), float("inf")


def brute(pts, step):
    """the contract by loops: python floats are IEEE doubles, float32 only at the ends"""
    p = np.asarray(pts, np.float32)
    n = len(p)
    live = [all(math.isfinite(float(v)) for v in p[i]) for i in range(n)]
    rows = [i for i in range(n) if live[i]]
    label = [0] * n
    if not rows:
        return np.zeros((0, 3), np.float32), [], label
    lo = [min(p[i][d] for i in rows) for d in range(3)]                                 # float32 minima
    cell = {i: tuple(int(math.floor((float(p[i][d]) - float(lo[d])) / step)) for d in range(3)) for i in rows}
    voxels = sorted(set(cell.values()))
    out, count = [], []
    for v, c in enumerate(voxels):
        members = [i for i in rows if cell[i] == c]                                    # ascending rows
        mean = []
        for d in range(3):
            s = 0.0
            for i in members:
                s = s + float(p[i][d])
            mean.append(np.float32(s / float(len(members))))
        out.append(mean); count.append(len(members))
        for i in members:
            label[i] = v + 1
    return np.array(out, np.float32).reshape(-1, 3), count, label


def both(pts, step):
    o, c, l = ref.downsample_ref(np.asarray(pts, np.float32), step)
    bo, bc, bl = brute(pts, step)
    assert o.dtype == np.float32 and c.dtype == np.int32 and l.dtype == np.int32
    np.testing.assert_array_equal(o.view(np.uint32), bo.view(np.uint32))
    assert list(c) == bc and list(l) == bl
    return o, list(c), list(l)


def test_two_points_in_one_voxel():
    o, c, l = both([[0.0, 0.0, 0.0], [0.5, 0.25, 0.75]], 1.0)
    assert o.tolist() == [[0.25, 0.125, 0.375]] and c == [2] and l == [1, 1]


def test_a_point_on_lo_and_one_exactly_one_step_from_it():
    # row 1 is lo itself (cell 0); row 0 lies exactly one step from it along x and must fall in cell 1; row 2 just below one step
    o, c, l = both([[2.5, 7.0, 7.0], [2.0, 7.0, 7.0], [np.nextafter(np.float32(2.5), np.float32(0)), 7.0, 7.0]], 0.5)
    assert l == [2, 1, 1] and c == [2, 1]
    assert o[1].tolist() == [2.5, 7.0, 7.0]
    assert o[0, 0] == np.float32((2.0 + float(np.nextafter(np.float32(2.5), np.float32(0)))) / 2.0)


def test_voxels_come_in_lexicographic_order_column_0_first():
    pts = [[1.5, 0.0, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 1.5], [0.0, 0.0, 0.0], [1.5, 1.5, 1.5]]
    o, c, l = both(pts, 1.0)
    assert o.tolist() == [[0, 0, 0], [0, 0, 1.5], [0, 1.5, 0], [1.5, 0, 0], [1.5, 1.5, 1.5]]
    assert l == [4, 3, 2, 1, 5] and c == [1] * 5


def test_a_flat_axis():
    o, c, l = both([[0.0, 3.0, 0.0], [0.25, 3.0, 2.0], [0.75, 3.0, 0.5]], 1.0)
    assert o.tolist() == [[0.375, 3.0, 0.25], [0.25, 3.0, 2.0]] and c == [2, 1] and l == [1, 2, 1]


def test_a_nan_row_belongs_to_no_voxel_and_does_not_move_lo():
    pts = [[-100.0, NAN, 0.0], [1.0, 1.0, 1.0], [INF, 0.0, 0.0], [1.5, 1.0, 1.0], [0.0, 0.0, -INF]]
    o, c, l = both(pts, 1.0)
    assert o.tolist() == [[1.25, 1.0, 1.0]] and c == [2] and l == [0, 1, 0, 1, 0]
    o, c, l = both([[NAN, 0.0, 0.0], [0.0, INF, 0.0]], 1.0)
    assert o.shape == (0, 3) and c == [] and l == [0, 0]
    o, c, l = both(np.zeros((0, 3)), 1.0)
    assert o.shape == (0, 3) and c == [] and l == []


def test_the_sum_runs_in_row_order():
    a, b, c3 = float(2.0 ** 60), float(-(2.0 ** 60)), 1.0
    assert np.float32(a) == a and (a + b) + c3 != (c3 + b) + a                     # the two orders differ: not a vacuous case
    o, c, l = both([[a, 0.0, 0.0], [b, 0.0, 0.0], [c3, 0.0, 0.0]], 2.0 ** 62)
    assert c == [3] and o[0, 0] == np.float32(1.0 / 3.0)
    o, c, l = both([[c3, 0.0, 0.0], [b, 0.0, 0.0], [a, 0.0, 0.0]], 2.0 ** 62)
    assert c == [3] and o[0, 0] == np.float32(0.0)


def test_the_cell_limit():
    pts = np.array([[0.0, 0.0, 0.0], [float(2 ** 21) - 0.5, 0.0, 0.0]], np.float32)
    o, c, l = both(pts, 1.0)                                                        # the largest index is 2^21 - 1: fine
    assert c == [1, 1]
    pts[1, 0] = float(2 ** 21)
    with pytest.raises(ref.Refused):
        ref.downsample_ref(pts, 1.0)
    with pytest.raises(ref.Refused):
        ref.downsample_ref(np.array([[0.0, 0.0, 0.0], [3e38, 0.0, 0.0]], np.float32), 1e-300)   # the quotient overflows
