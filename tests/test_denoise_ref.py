"""tests/denoise_ref.py on known answers, and the condition tests/test_gpu_denoise.py rests on: in every (family, k, t) case no row
lies within a relative 1e-7 of the threshold, so the inlier set of a correct implementation equals the reference's exactly."""
import numpy as np
import pytest

import denoise_ref as ref


def test_lattice_has_unit_distances():
    """32 x 32 unit lattice in z = 7, k = 2: every row has two rows at distance 1; mu = 1, sd = 0; every row an inlier at any t"""
    g = np.arange(32, dtype=np.float32)
    pts = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    for t in (0.0, 1.0, 2.5):
        r = ref.denoise(pts, 2, t)
        assert (r["n"] == 3).all() and (r["mean_dist"] == 1).all()
        assert r["nf"] == 1024 and r["mu"] == 1 and r["sd"] == 0 and r["thr"] == 1 and r["dmax"] == 1
        assert np.array_equal(r["inliers"], np.arange(1024))
    r = ref.denoise(pts, 4, 1.0)
    inside = (pts[:, 0] >= 1) & (pts[:, 0] <= 30) & (pts[:, 1] >= 1) & (pts[:, 1] <= 30)
    assert (r["mean_dist"][inside] == 1).all() and (r["mean_dist"][~inside] > 1).all()


def test_a_pair_of_points():
    """two rows 5 apart: each has the other as its only neighbour, whatever k; d = 5 both ways, sd = 0, both inliers"""
    pts = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    for k in (1, 4, 31):
        r = ref.denoise(pts, k, 1.0)
        assert (r["n"] == 2).all() and (r["mean_dist"] == 5).all()
        assert r["nf"] == 2 and r["mu"] == 5 and r["sd"] == 0 and r["thr"] == 5
        assert np.array_equal(r["inliers"], [0, 1])


def test_three_collinear_rows_by_hand():
    """rows at x = 0, 1, 3 with k = 2: d = (2, 1.5, 2.5); mu = 2, sd = 0.5 (MATLAB's std divides by nf - 1)"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    r = ref.denoise(pts, 2, 1.0)
    assert np.array_equal(r["mean_dist"].astype(np.float64), [2.0, 1.5, 2.5])
    assert r["mu"] == 2 and r["sd"] == 0.5 and r["thr"] == 2.5 and r["dmax"] == 2.5
    assert np.array_equal(r["inliers"], [0, 1, 2])
    assert np.array_equal(ref.denoise(pts, 2, 0.0)["inliers"], [0, 1])
    assert np.array_equal(ref.denoise(pts, 1, 0.0)["mean_dist"].astype(np.float64), [1.0, 1.0, 2.0])


def test_a_nan_row_is_no_neighbour_and_has_none():
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [3, 0, 0], [0, np.inf, 0]], np.float32)
    r = ref.denoise(pts, 2, 1.0)
    assert np.array_equal(r["n"], [3, 3, 0, 3, 0])
    assert np.isnan(r["mean_dist"][[2, 4]]).all()
    assert np.array_equal(r["mean_dist"][[0, 1, 3]].astype(np.float64), [2.0, 1.5, 2.5])
    assert r["nf"] == 3 and r["mu"] == 2 and r["sd"] == 0.5
    assert np.array_equal(r["inliers"], [0, 1, 3])


def test_a_single_row_and_no_row():
    r = ref.denoise(np.array([[1, 2, 3]], np.float32), 4, 1.0)
    assert r["n"][0] == 1 and np.isnan(r["mean_dist"][0]) and r["nf"] == 0 and np.isnan(r["thr"]) and len(r["inliers"]) == 0
    r = ref.denoise(np.zeros((0, 3), np.float32), 4, 1.0)
    assert r["nf"] == 0 and np.isnan(r["thr"]) and len(r["inliers"]) == 0 and r["mean_dist"].shape == (0,)


def test_the_mask_restated_on_returned_doubles():
    d = np.array([1.0, np.nan, 2.0, 2.0000000000000004, 0.0])
    assert np.array_equal(ref.inliers_of(d, 2.0), [0, 2, 4])
    assert len(ref.inliers_of(d, np.nan)) == 0


def test_families_hold_real_outliers():
    for name, m in ref.families().items():
        assert m.dtype == np.float32 and m.shape == (ref.M_FAMILY, 3) and np.isfinite(m).all()
        r = ref.denoise(m, 4, 1.0)
        assert r["nf"] == ref.M_FAMILY and 0 < len(r["inliers"]) < ref.M_FAMILY, name
        assert r["dmax"] > r["thr"] * 2, name                # (a thrown row stands far above the threshold)


@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_no_row_lies_at_the_threshold(name):
    """the 48 cases: the smallest relative gap |d_i - thr| / thr is 1.36e-6 (sheet, k = 3, t = 0); double rounding at nf = 2048 is
    about 5e-13, so the GPU test excuses no row"""
    m = ref.family(name)
    worst = min((ref.denoise(m, k, t)["rel_gap"], k, t) for k in ref.KS for t in ref.TS)
    print(f"{name}: smallest relative gap {worst[0]:.3e} at k = {worst[1]}, t = {worst[2]}")
    assert worst[0] >= ref.GAP_MIN
    assert all((ref.denoise(m, k, 0.0)["n"] == k + 1).all() for k in ref.KS)
