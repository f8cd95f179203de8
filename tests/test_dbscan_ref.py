"""The DBSCAN reference (tests/dbscan_ref.py) against scikit-learn's sequential DBSCAN, and its grid variant against its brute
force.  The clouds are integer lattices in [0, 12)^3 with many coincident rows, so every squared distance is exact in float32 and
in float64 and both sides decide the same pairs; what is compared is the rule: core rows, the numbering, and which cluster a border
row between two clusters goes to."""
import numpy as np
import pytest

import dbscan_ref as ref

EPS = (1.0, 1.5, 2.0, 3.0)


def family():
    """(cloud, eps, minpts) x 220: M up to 300, eps in EPS, minpts 1 .. 11"""
    rng = np.random.default_rng(2031)
    out = []
    for k in range(220):
        M = int(rng.integers(1, 301))
        out.append((ref.lattice_cloud(1000 + k, M), EPS[k % 4], 1 + (k // 4) % 11))
    return out


def test_the_fixtures_show_border_rows_noise_and_several_clusters():
    """a condition on the fixtures, by the reference alone"""
    border = noise = multi = 0
    for pts, eps, minpts in family():
        r = ref.dbscan(pts, np.float32(eps) ** 2, minpts)
        border += int(r["border"].sum()); noise += int(r["noise"].sum()); multi += int(r["n_clusters"] >= 2)
    print(f"{border} border rows, {noise} noise rows, {multi} clouds with two or more clusters")
    assert border >= 100 and noise >= 100 and multi >= 50, (border, noise, multi)


def test_the_reference_equals_scikit_learn():
    sk = pytest.importorskip("sklearn.cluster")
    for pts, eps, minpts in family():
        r = ref.dbscan(pts, np.float32(eps) ** 2, minpts)
        est = sk.DBSCAN(eps=eps, min_samples=minpts, algorithm="brute").fit(pts.astype(np.float64))
        np.testing.assert_array_equal(r["label"], est.labels_, err_msg=f"M = {len(pts)}, eps = {eps}, minpts = {minpts}")
        np.testing.assert_array_equal(np.flatnonzero(r["core"]), est.core_sample_indices_)


def test_the_grid_variant_equals_the_brute_force():
    for k, (pts, eps, minpts) in enumerate(family()[::7]):
        a, b = ref.dbscan(pts, np.float32(eps) ** 2, minpts), ref.dbscan(pts, np.float32(eps) ** 2, minpts, grid=True)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    rng = np.random.default_rng(8)
    pts = (rng.random((3000, 3)) * [30.0, 20.0, 10.0]).astype(np.float32)
    pts[rng.choice(3000, 9, replace=False)] = [np.nan, np.inf, 1.0]
    for r, minpts in ((0.9, 3), (1.4, 6)):
        a, b = ref.dbscan(pts, np.float32(r) ** 2, minpts), ref.dbscan(pts, np.float32(r) ** 2, minpts, grid=True)
        assert a["border"].any() and a["noise"].any() and a["n_clusters"] > 1
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_the_one_rounding_sum_is_the_float32_fma():
    """_fmaf_sq against exact rational arithmetic, the addends up to 2^60 apart"""
    from fractions import Fraction
    rng = np.random.default_rng(4)
    a = (rng.random(4000) * 2.0 ** rng.integers(-20, 20, 4000)).astype(np.float32)
    c = (rng.random(4000) * 2.0 ** rng.integers(-40, 40, 4000)).astype(np.float32)
    got = ref._fmaf_sq(a, c)
    for x, y, g in zip(a, c, got):
        exact = Fraction(float(x)) ** 2 + Fraction(float(y))
        lo = np.float32(float(exact))                          # float(Fraction) rounds once to float64; decide by neighbours instead
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert g == best, (x, y, g, best)
