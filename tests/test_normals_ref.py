"""The normals reference (tests/normals_ref.py) on known answers, without a GPU: points exactly on a plane, a three-point
neighbourhood, both sign rules, the NaN cases -- and the share of rows every (family, k) of tests/test_gpu_normals.py excludes from
the direction comparison (relative gap below 1e-3) against the 4 % cap stated there."""
import numpy as np
import pytest

import normals_ref as ref


def _sin_angle(a, b):
    c = np.cross(a, b)
    return np.sqrt((c * c).sum(axis=-1)) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.mark.parametrize("k", [3, 6, 16])
def test_points_on_a_plane(k):
    """z = a x + b y + c with coordinates that are exact in fp32: the normal is (a, b, -1) / norm, the variation ~ 0"""
    rng = np.random.default_rng(5)
    xy = rng.integers(-64, 64, (300, 2)).astype(np.float64)
    xy = np.unique(xy, axis=0)
    a, b, c = 0.5, -0.25, 3.0
    pts = np.column_stack([xy, a * xy[:, 0] + b * xy[:, 1] + c]).astype(np.float32)
    r = ref.normals(pts, k)
    want = np.array([a, b, -1.0]) / np.sqrt(a * a + b * b + 1)
    good = r["gap"] > 1e-6                                  # (three collinear lattice points have no plane)
    assert good.mean() > 0.9 and (r["n"] == k).all()
    assert _sin_angle(r["normal"][good], want[None]).max() < 1e-9
    assert np.abs(r["variation"][good]).max() < 1e-12


def test_three_points_give_the_triangle_normal():
    tri = np.array([[1, 2, 3], [4, 2, 5], [2, 6, 4]], np.float32)
    want = np.cross(tri[1].astype(float) - tri[0], tri[2].astype(float) - tri[0])
    for k in (3, 8):                                        # k = 8: only three rows exist, n = 3
        r = ref.normals(tri, k)
        assert (r["n"] == 3).all()
        assert _sin_angle(r["normal"], want[None]).max() < 1e-12
        assert np.abs(r["variation"]).max() < 1e-15


def test_both_sign_rules():
    tri = np.array([[0, 0, 5], [4, 0, 5], [0, 4, 5]], np.float32)
    r = ref.normals(tri, 3, viewpoint=(0, 0, -100))
    np.testing.assert_allclose(ref.oriented(r, tri), [[0, 0, 1]] * 3, atol=1e-15)                       # largest component made >= 0
    np.testing.assert_allclose(ref.oriented(r, tri, (0, 0, -100)), [[0, 0, -1]] * 3, atol=1e-15)        # towards a viewpoint below
    np.testing.assert_allclose(ref.oriented(r, tri, (0, 0, 100)), [[0, 0, 1]] * 3, atol=1e-15)
    assert np.allclose(np.abs(r["toward"]), np.abs(5 + 100) / np.linalg.norm(np.array([0, 0, -100.0]) - tri, axis=1))
    assert np.allclose(r["big"], 1.0)
    # the first of equal magnitudes decides: (1, -1, 0) / sqrt 2 keeps x positive
    r2 = dict(normal=np.array([[-1.0, 1.0, 0.0]]) / np.sqrt(2))
    np.testing.assert_array_equal(np.sign(ref.oriented(r2, np.zeros((1, 3), np.float32))), [[1, -1, 0]])


def test_nan_cases():
    # fewer than three rows
    for M in (1, 2):
        r = ref.normals(np.arange(3 * M, dtype=np.float32).reshape(M, 3), 3)
        assert np.isnan(r["normal"]).all() and np.isnan(r["variation"]).all() and (r["n"] == M).all()
    assert ref.normals(np.zeros((0, 3), np.float32), 3)["normal"].shape == (0, 3)
    # coincident rows: the trace is 0
    r = ref.normals(np.tile(np.array([[1, 2, 3]], np.float32), (5, 1)), 4)
    assert np.isnan(r["normal"]).all() and (r["n"] == 4).all()
    # a NaN row and a +inf row: no normal of their own, never a neighbour
    rng = np.random.default_rng(2)
    pts = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    bad = pts.copy()
    bad[7, 1] = np.nan
    bad[20, 0] = np.inf
    r = ref.normals(bad, 5)
    assert np.isnan(r["normal"][[7, 20]]).all() and (r["n"][[7, 20]] == 0).all()
    keep = np.setdiff1d(np.arange(40), [7, 20])
    r0 = ref.normals(pts[keep], 5)
    np.testing.assert_array_equal(r["normal"][keep], r0["normal"])
    np.testing.assert_array_equal(r["variation"][keep], r0["variation"])


@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_excluded_share_of_every_case(name, k):
    r = ref.normals(ref.family(name), k)
    share = ref.excluded_share(r)
    print(f"{name} k = {k}: {100 * share:.2f} % of the rows have a relative gap below {ref.GAP_MIN}")
    assert (r["n"] == k).all() and np.isfinite(r["gap"]).all()
    assert share <= ref.EXCLUDED_CAP
