"""The host reference of one RANSAC refit (ransac_refit_ref.py) and the scenes built on it (ransac_refit_scenes.py): CPU only."""
import numpy as np
import pytest

from conftest import rigid_case
from ransac_refit_scenes import ALL_SCENES, prepare
from ransac_refit_ref import exact_sum, refit_moments, refit_moments_fractions, refit_reference, two_prod


def test_two_prod_and_exact_sum_are_exact():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, 200) * 10.0 ** rng.uniform(-6, 7, 200); b = rng.uniform(-1, 1, 200) * 10.0 ** rng.uniform(-6, 7, 200)
    p, e = two_prod(a, b)
    for x, y, pp, ee in zip(a, b, p, e):
        assert Fraction(float(x)) * Fraction(float(y)) == Fraction(float(pp)) + Fraction(float(ee))
    assert exact_sum(p, e) == sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b))
    assert exact_sum([1e30, 1.0, -1e30, 2.0 ** -60]) == 1 + Fraction(1, 2 ** 60)


@pytest.mark.parametrize("shift", [0.0, 4.2e6])
def test_reference_equals_all_fraction_evaluation_bit_for_bit(shift):
    """n = 40: H and the centroids of the split-and-fsum evaluation are the bits of the all-Fraction evaluation of
    sum (m - cm)(d - cd)^T, at ordinary coordinates and under the cancellation of a 4e6 offset."""
    p1, p2, _ = rigid_case(40, 3, noise=0.01, outlier_frac=0.0)
    p1 = p1 + shift; p2 = p2 - 0.9 * shift
    rows = np.arange(40)[::-1]
    H, cd, cm, K = refit_moments(p1, p2, rows)
    Hf, cdf, cmf, Kf = refit_moments_fractions(p1, p2, rows)
    assert K == Kf == 40
    np.testing.assert_array_equal(H, Hf)
    np.testing.assert_array_equal(cd, cdf)
    np.testing.assert_array_equal(cm, cmf)


def test_reference_agrees_with_the_oracle(oracle_c):
    p1, p2, Ttrue = rigid_case(500, 11)
    rows = np.flatnonzero(oracle_c.calcDists(Ttrue, p1, p2) < 0.05)
    assert 300 < len(rows) < 500                              # a proper subset: `rows` is honoured
    T = refit_reference(p1, p2, rows)
    assert np.abs(T - oracle_c.estimateTransform(p1[rows], p2[rows])).max() < 1e-12
    full = refit_reference(p1, p2, np.arange(500))
    assert np.abs(full - oracle_c.estimateTransform(p1, p2)).max() < 1e-12
    assert np.abs(np.hstack([p2[rows], np.ones((len(rows), 1))]) @ T - np.hstack([p1[rows], np.ones((len(rows), 1))])).max() < 0.2


def test_reference_refuses_what_it_does_not_serve():
    p1, p2, _ = rigid_case(50, 5, outlier_frac=0.0)
    with pytest.raises(AssertionError):
        refit_reference(p1, p2, np.arange(3))
    flat = p1.copy(); flat[:, 2] = 0.0
    with pytest.raises(AssertionError):
        refit_reference(flat, p2, np.arange(50))


def test_reference_does_not_depend_on_a_far_row():
    """The reference subtracts no origin: rows outside `rows` are never read, wherever they lie."""
    p1, p2, _ = rigid_case(300, 8, outlier_frac=0.0)
    rows = np.arange(1, 300)
    T = refit_reference(p1, p2, rows)
    q1 = p1.copy(); q2 = p2.copy(); q1[0] = 1e9; q2[0] = -3e8
    np.testing.assert_array_equal(refit_reference(q1, q2, rows), T)


@pytest.mark.parametrize("name,n", ALL_SCENES)
def test_scenes_are_honest(name, n, oracle_c):
    """Every scene of the GPU tests, judged with the oracle alone: the reference can decide at least 6 of its 8 hypotheses
    and the scene bites (the assertions are prepare()'s); the refined pass is as sensitive as the first."""
    s = prepare(name, n)
    for h in s["hyps"]:
        assert h["ref"]["inlrNum"][0] >= 4 and h["e_ref"] < 1e-5
