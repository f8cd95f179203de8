"""Known answers of the plane extraction's reference (tests/planes_ref.py, the contract of pcreg_model_fit_planes_f32) on the CPU:
a lattice plane among off-plane rows, a void trial, a reference vector that rejects every trial, the stop rule, the sampler and
the exact fmaf."""
import math
from fractions import Fraction

import numpy as np

import planes_ref as R


def test_fma32_is_exact_against_rationals():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (rng.standard_normal(400) * 1e-3).astype(np.float32)
    c[:50] = -(a[:50].astype(np.float64) * b[:50].astype(np.float64)).astype(np.float32)          # cancellation
    got = R._fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)


def test_splitmix64_known_values():
    # the published test vector of splitmix64 seeded with 0: its first output is the hash of 0
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF
    assert R.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_lattice_plane_among_off_plane_rows():
    m = R.lattice_scene()
    out = R.fit_planes(m, 0.05, max_planes=1, n_trials=64, min_inliers=100, seed=3)
    assert out["n_planes"] == 1 and out["counts"][0] == 1024 and out["rmse"][0] == 0.0
    np.testing.assert_array_equal(out["planes"][0], [0.0, 0.0, 1.0, -7.0])
    assert (out["labels"][:1024] == 1).all() and not out["labels"][1024:].any()
    r = out["rounds"][0]
    assert r["best_count"] == 1024 and r["best_cost"] == 200 * R.QMAX and r["n"] == 1024
    assert r["N6"][2] == r["N6"][4] == r["N6"][5] == 0.0                   # the integer sums have exact zeros in z
    assert out["centres"][0][2] == 7.0


def test_coincident_sample_rows_are_void():
    m = R.lattice_scene()
    alive = R.finite_rows(m)
    samples = np.array([[5, 5, 5], [0, 1, 1], [0, 1, 2], [0, 1, 32], [0, 1, len(m)], [-1, 1, 32]])
    r = R.round_(m, alive, 0, 0.05, len(samples), samples=samples)
    # equal indices; collinear rows (L2 == 0); a proper triple; out of range on either side
    assert list(r["void"]) == [True, True, True, False, True, True]
    assert r["best_trial"] == 3 and r["best_count"] == 1024
    dup = m.copy()
    dup[1] = dup[0]
    dup[2] = dup[0]
    assert R.round_(dup, alive, 0, 0.05, 1, samples=np.array([[0, 1, 2]]))["void"][0]          # three coincident rows
    alive2 = alive.copy()
    alive2[32] = False
    assert R.round_(m, alive2, 0, 0.05, 1, samples=np.array([[0, 1, 32]]))["void"][0]          # a row that is not alive


def test_ref_vec_can_reject_every_trial():
    m = R.lattice_scene()[:1024]                                             # the plane alone: every proper trial has n = +-z
    out = R.fit_planes(m, 0.05, ref_vec=[1.0, 0.0, 0.0], max_angle=math.radians(30), max_planes=2, n_trials=32, seed=1)
    assert out["n_planes"] == 0 and out["best_trial"][0] == -1 and not out["labels"].any()
    ok = R.fit_planes(m, 0.05, ref_vec=[0.1, 0.0, -1.0], max_angle=math.radians(30), max_planes=1, n_trials=32, seed=1)
    assert ok["n_planes"] == 1
    np.testing.assert_array_equal(ok["planes"][0], [0.0, 0.0, -1.0, 7.0])     # signed towards the reference vector


def test_stop_rule_and_zero_tail():
    m = R.lattice_scene()
    out = R.fit_planes(m, 0.05, max_planes=4, n_trials=64, min_inliers=100, seed=3)
    assert out["n_planes"] == 1                                              # 200 scattered rows hold no plane of 100
    assert out["best_trial"][1] >= 0 and 3 <= out["best_count"][1] < 100     # the stopping round's diagnostics are recorded
    assert not out["counts"][1:].any() and not out["planes"][1:].any() and not out["best_count"][2:].any()
    none = R.fit_planes(m, 0.05, max_planes=2, n_trials=64, min_inliers=2000, seed=3)
    assert none["n_planes"] == 0 and none["best_count"][0] == 1024 and not none["labels"].any()


def test_degenerate_clouds():
    assert R.fit_planes(np.zeros((0, 3), np.float32), 0.1, max_planes=3)["n_planes"] == 0
    for M in (2, 3):
        pts = np.eye(3, dtype=np.float32)[:M] + 5
        out = R.fit_planes(pts, 0.1, max_planes=2, n_trials=64, seed=2)
        assert out["n_planes"] == (1 if M == 3 else 0)
    same = np.full((50, 3), 2.5, np.float32)
    out = R.fit_planes(same, 0.1, n_trials=16)
    assert out["n_planes"] == 0 and out["best_trial"][0] == -1 and R.exponent(same) == 0
    bad = R.lattice_scene()
    bad[7] = [np.nan, 1, 7]
    bad[9] = [3, np.inf, 7]
    out = R.fit_planes(bad, 0.05, n_trials=64, min_inliers=100, seed=3)
    assert out["counts"][0] == 1022 and out["labels"][7] == 0 and out["labels"][9] == 0


def test_scene_prototype():
    m = R.scene(1030)
    out = R.fit_planes(m, 0.08, max_planes=5, n_trials=128, min_inliers=40, seed=7)
    assert out["n_planes"] == 3
    assert 3 <= out["best_count"][3] < 40
    for r in out["rounds"][:3]:
        assert r["max_g"] <= 1 << 17
        assert (r["mu"][1] - r["mu"][0]) / r["normN"] > 0.5
