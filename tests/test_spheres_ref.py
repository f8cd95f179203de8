"""The premises of tests/test_gpu_fit_spheres.py, asserted on the CPU with the sphere extraction's reference alone
(tests/spheres_ref.py, the contract of pcreg_model_fit_spheres_f32): with the committed seed the reference finds the three spheres of
each scene and then stops; max |g| < 2^17; the tile and chunk counts the scenes are meant to have; refit_used = 1 in every fitted
round; the accuracy of finish64 against finish_exact; and the edge cases' outcomes -- the void samples, the radius bounds, the knife
edge's three verdicts, the refit that is not used."""
import functools
import math
from fractions import Fraction

import numpy as np

import spheres_ref as R

KAPPA_MAX = 8.0          # kappa_2(N) of the scenes' fitted rounds: 1.04 .. 1.18 for the full spheres, 4.2 for the hemisphere


@functools.lru_cache(maxsize=None)
def _extraction(M, B, mi):
    m = R.scene(M)
    m.setflags(write=False)
    return m, R.fit_spheres(m, R.SCENE_T, max_spheres=R.SCENE_P, n_trials=B, min_inliers=mi, seed=R.SCENE_SEED)


def test_circumsphere_of_exact_rows():
    c = np.array(R.KNIFE_C)
    q = (c + np.array([[9, 0, 0], [1, 4, 8], [-4, 4, 7], [3, -6, 6]])).astype(np.float32)
    det, u, rad = R.circumsphere(q)
    assert det != 0 and [q[0][k] + u[k] for k in range(3)] == list(R.KNIFE_C) and rad == 9.0
    assert R.circumsphere(np.array(R.COPLANAR, np.float32))[0] == 0.0


def test_scenes_three_spheres_then_stop():
    for M, B, mi in R.SCENES:
        m, out = _extraction(M, B, mi)
        assert out["n_spheres"] == 3 and 4 <= out["best_count"][3] < mi, M
        assert out["refit_used"][:3].tolist() == [1, 1, 1]
        want = np.array([0.40, 0.25, 0.15]) * M
        assert (np.abs(out["counts"][:3] - want) < 0.02 * M).all() and (out["rmse"][:3] < 0.03).all()
        for p, (c, rad) in enumerate(R.SCENE_SPHERES):                       # found in the order of their sizes, each where it was put
            got = out["spheres"][p]
            assert np.abs(got[:3] - (np.array(c) + np.array(R.SCENE_OFFSET))).max() < 0.02 and abs(got[3] - rad) < 0.01, (M, p)
        assert out["rounds"][0]["e"] == 5 and max(r["max_g"] for r in out["rounds"][:3]) < 1 << 17


def test_scene_tile_and_chunk_counts():
    (M0, _, _), (M1, _, _) = R.SCENES
    assert divmod(M0, 512) == (2, 6) and -(-M0 // 2048) == 1                  # two 512-row tiles and a 6-row tail, one scoring chunk
    assert -(-M1 // 2048) == 2 and R.finite_rows(R.scene(M1)).all()           # every row alive in round 0: two scoring chunks
    _, out = _extraction(*R.SCENES[1])
    assert [len(r["alive_rows"]) > 2048 for r in out["rounds"]] == [True, True, False, False]     # and one chunk once sphere 2 is gone


def test_finish64_against_finish_exact():
    """the relative error of a, in the 2-norm, is at most 64 eps kappa_2(N): the backward error of a 3 x 3 Cholesky solve is a few
    eps ||N|| (Higham's bound with n = 3 and its constants is below 64 eps), and a perturbation dN moves the solution by at most
    kappa_2(N) ||dN|| / ||N||"""
    worst = 0.0
    for M, B, mi in R.SCENES:
        _, out = _extraction(M, B, mi)
        for p, r in enumerate(out["rounds"][:3]):
            k = R.kappa2(r["N6"])
            ex = R.finish_exact(r["N6"], r["h"])
            err = math.sqrt(sum(float(Fraction(a) - x) ** 2 for a, x in zip(r["fit"]["a"], ex))) / math.sqrt(sum(float(x) ** 2 for x in ex))
            share = err / (64 * R.EPS * k)
            print(f"M = {M} round {p}: kappa_2(N) = {k:.3f}, relative error of a {err:.3e}, {share:.4f} of the bound")
            assert k < KAPPA_MAX and share <= 1.0
            worst = max(worst, share)
    print(f"worst share of the bound: {worst:.4f}")
    assert worst < 0.25


def test_bad_samples_are_void():
    _, plain = _extraction(*R.SCENES[0])
    m, smp = R.bad_sample_scene(plain["labels"])
    out = R.fit_spheres(m, R.SCENE_T, max_spheres=3, n_trials=256, min_inliers=40, samples=smp)
    assert out["n_spheres"] == 3
    for p, r in enumerate(out["rounds"]):
        assert r["void"][:4].all() and r["void"][4] == (p > 0), p
    assert (out["labels"][smp[1, 4]] == 1).all()


def test_radius_bounds():
    m, plain = _extraction(*R.SCENES[0])
    smp = R.sample_table(len(m), plain["labels"], 3, 256, 5)
    out = R.fit_spheres(m, R.SCENE_T, min_radius=2.5, max_radius=3.5, max_spheres=3, n_trials=256, min_inliers=40, samples=smp)
    assert out["n_spheres"] == 1 and abs(out["spheres"][0][3] - 3.0) < 0.01 and out["refit_used"][0] == 1
    none = R.fit_spheres(m, R.SCENE_T, min_radius=0.0, max_radius=0.01, max_spheres=3, n_trials=256, min_inliers=40, samples=smp)
    assert none["n_spheres"] == 0 and none["best_trial"][0] == -1 and none["rounds"][0]["void"].all()


def test_tiny_and_degenerate_clouds():
    m4 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) + 5
    out = R.fit_spheres(m4, 0.1, max_spheres=2, n_trials=32, seed=2)
    assert out["n_spheres"] == 1 and out["counts"][0] == 4 and out["best_trial"][1] == -1
    assert R.fit_spheres(m4[:3], 0.1, max_spheres=2, n_trials=32, seed=2)["n_spheres"] == 0
    co = R.fit_spheres(np.full((700, 3), 2.5, np.float32), 0.1, max_spheres=2, n_trials=64)
    assert co["n_spheres"] == 0 and co["rounds"][0]["void"].all()


def test_knife_edge_verdicts():
    """trial scoring and the final classification meet the same edge: with min_radius = max_radius = 9 the refit (whose radius the
    pairs at R + t pull above 9) is not used, so the round's sphere is the trial's own exact one"""
    m, n = R.knife_scene()
    t2, s = R.thresholds(R.KNIFE_T)
    smp = np.array([[[0, 1, n // 2, n - 1]]], np.int32)
    out = R.fit_spheres(m, R.KNIFE_T, min_radius=9.0, max_radius=9.0, n_trials=1, samples=smp)
    r = out["rounds"][0]
    assert not r["void"][0] and list(r["trial"][1]) == list(R.KNIFE_C) and r["trial"][2] == 9.0
    r2 = R.chain_r2(m[n:], r["trial"][1], r["trial"][2])
    assert (r2[:2] == t2).all() and (r2[2:4] < t2).all() and (r2[4:] > t2).all()
    assert list(R.q_of(r2[:2], s)) == [R.QMAX] * 2 and (R.q_of(r2[2:4], s) < R.QMAX).all()
    assert r["best_count"] == n + 4 and r["best_cost"] == 2 * R.QMAX + int(R.q_of(r2[2:4], s).sum()) + 2 * R.QMAX
    assert out["refit_used"][0] == 0 and list(out["spheres"][0]) == [*R.KNIFE_C, 9.0]
    assert list(out["labels"][n:]) == [1, 1, 1, 1, 0, 0] and out["counts"][0] == n + 4


def test_refit_not_used_keeps_the_trial():
    m, plain = _extraction(*R.SCENES[0])
    Rf = float(plain["rounds"][0]["trial"][2])
    out = R.fit_spheres(m, R.SCENE_T, min_radius=Rf, max_radius=Rf, n_trials=256, min_inliers=40, seed=R.SCENE_SEED)
    r = out["rounds"][0]
    assert out["n_spheres"] == 1 and r["best_trial"] == plain["best_trial"][0] and out["refit_used"][0] == 0
    assert r["fit"]["Rg2"] > 0 and np.float32(math.sqrt(r["fit"]["Rg2"]) * 2.0 ** -(17 - r["e"])) != np.float32(Rf)
    assert list(out["spheres"][0]) == [float(v) for v in r["trial"][1]] + [Rf]
