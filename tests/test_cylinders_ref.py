"""The premises of tests/test_gpu_fit_cylinders.py, asserted on the CPU with the cylinder extraction's reference alone
(tests/cylinders_ref.py, the contract of pcreg_model_fit_cylinders_f32): with the committed seed the reference finds exactly the two
cylinders of each scene and then stops; refit_used = 1 in both fitted rounds; max |gn|, max |g| and every sum within its stated
bound; the tile and chunk counts the scenes are meant to have; the accuracy of finish64 against finish_exact and kappa_2(N) of the
half turn; and the edge cases' outcomes -- a normal's sign, the void samples, the radius bounds, the angle rule, the knife edge's
three verdicts, the refit that is not used."""
import functools
import math
from fractions import Fraction

import numpy as np

import cylinders_ref as R

KAPPA_MAX = 16.0         # kappa_2(N) of the scenes' fitted rounds: 1.23 and 1.29 for the full turn, 5.14 and 5.60 for the half turn (printed below)


@functools.lru_cache(maxsize=None)
def _extraction(M, B, mi):
    m, nrm, kind = R.scene(M)
    for a in (m, nrm, kind):
        a.setflags(write=False)
    return m, nrm, kind, R.fit_cylinders(m, nrm, R.SCENE_T, max_radius=R.SCENE_RMAX, max_cylinders=R.SCENE_P, n_trials=B, min_inliers=mi,
                                         seed=R.SCENE_SEED)


def _which(cyl):
    """the scene's cylinder (0 or 1) a fitted one is, by its radius"""
    return 0 if abs(cyl[6] - 3.0) < abs(cyl[6] - 1.5) else 1


def test_trial_cylinder_of_exact_rows_and_the_sign_of_a_normal():
    m, nrm, n = R.knife_scene()
    i, j = R.KNIFE_SAMPLE
    ok, a, w, rad = R.trial_cylinder(m[i], m[j], nrm[i], nrm[j])
    assert ok and a == [*R.KNIFE_C, float(m[i, 2])] and [abs(v) for v in w] == [0.0, 0.0, 1.0] and w[2] == 1.0 and rad == 5.0
    for s0, s1 in ((-1, 1), (1, -1), (-1, -1)):                              # negation is exact: no bit of the trial changes
        assert R.trial_cylinder(m[i], m[j], s0 * nrm[i], s1 * nrm[j]) == (ok, a, w, rad)
    mm, nn, _ = R.scene(1030)
    for i, j in ((3, 500), (17, 18), (1000, 2)):
        want = R.trial_cylinder(mm[i], mm[j], nn[i], nn[j])
        for s0, s1 in ((-1, 1), (1, -1), (-1, -1)):
            assert R.trial_cylinder(mm[i], mm[j], s0 * nn[i], s1 * nn[j]) == want
    assert R.trial_cylinder(m[0], m[1], nrm[0], nrm[0])[0] is False          # parallel normals: L2 == 0
    assert R.axis_sums(nn[:300])[0] == R.axis_sums(-nn[:300])[0]


def test_scenes_two_cylinders_then_stop():
    for M, B, mi in R.SCENES:
        m, nrm, kind, out = _extraction(M, B, mi)
        assert out["n_cylinders"] == 2 and 4 <= out["best_count"][2] < mi, M
        assert out["refit_used"][:2].tolist() == [1, 1]
        assert sorted(_which(c) for c in out["cylinders"][:2]) == [0, 1]
        for p in range(2):
            got = out["cylinders"][p]
            c, w, rad, L, _ = R.SCENE_CYLINDERS[_which(got)]
            w = np.array(w) / np.linalg.norm(w)
            d = got[:3] - (np.array(c) + np.array(R.SCENE_OFFSET))
            print(f"M = {M} round {p}: radius {got[6]:.4f}, count {out['counts'][p]}, best count {out['best_count'][p]}, rmse {out['rmse'][p]:.4f}")
            assert abs(got[6] - rad) < 0.05 and abs(abs(got[3:6] @ w) - 1.0) < 1e-3 and np.linalg.norm(d - (d @ w) * w) < 0.05, (M, p)
            assert out["extents"][p, 1] - out["extents"][p, 0] > L - 0.5        # (the clutter's rows near the surface extend it)
            share = (0.40, 0.25)[_which(got)]
            assert abs(out["counts"][p] - share * M) < 0.03 * M and out["rmse"][p] < 0.04
        for r in out["rounds"][:2]:                                           # the stated bounds of the quantised values and the sums
            assert r["e"] == 5 and r["max_gn"] <= 1 << 17 and r["max_g"] < 1 << 17 and r["max_xy"] < 1 << 18
            assert all(abs(v) < 1 << 60 for v in r["asums"]) and all(abs(v) < 1 << 62 for v in r["csums"])
            assert r["asums"][0] == r["csums"][0]                             # every inlier's normal is usable here


def test_scene_tile_and_chunk_counts():
    (M0, _, _), (M1, _, _) = R.SCENES
    assert divmod(M0, 512) == (2, 6) and -(-M0 // 2048) == 1                  # two 512-row tiles and a 6-row tail, one scoring chunk
    assert -(-M1 // 2048) == 2 and R.finite_rows(R.scene(M1)[0]).all()        # every row alive in round 0: two scoring chunks
    *_, out = _extraction(*R.SCENES[1])
    assert [len(r["alive_rows"]) > 2048 for r in out["rounds"]] == [True, True, False]       # and one chunk once both are gone


def test_finish64_against_finish_exact():
    """the relative error of a, in the 2-norm, is at most 64 eps kappa_2(N): the backward error of a Cholesky solve is a few eps
    ||N|| (Higham's bound with n = 2 and its constants is below 64 eps), and a perturbation dN moves the solution by at most
    kappa_2(N) ||dN|| / ||N||"""
    worst = 0.0
    for M, B, mi in R.SCENES:
        *_, out = _extraction(M, B, mi)
        for p, r in enumerate(out["rounds"][:2]):
            N3, h = r["fit"]["circle"][:2]
            k = R.kappa2(N3)
            ex = R.finish_exact(N3, h)
            err = math.sqrt(sum(float(Fraction(a) - x) ** 2 for a, x in zip(r["fit"]["a"], ex))) / math.sqrt(sum(float(x) ** 2 for x in ex))
            share = err / (64 * R.EPS * k)
            print(f"M = {M} round {p} (radius {out['cylinders'][p, 6]:.2f}): kappa_2(N) = {k:.3f}, relative error of a {err:.3e}, "
                  f"{share:.4f} of the bound")
            assert k < KAPPA_MAX and share <= 1.0
            worst = max(worst, share)
    print(f"worst share of the bound: {worst:.4f}")
    assert worst < 0.25


def test_bad_samples_are_void():
    m, nrm, smp, kind = R.bad_sample_scene()
    out = R.fit_cylinders(m, nrm, R.SCENE_T, max_radius=R.SCENE_RMAX, max_cylinders=3, n_trials=256, min_inliers=60, samples=smp)
    assert out["n_cylinders"] == 2
    for p, r in enumerate(out["rounds"]):
        assert r["void"][:6].all() and r["void"][6] == (p > 0), p
    assert (out["labels"][smp[1, 6]] == 1).all()


def test_radius_bounds_and_the_angle_rule():
    m, nrm, kind, plain = _extraction(*R.SCENES[0])
    smp = R.sample_table(len(m), kind, 3, 256, 5)
    out = R.fit_cylinders(m, nrm, R.SCENE_T, min_radius=1.0, max_radius=2.0, max_cylinders=3, n_trials=256, min_inliers=60, samples=smp)
    assert out["n_cylinders"] >= 1 and abs(out["cylinders"][0][6] - 1.5) < 0.05 and out["refit_used"][0] == 1
    assert all(abs(c[6] - 3.0) > 0.5 for c in out["cylinders"][:out["n_cylinders"]])
    none = R.fit_cylinders(m, nrm, R.SCENE_T, min_radius=0.0, max_radius=0.01, max_cylinders=3, n_trials=256, min_inliers=60, samples=smp)
    assert none["n_cylinders"] == 0 and none["best_trial"][0] == -1 and none["rounds"][0]["void"].all()
    M, B, mi = R.SCENES[0]
    rv = tuple(-v for v in R.SCENE_CYLINDERS[0][1])
    ang = R.fit_cylinders(m, nrm, R.SCENE_T, max_radius=R.SCENE_RMAX, ref_vec=rv, max_angle=math.radians(10.0), max_cylinders=3, n_trials=B,
                          min_inliers=mi, seed=R.SCENE_SEED)
    assert ang["n_cylinders"] == 1 and abs(ang["cylinders"][0][6] - 3.0) < 0.05 and ang["cylinders"][0][5] < 0
    assert plain["cylinders"][[_which(c) for c in plain["cylinders"][:2]].index(0)][5] > 0     # the largest-component rule's sign


def test_tiny_and_degenerate_clouds():
    m2 = np.array([[0, 0, 0], [1, 1, 0]], np.float32) + 5
    n2 = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    out = R.fit_cylinders(m2, n2, 0.1, max_cylinders=2, n_trials=32, seed=2)
    assert out["n_cylinders"] == 0 and out["best_trial"][0] == -1 and not out["rounds"][0]["void"].all()
    assert R.fit_cylinders(m2[:1], n2[:1], 0.1, max_cylinders=2, n_trials=32, seed=2)["rounds"][0]["void"].all()
    m = np.full((700, 3), 2.5, np.float32)
    nrm = np.random.default_rng(3).normal(size=(700, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    co = R.fit_cylinders(m, nrm, 0.1, max_cylinders=2, n_trials=64)
    assert co["n_cylinders"] == 1 and co["counts"][0] == 700 and co["refit_used"][0] == 0 and co["cylinders"][0][6] == 0.0
    assert R.fit_cylinders(m, nrm, 0.1, min_radius=0.5, max_cylinders=2, n_trials=64)["rounds"][0]["void"].all()
    eq = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (1030, 1))
    assert R.fit_cylinders(R.scene(1030)[0], eq, R.SCENE_T, max_cylinders=2, n_trials=64, seed=1)["rounds"][0]["void"].all()


def test_knife_edge_verdicts():
    """trial scoring and the final classification meet the same edge: with min_radius = max_radius = 5 the refit (whose radius the
    pairs at R + t pull above 5) is not used, so the round's cylinder is the trial's own exact one"""
    m, nrm, n = R.knife_scene()
    t2, s = R.thresholds(R.KNIFE_T)
    smp = np.array([[list(R.KNIFE_SAMPLE)]], np.int32)
    out = R.fit_cylinders(m, nrm, R.KNIFE_T, min_radius=5.0, max_radius=5.0, n_trials=1, samples=smp)
    r = out["rounds"][0]
    z0 = float(m[R.KNIFE_SAMPLE[0], 2])
    p0, af, wf, Rf = r["trial"]
    assert not r["void"][0] and list(af) == [*R.KNIFE_C, z0] and list(wf) == [0.0, 0.0, 1.0] and Rf == 5.0
    r2 = R.chain_r2(m[n:], af, wf, Rf)
    assert (r2[:2] == t2).all() and (r2[2:4] < t2).all() and (r2[4:] > t2).all()
    assert list(R.q_of(r2[:2], s)) == [R.QMAX] * 2 and (R.q_of(r2[2:4], s) < R.QMAX).all()
    assert r["best_count"] == n + 4 and r["best_cost"] == 2 * R.QMAX + int(R.q_of(r2[2:4], s).sum()) + 2 * R.QMAX
    assert r["fit"]["basis_ok"] and r["fit"]["w"] == [0.0, 0.0, 1.0] and r["fit"]["Rg2"] > 0
    assert out["refit_used"][0] == 0 and list(out["cylinders"][0]) == [*R.KNIFE_C, z0, 0.0, 0.0, 1.0, 5.0]
    assert list(out["labels"][n:]) == [1, 1, 1, 1, 0, 0] and out["counts"][0] == n + 4
    free = R.fit_cylinders(m, nrm, R.KNIFE_T, n_trials=1, samples=smp)
    assert free["refit_used"][0] == 1 and free["cylinders"][0][6] > 5.0 and list(free["cylinders"][0][3:6]) == [0.0, 0.0, 1.0]


def test_refit_not_used_keeps_the_trial():
    m, nrm, kind, plain = _extraction(*R.SCENES[0])
    Rf = float(plain["rounds"][0]["trial"][3])
    out = R.fit_cylinders(m, nrm, R.SCENE_T, min_radius=Rf, max_radius=Rf, n_trials=256, min_inliers=60, seed=R.SCENE_SEED)
    r = out["rounds"][0]
    assert out["n_cylinders"] == 1 and r["best_trial"] == plain["best_trial"][0] and out["refit_used"][0] == 0
    assert r["fit"]["Rg2"] > 0 and np.float32(math.sqrt(r["fit"]["Rg2"]) * 2.0 ** -(17 - r["e"])) != np.float32(Rf)
    assert list(out["cylinders"][0]) == [float(v) for v in (*r["trial"][1], *r["trial"][2], Rf)]
