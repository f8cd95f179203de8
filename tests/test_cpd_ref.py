"""The references of the coherent-point-drift refit (tests/cpd_ref.py) against each other, against the point-to-point
reference, and the fit that ships (pcreg_amd/csrc/cpd_fit.hpp) against its float64 restatement -- no GPU.

(a) the METHOD ERROR |step32 - step_ld| of the main scene's six cases, printed: the yardstick tests/test_gpu_cpd.py holds the device to.
(b) the LIMIT: with w = 0 and sigma = 1/100 of the model's spacing, step_ld's T_step is the point-to-point step at r2 = +inf
    (tests/refit_ref.py: the nearest row, estimateTransform) -- the roles, the convention and the determinant rule are right.
(c) the TRAJECTORY of the worst perturbation over twenty steps, printed (recorded, not required).
(d) cpd_fit.hpp as a stand-alone host program (tests/cpdfit/cpd_fit_main.cpp), built with the address and undefined-behaviour
    sanitizers where the toolchain links them, equal to fit64 bit for bit on (a)'s sums and on a planar, a collinear and a
    reflected cross-covariance."""
import os
import subprocess

import numpy as np
import pytest

import cpd_ref
import plane_ref
import refit_ref
import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def test_method_error_of_the_main_scene():
    for w in cpd_ref.OUTLIERS:
        for s2 in cpd_ref.scene_sigma2s():
            ld, s32 = cpd_ref.scene_case(w, s2)
            both, E, draws = cpd_ref.method_error(ld, s32)
            print(f"w = {w}, sigma2_in = {s2:.6g}: empty (longdouble) {ld['empty'].astype(int)}, (fp32 restatement) {s32['empty'].astype(int)}")
            for k, v in E.items():
                print(f"    E_method {k}: {v:.3e}, the candidates' {draws[k][both]}")
            assert (ld["n_live"] == s32["n_live"]).all() and ld["n_live"].tolist() == [2500, 2500, 2500, 2500, 0, 0]
            assert ld["empty"][4:].all() and s32["empty"][4:].all()        # the all-zero transform and the one with a NaN
            if not (w > 0 and 0 < s2 < 1e-3):                              # (a variance far below the residual with w > 0: a handful of queries decide)
                assert both[:4].all()
                assert E["T_step"] < 1e-4 and all(E[k] < 1e-5 for k in ("sigma2_out", "Np", "sum_res2"))
            if w == 0:                                                     # every live query has p_i = 1
                assert np.abs(ld["Np"][:4] - 2500).max() < 1e-9 and np.abs(s32["Np"][:4] - 2500).max() < 1e-9


def test_small_variance_is_the_point_to_point_step():
    sc = plane_ref.scene()
    s2 = cpd_ref.scene_sigma2s()[2]
    ld, _ = cpd_ref.scene_case(0.0, s2)
    p2p = refit_ref.step(sc["surf"], sc["model"], sc["T"], np.inf)
    tq = score_ref.transformed(sc["surf"], sc["T"]).astype(np.float64)
    assert ld["empty"].tolist() == p2p["empty"].tolist() == [False] * 4 + [True] * 2
    for b in range(4):
        D = ld["T_step"][b] - p2p["T_step"][b]
        disp = np.linalg.norm(tq[b] @ D[:3, :3] + D[3, :3], axis=1).max()
        gap = ld["gap"][b]                  # the mean distance between a query's weighted model point and its nearest row
        print(f"candidate {b}: soft-to-hard gap {gap:.3e}, largest displacement between the two steps {disp:.3e}, |dT|_F {np.linalg.norm(D):.3e}")
        assert disp <= 10 * gap + 1e-9      # (1e-9: the point-to-point fit's own bound against its oracle)
        assert abs(np.linalg.det(ld["T_step"][b][:3, :3]) - 1) < 1e-12


def test_trajectory_of_the_worst_perturbation():
    sc = plane_ref.scene()
    start = plane_ref.rms_to_truth(sc["surf"], sc["T"][3], sc["cloud"])
    rms = cpd_ref.trajectory()
    print(f"RMS to truth: start {start:.4f}; after {cpd_ref.TRAJECTORY_STEPS} steps {[round(r, 4) for r in rms]}")
    assert all(np.isfinite(rms))


# ---------------------------------------------------------------------------------------------------------------- (d) the header
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("cpdfit")
    src, exe = os.path.join(ROOT, "tests", "cpdfit", "cpd_fit_main.cpp"), str(d / "cpd_fit_main")
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("cpd_fit_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("cpd_fit_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    return exe, d


def _check(program, cases):
    """cases: (sums [19], o [3]) -> the verdicts; every case: the same verdict as fit64 and the same bits"""
    exe, d = program
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    np.array([np.concatenate([s, o]) for s, o in cases], np.float64).tofile(src)
    subprocess.check_call([exe, src, dst])             # a sanitizer report here fails the test
    out = np.fromfile(dst, np.float64).reshape(-1, 18)
    assert len(out) == len(cases)
    for (s, o), r in zip(cases, out):
        want = cpd_ref.fit64(s, o)
        assert (r[0] == 1.0) == (want is not None)
        if want is None:
            assert not r[1:].any()
        else:
            assert r[1:17].view(np.uint64).tolist() == want[0].view(np.uint64).tolist()
            assert r[17:].view(np.uint64).tolist() == np.array([want[1]]).view(np.uint64).tolist()
    return out[:, 0] == 1.0


def sums_of(u, y, p, extra=1.0):
    """the 19 sums of weighted pairs (u_i, y_i / p_i) with weights p_i; `extra` scales the residual terms"""
    s = np.zeros(19)
    m = y / p[:, None]
    s[0], s[1:4], s[4:7] = p.sum(), (p[:, None] * u).sum(axis=0), y.sum(axis=0)
    s[7:16] = (u[:, :, None] * y[:, None, :]).sum(axis=0).ravel()
    s[16], s[17] = (p * (u * u).sum(axis=1)).sum(), (p * (m * m).sum(axis=1)).sum() + extra
    s[18] = extra
    return s


def test_fit_header_on_the_scene_sums(program):
    o = plane_ref.origin(cpd_ref.live_rows(plane_ref.scene()["model"]))
    cases = [(cpd_ref.scene_case(w, s2)[1]["sums"][b], o) for w in cpd_ref.OUTLIERS for s2 in cpd_ref.scene_sigma2s()[:2] for b in range(4)]
    assert _check(program, cases).all()


def test_fit_header_on_degenerate_cross_covariances(program):
    rng = np.random.default_rng(27)
    o = np.array([170.0, -30.0, 12.0])
    u = rng.normal(0, 5, (40, 3))
    p = rng.uniform(0.2, 1.0, 40)
    R = plane_ref.rigid([0.2, -0.1, 0.3], [0, 0, 0])[:3, :3]
    flat, line = u * [1, 1, 0], u * [1, 0, 0]
    mirror = u * [1, 1, -1]
    cases = [(sums_of(u, p[:, None] * (u @ R + [0.3, -0.2, 0.1]), p), o),              # a rigid motion: found
             (sums_of(flat, p[:, None] * (flat @ R), p), o),                            # planar: two singular values, a rotation
             (sums_of(line, p[:, None] * (line @ R), p), o),                            # collinear: one, empty
             (sums_of(u, p[:, None] * mirror, p), o),                                   # a reflection: a proper rotation all the same
             (sums_of(u, p[:, None] * u, p, extra=0.0), o),                             # the identity with no residual: sigma2_out = 0 or below, empty
             (np.zeros(19), o), (np.full(19, np.nan), o)]
    ok = _check(program, cases)
    assert ok[:2].all() and not ok[2] and ok[3] and not ok[5:].any()
    T = np.array(cpd_ref.fit64(*cases[3])[0]).reshape(4, 4)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12                                    # the determinant correction
    T = np.array(cpd_ref.fit64(*cases[0])[0]).reshape(4, 4)
    assert np.abs(T[:3, :3].T - R).max() < 1e-12                                        # [p, 1] @ T moves u onto u @ R
