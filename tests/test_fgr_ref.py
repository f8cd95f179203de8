"""The references of fast global registration (tests/fgr_ref.py) against the planted scenes and against each other, and
the per-pair header that ships (pcreg_amd/csrc/fgr_pair.hpp) against its float64 restatement -- no GPU.

(a) THE CONDITION: run_ld returns exactly the planted inlier set on every generated case; run64 and run_tree do too, and the method
    error |run64 - run_ld| (the yardstick tests/test_gpu_fgr.py holds the device to) is printed.
(b) kept_mask equals a brute-force loop over the triples, with the built-in triples and with a table that holds out-of-range entries.
(c) with the scale of one side changed by 10 % no triple passes and failed = 1.
(d) fgr_pair.hpp and plane_fit.hpp as a stand-alone host program (tests/fgrpair/fgr_pair_main.cpp), built with the address and
    undefined-behaviour sanitizers (a toolchain that cannot link them fails the test): the 28 sums of a few pairs, one step and T * T_step equal
    run64's arithmetic bit for bit; so do liveness, rr, the weights, the triple verdicts and the anneal of mu."""
import os
import subprocess

import numpy as np
import pytest

import fgr_ref
import plane_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("k", range(len(fgr_ref.CASES)), ids=[f"n{c[0]}" for c in fgr_ref.CASES])
def test_the_planted_inlier_set_is_recovered(k):
    sc = fgr_ref.scenes()[k]
    o = fgr_ref.options()
    planted = (np.flatnonzero(sc["inliers"]) + 1).astype(np.int32)
    ld, r64, rt = (f(sc["p1"], sc["p2"], o) for f in (fgr_ref.run_ld, fgr_ref.run64, fgr_ref.run_tree))
    for r in (ld, r64, rt):
        assert not r["failed"] and r["n_kept"] == r["n_live"] == len(sc["p1"])
        np.testing.assert_array_equal(r["inlier_idx"], planted)
    E = fgr_ref.method_error([ld], [r64])
    R = ld["T"][:3, :3]
    ang = np.degrees(np.arccos(np.clip((np.trace(R @ sc["T"][:3, :3].T) - 1) / 2, -1, 1)))
    print(f"n = {len(sc['p1'])}: rotation error {ang:.4f} deg, E_method T {E['T']:.3e}, cost {E['cost']:.3e}, mu0 {ld['mu0']:.6g}, mu_final {ld['mu_final']:.6g}")
    assert ang < 0.05 and E["T"] < 1e-10 and E["cost"] < 1e-10
    assert ld["mu0"] == r64["mu0"] and ld["mu_final"] == r64["mu_final"]


def _brute(p1, p2, opts, b=0, tuple_idx=None):
    n = len(p1)
    kept = np.zeros(n, bool)
    if opts["n_tuples"] == 0:
        return np.array([all(np.isfinite(v) for v in list(p1[i]) + list(p2[i])) for i in range(n)], bool)
    if n < 3:
        return kept
    s2 = opts["tuple_scale"] * opts["tuple_scale"]
    d2 = lambda A, i, j: ((A[i][0] - A[j][0]) * (A[i][0] - A[j][0]) + (A[i][1] - A[j][1]) * (A[i][1] - A[j][1])) + (A[i][2] - A[j][2]) * (A[i][2] - A[j][2])
    for t in fgr_ref.triples(n, opts, b, tuple_idx):
        if not all(np.isfinite(p1[i]).all() and np.isfinite(p2[i]).all() for i in t):
            continue
        ok = True
        for i, j in ((t[0], t[1]), (t[0], t[2]), (t[1], t[2])):
            a, bb = d2(p1, i, j), d2(p2, i, j)
            ok = ok and s2 * a < bb and s2 * bb < a
        if ok:
            kept[t] = True
    return kept


def test_kept_mask_is_the_brute_force_loop():
    sc = fgr_ref.scenes()[0]
    p1, p2 = sc["p1"].copy(), sc["p2"].copy()
    p1[7, 1], p2[30, 2] = np.nan, np.inf
    for opts, b in ((fgr_ref.options(n_tuples=3000, seed=3), 0), (fgr_ref.options(n_tuples=500, seed=3), 4), (fgr_ref.options(), 0)):
        got = fgr_ref.kept_mask(p1, p2, opts, b)
        np.testing.assert_array_equal(got, _brute(p1, p2, opts, b))
        assert not got[7] and not got[30]
    assert 3 < fgr_ref.kept_mask(p1, p2, fgr_ref.options(n_tuples=3000, seed=3)).sum() < len(p1)
    rng = np.random.default_rng(5)
    table = rng.integers(-50, len(p1) + 50, (800, 3))
    opts = fgr_ref.options(n_tuples=800)
    got = fgr_ref.kept_mask(p1, p2, opts, 0, table)
    np.testing.assert_array_equal(got, _brute(p1, p2, opts, 0, table))
    assert got.any()


def test_a_changed_scale_passes_no_triple():
    sc = fgr_ref.scenes()[0]
    opts = fgr_ref.options(n_tuples=3000)
    for run in (fgr_ref.run_ld, fgr_ref.run64):
        r = run(sc["p1"] * 1.1, sc["p2"], opts)
        assert r["failed"] and r["n_kept"] == 0 and not r["kept"].any() and not r["T"].any() and r["n_inliers"] == 0
        assert r["n_live"] == len(sc["p1"])


# ---------------------------------------------------------------------------------------------------------------- (d) the header
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("fgrpair")
    src, exe = os.path.join(ROOT, "tests", "fgrpair", "fgr_pair_main.cpp"), str(d / "fgr_pair_main")
    subprocess.check_call(["g++"] + FLAGS + SAN + [src, "-o", exe])          # the sanitized build or none: no plain build in its place
    return exe, d


def _host(program, T, o, mu, p1, p2):
    exe, d = program
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    n = len(p1)
    np.concatenate([np.asarray(T, np.float64).reshape(4, 4).ravel(order="F"), o, [mu, float(n)], np.concatenate([p1, p2], axis=1).ravel()]).tofile(src)
    subprocess.check_call([exe, src, dst])             # a sanitizer report here fails the test
    out = np.fromfile(dst, np.float64)
    assert len(out) == 28 + 1 + 32 + 3 * n + max(n - 2, 0) + 1
    return dict(sums=out[:28], ok=out[28] == 1.0, S=out[29:45].reshape(4, 4, order="F"), Tn=out[45:61].reshape(4, 4, order="F"),
                per=out[61:61 + 3 * n].reshape(n, 3), tri=out[61 + 3 * n:-1] == 1.0, mu_next=out[-1])


@pytest.mark.parametrize("n", [3, 5, 40])
def test_header_equals_the_restatement(program, n):
    sc = fgr_ref.scenes()[0]
    rows = np.flatnonzero(sc["inliers"])[:n]
    p1, p2 = sc["p1"][rows], sc["p2"][rows]
    T = fgr_ref.compose(sc["T"], plane_ref.rigid([0.02, -0.01, 0.015], [0.3, -0.2, 0.1])) if n != 5 else np.eye(4)
    o, mu0 = fgr_ref.box_values(p1, p2, fgr_ref.options())
    for mu in (mu0, 1.0):
        got = _host(program, T, o, mu, p1, p2)
        want = fgr_ref.sums28(p1, p2, T, o, mu, fgr_ref._seq_sum)
        np.testing.assert_array_equal(_bits(got["sums"]), _bits(want))
        S = plane_ref.finish64(want, 3 * n, o)
        assert got["ok"] == (S is not None)
        if S is not None:
            S = S.reshape(4, 4, order="F")
            np.testing.assert_array_equal(_bits(got["S"]), _bits(S))
            np.testing.assert_array_equal(_bits(got["Tn"]), _bits(fgr_ref.compose(T, S)))
        _q, _r, rr = fgr_ref._residuals(p1, p2, T)
        t = mu / (mu + rr)
        np.testing.assert_array_equal(_bits(got["per"][:, 1]), _bits(rr))
        np.testing.assert_array_equal(_bits(got["per"][:, 2]), _bits(t * t))
        assert got["per"][:, 0].all()
        m = mu / 1.4
        assert got["mu_next"] == (m if m > 1.0 else 1.0)
    assert got["ok"] or n == 3


def test_header_liveness_triples_and_collinear_pairs(program):
    sc = fgr_ref.scenes()[0]
    p1, p2 = sc["p1"][:60].copy(), sc["p2"][:60].copy()
    p1[4, 0], p2[9, 1], p1[20, 2] = np.nan, -np.inf, np.inf
    got = _host(program, np.eye(4), np.zeros(3), 10.0, p1, p2)
    live = np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)
    np.testing.assert_array_equal(got["per"][:, 0] == 1.0, live)
    table = np.stack([np.arange(58), np.arange(58) + 1, np.arange(58) + 2], axis=1) + 1
    opts = fgr_ref.options(n_tuples=58)
    want = np.zeros(58, bool)
    for p in range(58):                                 # one triple at a time: the verdict of each
        want[p] = fgr_ref.kept_mask(p1, p2, fgr_ref.options(n_tuples=1), 0, table[p:p + 1]).any()
    np.testing.assert_array_equal(got["tri"], want)
    assert want.any() and not want.all()
    # collinear pairs: the rotation about their line is free, a pivot falls to 0 and the fit answers empty
    x = np.linspace(-3.0, 5.0, 9)
    line = np.stack([x, 2 * x + 1, -x], axis=1)
    got = _host(program, np.eye(4), fgr_ref.box_values(line, line, opts)[0], 4.0, line, line + [0.5, 0, 0])
    assert not got["ok"] and not got["S"].any()
    assert plane_ref.finish64(got["sums"], 27, fgr_ref.box_values(line, line, opts)[0]) is None
