"""The sphere refit that ships (pcreg_amd/csrc/sphere_fit.hpp), compiled for the host into a stand-alone program
(tests/spherefit/sphere_fit_main.cpp), against its float64 restatement tests/spheres_ref.py: finish64 -- the verdict exactly, centre
and R bit for bit.  The header is plain C++17 without a HIP include, so this needs no GPU; the device's sf_solve_kernel calls the
same function.  The program is built with -Wall -Wextra -Werror, and with the address and undefined-behaviour sanitizers where the
toolchain links them (a plain build otherwise; the test prints which).  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import spheres_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
W = 20


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("spherefit")
    src, exe = os.path.join(ROOT, "tests", "spherefit", "sphere_fit_main.cpp"), str(d / "sphere_fit_main")
    probe = str(d / "probe.bin")
    np.zeros(W).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("sphere_fit_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("sphere_fit_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


def _run(program, recs):
    exe, d = program
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, W)
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    recs.tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, 5)
    assert len(out) == len(recs)
    return out


def _want(r):
    return ref.finish64(r[0:6], r[6:9], r[9:12], r[12], r[13], r[14:17], r[17], r[18], r[19])


def _check(program, recs):
    """-> the verdicts; every record: the same verdict as finish64 and the same 4 x 64 bits"""
    recs = np.asarray(recs, np.float64).reshape(-1, W)
    out = _run(program, recs)
    for r, o in zip(recs, out):
        want = _want(r)
        assert (o[0] == 1.0) == want["used"], r
        if not want["used"]:
            assert not o[1:].any() and not np.signbit(o[1:]).any()
        else:
            got = np.array([*want["centre"], want["R"]], np.float64)
            assert o[1:].view(np.uint64).tolist() == got.view(np.uint64).tolist(), r
    return out[:, 0] == 1.0


def _record(N6, h, S1, sw, n, p0=(3.0, -2.0, 5.0), back=2.0 ** -12, rmin=0.0, rmax=np.inf):
    return np.array([*N6, *h, *S1, sw, n, *p0, back, np.float32(rmin), np.float32(rmax)], np.float64)


def _from_rows(rng, n, R=5.0, sigma=0.02, e=5, cap=1.0, rmin=0.0, rmax=np.inf):
    """the normal equations of n noisy rows on a sphere (the part of it with z / R >= 1 - 2 cap), through the integer sums"""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 2] = 1.0 - cap * (1.0 - v[:, 2])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    c = rng.uniform(-8, 8, 3)
    rows = (c + v * (R + rng.normal(0, sigma, (n, 1)))).astype(np.float32)
    p0 = rows[0]
    g = [[int(x) for x in row] for row in np.rint((rows - p0).astype(np.float64) * 2.0 ** (17 - e))]
    return _record(*ref.normal_equations(ref.integer_sums(g)), p0=[float(x) for x in p0], back=2.0 ** -(17 - e), rmin=rmin, rmax=rmax)


def test_random_sets(program):
    rng = np.random.default_rng(20261020)
    recs = [_from_rows(rng, int(n), R=float(R), sigma=float(sg), e=int(e), cap=float(cap)) for n, R, sg, e, cap in
            zip(rng.integers(8, 400, 300), 10.0 ** rng.uniform(-0.5, 1, 300), 10.0 ** rng.uniform(-4, -1, 300), rng.integers(4, 9, 300),
                rng.uniform(0.05, 1.0, 300))]
    ok = _check(program, recs)
    assert ok.all()


def test_radicands_on_either_side_of_zero(program):
    rng = np.random.default_rng(7)
    recs = []
    for k in range(3):                                 # radicand k = r0, r1, r2 swept through 0 with the others well above it
        for f in np.concatenate([-np.geomspace(1e-18, 1.0, 20), [0.0], np.geomspace(1e-18, 1.0, 20)]):
            L = np.tril(rng.normal(size=(3, 3)))
            L[np.diag_indices(3)] = rng.uniform(0.5, 2.0, 3)
            L[k, k] = np.sqrt(abs(f))                  # row k of L keeps its off-diagonal size; its pivot is sqrt(|f|)
            N = L @ L.T * 1e12
            N[k, k] = (float(L[k, :k] @ L[k, :k]) + f) * 1e12
            recs.append(_record([N[0, 0], N[0, 1], N[0, 2], N[1, 1], N[1, 2], N[2, 2]], rng.normal(size=3) * 1e14, rng.normal(size=3) * 1e4,
                                1e12, 100.0))
    ok = _check(program, recs).reshape(3, 41)
    print("refits used per radicand, of 41:", ok.sum(axis=1).tolist())
    assert not ok[:, 10:20].any()                      # a radicand below zero by more than rounding (f <= -3e-10): never used
    assert (ok[:, 30:].sum(axis=1) >= 5).all()         # clearly above it: used wherever R_g^2 allows


def test_rg2_on_either_side_of_zero(program):
    rng = np.random.default_rng(9)
    base = _from_rows(rng, 200)
    f = _want(base)
    a, S1, n = f["a"], base[9:12], base[13]
    c2 = sum((v / 2) ** 2 for v in a)
    dot = sum(x * y for x, y in zip(a, S1))
    recs = []
    for d in np.concatenate([-np.geomspace(1e-15, 1.0, 30), [0.0], np.geomspace(1e-15, 1.0, 30)]):
        r = base.copy()
        r[12] = dot - n * c2 * (1.0 - d)               # beta ~ -|c_g|^2 (1 - d): R_g^2 ~ d |c_g|^2
        recs.append(r)
    ok = _check(program, recs)
    rg2 = np.array([_want(r)["Rg2"] for r in recs])
    print(f"R_g^2 swept from {rg2.min():.3e} to {rg2.max():.3e}: {int(ok.sum())} used, {int((~ok).sum())} not")
    assert np.array_equal(ok, rg2 > 0) and ok.sum() >= 20 and (~ok).sum() >= 20


def test_radius_bounds_and_non_finite_entries(program):
    rng = np.random.default_rng(11)
    good = _from_rows(rng, 120)
    R32 = np.float32(_want(good)["R"])
    up, dn = np.nextafter(R32, np.float32(np.inf)), np.nextafter(R32, np.float32(-np.inf))
    recs = []
    for lo, hi in ((R32, R32), (0, R32), (R32, np.inf), (up, np.inf), (0, dn), (dn, up), (0, 0)):
        r = good.copy(); r[18], r[19] = lo, hi; recs.append(r)
    for k in range(18):                                # NaN and inf anywhere the fit reads
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = v; recs.append(r)
    ok = _check(program, recs)
    assert ok[:7].tolist() == [True, True, True, False, False, True, False]
    assert not ok[7:7 + 3 * 9].any()                   # N and h: a non-finite entry there reaches a radicand or the sphere
