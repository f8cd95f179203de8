"""The cylinder refit that ships (pcreg_amd/csrc/cylinder_fit.hpp), compiled for the host into a stand-alone program
(tests/cylinderfit/cylinder_fit_main.cpp), against its float64 restatement tests/cylinders_ref.py: finish64 -- both verdicts
exactly, and w, u, v, centre and R bit for bit.  The header is plain C++17 without a HIP include, so this needs no GPU; the
device's cy_basis_kernel and cy_solve_kernel call the same functions.  The program is built with -Wall -Wextra -Werror, and with
the address and undefined-behaviour sanitizers where the toolchain links them (a plain build otherwise; the test prints which).
Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import cylinders_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
W, WO = 26, 15


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("cylinderfit")
    src, exe = os.path.join(ROOT, "tests", "cylinderfit", "cylinder_fit_main.cpp"), str(d / "cylinder_fit_main")
    probe = str(d / "probe.bin")
    np.zeros(W).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("cylinder_fit_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("cylinder_fit_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


def _run(program, recs):
    exe, d = program
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, W)
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    recs.tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, WO)
    assert len(out) == len(recs)
    return out


def _want(r):
    return ref.finish64(r[0:6], int(r[6]), (r[11:14], r[14:16], r[16:18], r[18], r[19]), r[20:23], r[23], r[24], r[25],
                        r[8:11] if r[7] else None)


def _bits(v):
    return np.asarray(v, np.float64).view(np.uint64).tolist()


def _check(program, recs):
    """-> (basis verdicts, used verdicts); every record: finish64's verdicts and the same bits"""
    recs = np.asarray(recs, np.float64).reshape(-1, W)
    out = _run(program, recs)
    for r, o in zip(recs, out):
        want = _want(r)
        assert (o[0] == 1.0) == want["basis_ok"], r
        assert (o[10] == 1.0) == want["used"], r
        if not want["basis_ok"]:
            assert not o[1:].any() and not np.signbit(o[1:]).any()
            continue
        assert _bits(o[1:10]) == _bits([*want["w"], *want["u"], *want["v"]]), r
        if want["used"]:
            assert _bits(o[11:]) == _bits([*want["centre"], want["R"]]), r
        else:
            assert not o[11:].any() and not np.signbit(o[11:]).any()
    return out[:, 0] == 1.0, out[:, 10] == 1.0


def _record(A6, n_n, circle, p0=(3.0, -2.0, 5.0), back=2.0 ** -12, rmin=0.0, rmax=np.inf, ref_vec=None):
    N3, h, S1, sw, n = circle
    rv = [1.0, *ref_vec] if ref_vec is not None else [0.0, 0.0, 0.0, 0.0]
    return np.array([*A6, n_n, *rv, *N3, *h, *S1, sw, n, *p0, back, np.float32(rmin), np.float32(rmax)], np.float64)


def _cloud(rng, n, R=3.0, sigma=0.02, turn=2 * np.pi, axis=None, nsig=0.03):
    w, u, v = ref._frame(rng.normal(size=3) if axis is None else axis)
    th, hh = rng.uniform(0, turn, n), rng.uniform(-4, 4, n)
    rad = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
    rows = (rng.uniform(-8, 8, 3) + hh[:, None] * w + rad * (R + rng.normal(0, sigma, (n, 1)))).astype(np.float32)
    nrm = rad + rng.normal(0, nsig, rad.shape) if nsig else rad
    if nsig:
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return rows, nrm.astype(np.float32)


def _from_rows(rows, nrm, e=5, rmin=0.0, rmax=np.inf, ref_vec=None, n_n=None):
    """the record of a set of inliers through both sets of integer sums (the circle's on finish64's own basis; where there is no
    basis, on the coordinate axes x and y, so that the record stays well formed)"""
    asums, _ = ref.axis_sums(nrm)
    p0 = rows[0]
    g = [[int(x) for x in row] for row in np.rint((rows - p0).astype(np.float64) * 2.0 ** (17 - e))]
    nn = asums[0] if n_n is None else n_n
    ok, _, u, v = ref.basis64([float(x) for x in asums[1:]], nn, ref_vec)
    if not ok:
        u, v = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    S, _ = ref.circle_sums(g, u, v)
    return _record([float(x) for x in asums[1:]], nn, ref.normal_equations(S), p0=[float(x) for x in p0], back=2.0 ** -(17 - e), rmin=rmin,
                   rmax=rmax, ref_vec=ref_vec)


def test_random_sets(program):
    rng = np.random.default_rng(20261020)
    recs = []
    for n, R, sg, e, turn, k in zip(rng.integers(8, 400, 300), 10.0 ** rng.uniform(-0.5, 1, 300), 10.0 ** rng.uniform(-4, -1, 300),
                                    rng.integers(4, 9, 300), rng.uniform(0.5, 2 * np.pi, 300), range(300)):
        rows, nrm = _cloud(rng, int(n), float(R), float(sg), float(turn))
        recs.append(_from_rows(rows, nrm, int(e), ref_vec=rng.normal(size=3) if k % 3 == 0 else None))
    basis, used = _check(program, recs)
    assert basis.all() and used.all()


def test_usable_normal_counts_and_parallel_normals(program):
    rng = np.random.default_rng(5)
    rows, nrm = _cloud(rng, 150)
    recs = [_from_rows(rows, nrm, n_n=k) for k in (0, 1, 2, 3)]          # n_n 0 and 1: no basis whatever the sums hold
    flat = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (150, 1))    # a plane's inliers: all normals parallel
    recs.append(_from_rows(rows, flat))
    recs.append(_from_rows(rows, -flat))
    nan = nrm.copy(); nan[:] = np.nan                                    # no usable normal at all: the sums are zero, n_n = 0
    recs.append(_from_rows(rows, nan))
    basis, used = _check(program, recs)
    assert basis.tolist() == [False, False, True, True, True, True, False]
    assert recs[4][:6].tolist() == recs[5][:6].tolist()                  # the sign of the normals is not in the sums


def test_axis_along_each_coordinate_axis(program):
    """exact normals in a coordinate plane: A6 has a zero row and column, Jacobi turns within the other two at most, w is a
    coordinate axis exactly and two components tie at magnitude 0 -- the first of them is e_k"""
    rng = np.random.default_rng(6)
    recs, want_w = [], []
    for ax in range(3):
        rows, _ = _cloud(rng, 64, axis=np.eye(3)[ax], nsig=0)
        others = [c for c in range(3) if c != ax]
        nrm = np.zeros((64, 3), np.float32)
        pick = rng.integers(0, 4, 64)
        nrm[np.arange(64), np.array(others)[pick % 2]] = np.where(pick < 2, 1.0, -1.0)      # +-e_a, +-e_b: a diagonal A6
        recs.append(_from_rows(rows, nrm))
        th = rng.uniform(0, 2 * np.pi, 64)
        nrm2 = np.zeros((64, 3), np.float32)
        nrm2[:, others[0]], nrm2[:, others[1]] = np.cos(th), np.sin(th)                       # a turning Jacobi, a zero third row
        recs.append(_from_rows(rows, nrm2))
        want_w += [ax, ax]
    basis, used = _check(program, recs)
    assert basis.all() and used.all()
    out = _run(program, recs)
    for o, ax in zip(out, want_w):
        assert np.abs(o[1:4]).tolist() == np.eye(3)[ax].tolist()
        k = [c for c in range(3) if c != ax][0]                                               # the first of the two zero components
        assert np.abs(o[4:7]).tolist() == np.abs(np.cross(np.eye(3)[ax], np.eye(3)[k])).tolist()


def test_radicands_on_either_side_of_zero(program):
    rng = np.random.default_rng(7)
    rows, nrm = _cloud(rng, 100)
    base = _from_rows(rows, nrm)
    recs = []
    for k in range(2):                                 # radicand k = r0, r1 swept through 0 with the other well above it
        for f in np.concatenate([-np.geomspace(1e-18, 1.0, 20), [0.0], np.geomspace(1e-18, 1.0, 20)]):
            L = np.tril(rng.normal(size=(2, 2)))
            L[np.diag_indices(2)] = rng.uniform(0.5, 2.0, 2)
            L[k, k] = np.sqrt(abs(f))
            N = L @ L.T * 1e12
            N[k, k] = (float(L[k, :k] @ L[k, :k]) + f) * 1e12
            r = base.copy()
            r[11:14] = [N[0, 0], N[0, 1], N[1, 1]]
            r[14:16] = rng.normal(size=2) * 1e14
            r[16:18] = rng.normal(size=2) * 1e4
            r[18], r[19] = 1e12, 100.0
            recs.append(r)
    basis, used = _check(program, recs)
    used = used.reshape(2, 41)
    print("refits used per radicand, of 41:", used.sum(axis=1).tolist())
    assert basis.all()
    assert not used[:, 10:20].any()                    # a radicand below zero by more than rounding: never used
    assert (used[:, 30:].sum(axis=1) >= 5).all()       # clearly above it: used wherever R_g^2 allows


def test_rg2_on_either_side_of_zero(program):
    rng = np.random.default_rng(9)
    rows, nrm = _cloud(rng, 200)
    base = _from_rows(rows, nrm)
    f = _want(base)
    a, S1, n = f["a"], base[16:18], base[19]
    c2 = sum((x / 2) ** 2 for x in a)
    dot = sum(x * y for x, y in zip(a, S1))
    recs = []
    for d in np.concatenate([-np.geomspace(1e-15, 1.0, 30), [0.0], np.geomspace(1e-15, 1.0, 30)]):
        r = base.copy()
        r[18] = dot - n * c2 * (1.0 - d)               # beta ~ -|c2|^2 (1 - d): R_g^2 ~ d |c2|^2
        recs.append(r)
    _, used = _check(program, recs)
    rg2 = np.array([_want(r)["Rg2"] for r in recs])
    print(f"R_g^2 swept from {rg2.min():.3e} to {rg2.max():.3e}: {int(used.sum())} used, {int((~used).sum())} not")
    assert np.array_equal(used, rg2 > 0) and used.sum() >= 20 and (~used).sum() >= 20


def test_radius_bounds_and_non_finite_entries(program):
    rng = np.random.default_rng(11)
    rows, nrm = _cloud(rng, 120)
    good = _from_rows(rows, nrm)
    R32 = np.float32(_want(good)["R"])
    up, dn = np.nextafter(R32, np.float32(np.inf)), np.nextafter(R32, np.float32(-np.inf))
    recs = []
    for lo, hi in ((R32, R32), (0, R32), (R32, np.inf), (up, np.inf), (0, dn), (dn, up), (0, 0)):
        r = good.copy(); r[24], r[25] = lo, hi; recs.append(r)
    idx = list(range(0, 6)) + list(range(11, 24))
    for k in idx:                                      # NaN and inf anywhere the fit reads
        for x in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = x; recs.append(r)
    basis, used = _check(program, recs)
    assert used[:7].tolist() == [True, True, True, False, False, True, False]
    assert not used[7:7 + 3 * 6].any()                 # a non-finite entry of A6 reaches Jacobi's output or the basis
    assert not used[7 + 3 * 6:7 + 3 * 11].any()        # N and h: a non-finite entry there reaches a radicand or the cylinder
