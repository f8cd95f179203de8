"""The fit that ships (pcreg_amd/csrc/plane_fit.hpp), compiled for the host into a stand-alone program
(tests/planefit/plane_fit_main.cpp), against its float64 restatement tests/plane_ref.py: finish64 -- the verdict exactly, T_step
bit for bit.  The header is plain C++17 without a HIP include, so this needs no GPU; the device's plane_finish_kernel calls the
same function.  The program is built with -Wall -Wextra -Werror, and with the address and undefined-behaviour sanitizers where
the toolchain links them (a plain build otherwise; the test prints which)."""
import os
import subprocess

import numpy as np
import pytest

import plane_ref
from plane_ref import tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("planefit")
    src, exe = os.path.join(ROOT, "tests", "planefit", "plane_fit_main.cpp"), str(d / "plane_fit_main")
    probe = str(d / "probe.bin")
    np.zeros(32).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("plane_fit_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("plane_fit_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


def _run(program, recs):
    exe, d = program
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, 32)
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    recs.tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, 17)
    assert len(out) == len(recs)
    return out


def _check(program, recs):
    """-> the verdicts; every record: the same verdict as finish64 and the same 16 x 64 bits"""
    recs = np.asarray(recs, np.float64).reshape(-1, 32)
    out = _run(program, recs)
    for r, o in zip(recs, out):
        want = plane_ref.finish64(r[:28], int(r[28]), r[29:32])
        assert (o[0] == 1.0) == (want is not None), r
        if want is None:
            assert not o[1:].any() and not np.signbit(o[1:]).any()
        else:
            assert o[1:].view(np.uint64).tolist() == want.view(np.uint64).tolist(), r
    return out[:, 0] == 1.0


def _from_pairs(rng, n, spread=10.0, o=(3.0, -2.0, 5.0)):
    """the float64 sums of n random plane pairs about o, as one record"""
    p = rng.normal(0, spread, (n, 3)) + o
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    m = p + rng.normal(0, 0.05 * spread, (n, 3))
    sums, cnt = plane_ref.sums_of_pairs(m, p, nrm, o)
    return np.concatenate([sums.astype(np.float64), [cnt], o])


def _with_last_pivot(rng, pivot):
    """sums whose scaled matrix has unit-length Cholesky rows and, up to rounding, `pivot` as the last pivot"""
    L = np.zeros((6, 6))
    for i in range(6):
        v = rng.normal(size=i)
        keep = pivot if i == 5 else rng.uniform(0.2, 0.9)
        L[i, :i] = v / np.linalg.norm(v) * np.sqrt(1.0 - keep) if i else v
        L[i, i] = np.sqrt(keep if i else 1.0)
    s = 10.0 ** rng.uniform(-2, 3, 6)
    A = (L @ L.T) * np.outer(s, s)
    rec = np.zeros(32)
    for i in range(6):
        for j in range(i, 6):
            rec[tri(i, j)] = A[i, j]
    rec[21:27] = rng.normal(size=6) * s
    rec[27], rec[28], rec[29:] = 1.0, 100, rng.normal(0, 50, 3)
    return rec


def test_random_well_conditioned_sets(program):
    rng = np.random.default_rng(20261019)
    recs = [_from_pairs(rng, int(n), spread=float(sp), o=tuple(rng.normal(0, 100, 3))) for n, sp in
            zip(rng.integers(20, 200, 200), 10.0 ** rng.uniform(-1, 2, 200))]
    ok = _check(program, recs)
    assert ok.all()


def test_pivots_on_either_side_of_the_threshold(program):
    rng = np.random.default_rng(7)
    t = 2.0 ** -26
    recs = [_with_last_pivot(rng, t * f) for f in np.concatenate([np.geomspace(0.25, 4.0, 61), [1e-3, 1e3, 1e6]])]
    ok = _check(program, recs)
    print(f"near 2^-26: {int(ok.sum())} fits, {int((~ok).sum())} empty")
    assert ok[-2:].all() and not ok[0] and not ok[61] and ok.sum() >= 20 and (~ok).sum() >= 20          # both verdicts are exercised


def test_the_empty_rules(program):
    rng = np.random.default_rng(11)
    good = _from_pairs(rng, 60)
    recs = []
    for n in (0, 5, 6, 7):                             # the count rule on sums that would fit
        r = good.copy(); r[28] = n; recs.append(r)
    for i in range(6):                                 # a zero, a negative, an infinite and a NaN diagonal entry
        for v in (0.0, -1.0, np.inf, np.nan):
            r = good.copy(); r[tri(i, i)] = v; recs.append(r)
    for k in list(range(27)) + [29, 30, 31]:           # NaN and inf anywhere the fit reads (rr at 27 is not read)
        for v in (np.nan, np.inf):
            r = good.copy(); r[k] = v; recs.append(r)
    r = good.copy(); r[27] = np.nan; recs.append(r)
    recs.append(_from_pairs(rng, 5)); recs.append(_from_pairs(rng, 6)); recs.append(_from_pairs(rng, 7))      # six unknowns from 5, 6, 7 pairs
    flat = good.copy()                                 # a flat model: J_2 = J_3 = J_4 = 0 throughout
    for i in range(6):
        for j in range(i, 6):
            if {i, j} & {2, 3, 4}:
                flat[tri(i, j)] = 0.0
    flat[23:26] = 0.0
    recs.append(flat)
    ok = _check(program, recs)
    assert ok[:4].tolist() == [False, False, True, True]
    assert not ok[4:28].any() and not ok[28:88].any() and ok[88]
    assert not ok[89] and ok[90] and ok[91] and not ok[92]
