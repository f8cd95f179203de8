"""The pair weight that ships (pcreg_amd/csrc/gicp_pair.hpp), compiled for the host into a stand-alone program
(tests/gicppair/gicp_pair_main.cpp), against its float64 restatement tests/gicp_ref.py: pair64 -- the verdict exactly, W bit for
bit.  The header is plain C++17 without a HIP include, so this needs no GPU; the device's gicp_moments_kernel calls the same
function.  The program is built with -Wall -Wextra -Werror, and with the address and undefined-behaviour sanitizers where the
toolchain links them (a plain build otherwise; the test prints which)."""
import os
import subprocess

import numpy as np
import pytest

import gicp_ref
import plane_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
EPSILONS = (1e-6, 1e-3, 1.0)


def _records(cases):
    recs = np.zeros((len(cases), 23), np.float64)
    for r, (n, nq, T16, a) in zip(recs, cases):
        r[0:3], r[3:6], r[6:22], r[22] = np.asarray(n, np.float32), np.asarray(nq, np.float32), T16, a
    return recs


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("gicppair")
    src, exe = os.path.join(ROOT, "tests", "gicppair", "gicp_pair_main.cpp"), str(d / "gicp_pair_main")
    probe = str(d / "probe.bin")
    _records([([0, 0, 1], [0, 1, 0], np.eye(4).ravel(), 0.999)]).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("gicp_pair_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("gicp_pair_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


def _check(program, cases):
    """-> the verdicts; every case: the same verdict as pair64 and the same bits of W"""
    exe, d = program
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    _records(cases).tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, 7)
    assert len(out) == len(cases)
    for c, o in zip(cases, out):
        W = gicp_ref.pair64(*c)
        assert (o[0] == 1.0) == (W is not None), c
        if W is None:
            assert not o[1:].any() and not np.signbit(o[1:]).any()
        else:
            assert o[1:].view(np.uint64).tolist() == np.array(W, np.float64).view(np.uint64).tolist(), c
    return out[:, 0] == 1.0


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _rigid16(rng):
    return gicp_ref.t16(plane_ref.rigid(rng.uniform(-1, 1, 3), rng.uniform(-50, 50, 3)))


def test_random_pairs(program):
    rng = np.random.default_rng(20261020)
    cases = []
    for eps in EPSILONS:
        for n, nq in zip(_unit(rng, 100), _unit(rng, 100)):
            cases.append((n, nq, _rigid16(rng), 1.0 - eps))
        for n, nq in zip(_unit(rng, 40), _unit(rng, 40)):          # lengths off 1, both ways, and a transform that is not rigid
            T16 = _rigid16(rng)
            T16[[0, 1, 2, 4, 5, 6, 8, 9, 10]] *= rng.uniform(0.7, 1.2)
            cases.append((n * np.float32(rng.uniform(0.5, 1.3)), nq * np.float32(rng.uniform(0.5, 1.3)), T16, 1.0 - eps))
    ok = _check(program, cases)
    assert ok[:100].all() and ok.sum() > len(cases) // 2


def test_parallel_orthogonal_and_long_normals(program):
    rng = np.random.default_rng(5)
    I16 = np.eye(4).ravel()
    cases, want = [], []
    for eps in EPSILONS:
        a = 1.0 - eps
        for n in list(np.eye(3, dtype=np.float32)) + list(_unit(rng, 5)):
            cases.append((n, n, I16, a)); want.append(True)                      # parallel: S has the eigenvalue 2 eps along n
            cases.append((n, -n, I16, a)); want.append(True)
            t = np.cross(n, [0.3, -0.5, 0.8]).astype(np.float32)
            cases.append((n, t / np.linalg.norm(t), I16, a)); want.append(True)  # orthogonal (up to fp32 rounding)
            # a normal of length 1.5: S_nn = 2 - a (2.25 + ..) < 0 unless a is small -- judged exactly as pair64 judges it
            cases.append((np.float32(1.5) * n, n, I16, a)); want.append(None)
            cases.append((n, np.float32(1.5) * n, I16, a)); want.append(None)
        cases.append(([0, 0, 0], [0, 0, 0], I16, a)); want.append(True)          # zero normals: S = 2 I
    ok = _check(program, cases)
    for c, o, w in zip(cases, ok, want):
        if w is not None:
            assert o == w, c
    long_ = [o for o, w, c in zip(ok, want, cases) if w is None]
    assert not any(long_[:2 * 16]) and all(long_[-16:])                          # degenerate at epsilon 1e-6 and 1e-3, S = 2 I at epsilon = 1


def test_nan_and_inf_components(program):
    rng = np.random.default_rng(9)
    cases = []
    for eps in EPSILONS:
        for bad in (np.nan, np.inf, -np.inf):
            for side in (0, 1):
                for c in range(3):
                    n, nq = _unit(rng, 2)
                    (n if side == 0 else nq)[c] = bad
                    cases.append((n, nq, _rigid16(rng), 1.0 - eps))
            T16 = _rigid16(rng)
            T16[int(rng.integers(0, 3)) * 4 + int(rng.integers(0, 3))] = bad     # in the rotation part: v is not finite
            cases.append((*_unit(rng, 2), T16, 1.0 - eps))
        T16 = _rigid16(rng)
        T16[3] = np.nan                                                          # in the translation: not read
        cases.append((*_unit(rng, 2), T16, 1.0 - eps))
        cases.append((np.float32([3e38, 0, 0]), np.float32([0, 1, 0]), _rigid16(rng), 1.0 - eps))     # n_x n_x overflows a float, not a double
        cases.append((*_unit(rng, 2), np.zeros(16), 1.0 - eps))                  # the all-zero transform: v = 0
    ok = _check(program, cases)
    per = len(cases) // 3
    for e in range(3):
        blk = ok[e * per:(e + 1) * per]
        assert not blk[:21].any() and blk[21] and blk[23]
