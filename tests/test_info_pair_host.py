"""The per-pair terms that ship (pcreg_amd/csrc/info_pair.hpp), compiled for the host into a stand-alone
program (tests/infopair/info_pair_main.cpp), against their float64 restatement tests/ndt_ref.py: info_pair64 -- the 27 sums, y and
qq of both instantiations bit for bit, every fused add as the correctly rounded fma.  The header is plain C++17 without a HIP
include, so this needs no GPU; the device's ndt_moments_kernel (weighted) and gicp_moments_kernel (unweighted) call the same
functions.  The program is built with -Wall -Wextra -Werror, and with the address and undefined-behaviour sanitizers where the
toolchain links them (a plain build otherwise; the test prints which)."""
import os
import subprocess

import numpy as np
import pytest

import gicp_ref
import ndt_ref
import plane_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
EXTENT = 50.0                                          # the scenes' extent: residuals and levers up to this


def _records(cases):
    recs = np.zeros((len(cases), 40), np.float64)
    for r, (C, x, u, e, acc0) in zip(recs, cases):
        r[0:6], r[6:9], r[9:12], r[12], r[13:40] = C, x, u, e, acc0
    return recs


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("infopair")
    src, exe = os.path.join(ROOT, "tests", "infopair", "info_pair_main.cpp"), str(d / "info_pair_main")
    probe = str(d / "probe.bin")
    _records([([1, 0, 0, 1, 0, 1], [1, 2, 3], [4, 5, 6], 0.5, np.zeros(27))]).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("info_pair_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("info_pair_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


@pytest.fixture(scope="module")
def matrices():
    """-> (C [n, 6] of ndt_ref's Gaussians, W [n, 6] of gicp_ref.pair64)"""
    rng = np.random.default_rng(20261021)
    cloud = (rng.uniform(0, EXTENT, (600, 3)) * [1.0, 1.0, 0.2]).astype(np.float32)        # a slab: anisotropic Gaussians
    C = ndt_ref.table(cloud, 25.0)["C"]
    assert len(C) >= 4
    W = []
    while len(W) < 12:
        n, nq = rng.normal(size=(2, 3))
        T16 = gicp_ref.t16(plane_ref.rigid(rng.uniform(-1, 1, 3), rng.uniform(-EXTENT, EXTENT, 3)))
        w = gicp_ref.pair64(n / np.linalg.norm(n), nq / np.linalg.norm(nq), T16, 1.0 - (1e-3, 1e-6, 1.0)[len(W) % 3])
        if w is not None:
            W.append(w)
    return np.asarray(C, np.float64), np.asarray(W, np.float64)


def _bits(a):
    return np.asarray(a, np.float64).ravel().view(np.uint64).tolist()


def _check(program, cases):
    """every case: both instantiations' 27 sums, y and qq are info_pair64's bits -> the program's records [n, 2, 31]"""
    exe, d = program
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    _records(cases).tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, 2, 31)
    assert len(out) == len(cases)
    for c, o in zip(cases, out):
        for weighted, got in ((True, o[0]), (False, o[1])):
            acc, y, qq = ndt_ref.info_pair64(*c, weighted)
            assert _bits(got[:27]) == _bits(acc), (weighted, c)
            assert _bits(got[27:30]) == _bits(y) and _bits(got[30]) == _bits(qq), (weighted, c)
    return out


def _cases(rng, mats, n, weights, random_acc):
    cases = []
    for k in range(n):
        C = mats[k % len(mats)]
        scale = EXTENT * 10.0 ** -rng.integers(0, 4)                                       # from the extent down to a close pair
        x, u = rng.uniform(-scale, scale, 3), rng.uniform(-EXTENT, EXTENT, 3)
        acc0 = rng.normal(0, 1e4, 27) * (rng.random(27) < 0.8) if random_acc else np.zeros(27)
        cases.append((C, x, u, weights(k), acc0))
    return cases


@pytest.mark.parametrize("random_acc", [False, True])
def test_random_weights(program, matrices, random_acc):
    rng = np.random.default_rng(7 + random_acc)
    for mats in matrices:
        out = _check(program, _cases(rng, mats, 60, lambda k: 1.0 - rng.random(), random_acc))     # e in (0, 1]
        assert np.isfinite(out).all() and (out[:, :, :27] != 0).any(axis=0).all()                  # every sum is written


@pytest.mark.parametrize("random_acc", [False, True])
def test_weight_one_and_a_half(program, matrices, random_acc):
    """e = 0.5 and e = 1.0; with e = 1.0 the weighted sums are the unweighted ones, bit for bit"""
    rng = np.random.default_rng(11 + random_acc)
    for mats in matrices:
        cases = _cases(rng, mats, 40, lambda k: (1.0, 0.5)[k % 2], random_acc)
        out = _check(program, cases)
        for c, o in zip(cases, out):
            if c[3] == 1.0:
                assert _bits(o[0]) == _bits(o[1]), c
        assert any(_bits(o[0][:27]) != _bits(o[1][:27]) for c, o in zip(cases, out) if c[3] == 0.5)
