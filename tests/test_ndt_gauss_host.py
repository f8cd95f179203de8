"""The voxel Gaussian that ships (pcreg_amd/csrc/ndt_gauss.hpp), compiled for the host into a stand-alone program
(tests/ndtgauss/ndt_gauss_main.cpp), against its float64 restatement tests/ndt_ref.py: gauss64 -- the verdict exactly, the mean
and C bit for bit.  The header is plain C++17 without a HIP include, so this needs no GPU; the device's ndt_gauss_kernel calls
the same function.  The program is built with -Wall -Wextra -Werror, and with the address and undefined-behaviour sanitizers
where the toolchain links them (a plain build otherwise; the test prints which)."""
import os
import subprocess

import numpy as np
import pytest

import ndt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pcreg_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
KMAX = 64
MIN_POINTS = 6


def _records(sets):
    recs = np.zeros((len(sets), 1 + 3 * KMAX), np.float32)
    for r, s in zip(recs, sets):
        s = np.asarray(s, np.float32).reshape(-1, 3)
        r[0] = len(s)
        r[1:1 + 3 * len(s)] = s.ravel()
    return recs


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("ndtgauss")
    src, exe = os.path.join(ROOT, "tests", "ndtgauss", "ndt_gauss_main.cpp"), str(d / "ndt_gauss_main")
    probe = str(d / "probe.bin")
    _records([np.eye(3)]).tofile(probe)
    san = subprocess.run(["g++"] + FLAGS + SAN + [src, "-o", exe], stderr=subprocess.PIPE, text=True)
    if san.returncode == 0:
        print("ndt_gauss_main: built with -fsanitize=address,undefined")
    else:                                              # the toolchain lacks the runtimes (a link failure): say so, build plain
        print("ndt_gauss_main: the sanitized build failed, a plain build instead:\n" + san.stderr)
        subprocess.check_call(["g++"] + FLAGS + [src, "-o", exe])
    subprocess.check_call([exe, probe, probe + ".out"])    # whichever build it is must run: a sanitizer report here fails the tests
    return exe, d


def _check(program, sets):
    """-> the verdicts; every set: the same verdict as gauss64 and the same bits of the mean and of C"""
    exe, d = program
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    _records(sets).tofile(src)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.float64).reshape(-1, 10)
    assert len(out) == len(sets)
    for s, o in zip(sets, out):
        mean, C = ndt_ref.gauss64(s)
        assert o[1:4].view(np.uint64).tolist() == mean.view(np.uint64).tolist(), s
        assert (o[0] == 1.0) == (C is not None), s
        if C is None:
            assert not o[4:].any() and not np.signbit(o[4:]).any()
        else:
            assert o[4:].view(np.uint64).tolist() == C.view(np.uint64).tolist(), s
    return out[:, 0] == 1.0


def test_random_member_sets(program):
    rng = np.random.default_rng(20261020)
    sets = []
    for n, scale, off in zip(rng.integers(6, KMAX + 1, 240), 10.0 ** rng.uniform(-2, 2, 240), rng.normal(0, 200, (240, 3))):
        shape = 10.0 ** rng.uniform(-2, 0, 3)          # anisotropic: some axes fall under the floor
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        sets.append(((rng.normal(size=(n, 3)) * shape * scale) @ q + off).astype(np.float32))
    ok = _check(program, sets)
    assert ok.all()


def test_degenerate_sets_and_small_counts(program):
    rng = np.random.default_rng(3)
    base = np.array([170.0, -30.0, 12.5])
    sets, want = [], []
    for n in (2, 3, MIN_POINTS - 1, MIN_POINTS, 17):
        sets.append((rng.normal(size=(n, 3)) + base).astype(np.float32)); want.append(True)               # general position (2: a line; valid, floored)
        sets.append(np.repeat(base[None], n, axis=0).astype(np.float32)); want.append(False)              # identical: void
        t = rng.uniform(-2, 2, n)
        sets.append((base + t[:, None] * [0.5, 0.25, -1.0]).astype(np.float32)); want.append(True)        # collinear (up to fp32 rounding)
        sets.append((base + t[:, None] * [1.0, 0.0, 0.0]).astype(np.float32)); want.append(True)          # collinear along x, exactly
        uv = rng.uniform(-2, 2, (n, 2))
        sets.append((base + np.column_stack([uv, np.zeros(n)])).astype(np.float32)); want.append(True)    # coplanar, exactly
        sets.append((base + uv[:, :1] * [1.0, 2.0, 2.0] + uv[:, 1:] * [2.0, -2.0, 1.0]).astype(np.float32)); want.append(True)   # coplanar, tilted
    sets.append(np.array([[1e30, 0, 0]] * 3 + [[-1e30, 0, 0]] * 3, np.float32)); want.append(True)        # large, finite
    sets.append(np.array([[1e-30, 0, 0]] * 3 + [[-1e-30, 0, 0]] * 3, np.float32)); want.append(True)      # tiny: below Jacobi's absolute threshold
    ok = _check(program, sets)
    assert ok.tolist() == want
    for s, o in zip(sets, ok):                         # a Gaussian's C has a condition number of at most 100
        if o:
            w = np.linalg.eigvalsh(ndt_ref.full(ndt_ref.gauss64(s)[1]))
            assert w[0] > 0 and w[2] / w[0] <= 100.0 * (1 + 1e-6), (s, w)
