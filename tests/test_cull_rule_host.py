"""The culling rule that ships (pcreg_amd/csrc/cull_rule.hpp), compiled for the host, against the float64
restatement of tests/knn_cull_ref.py: G2 bit for bit, the verdict exactly.  The header is plain C++17 without a HIP include, so
this needs no GPU; the device sites call the same two functions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import knn_cull_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
INF = np.inf

SHIM = r"""
#include "cull_rule.hpp"
// pair i: tile box t[6 i ..] (lo xyz, hi xyz) against block box b[6 i ..], bound D[i]; the block side as floats, or converted first
extern "C" void cull_rule_pairs(const float* t, const float* b, const float* D, int n, int block_as_double, double* g2, int* skips) {
    for (int i = 0; i < n; ++i) {
        const float *tb = t + 6 * i, *bb = b + 6 * i;
        if (block_as_double) {
            const double lo[3] = {bb[0], bb[1], bb[2]}, hi[3] = {bb[3], bb[4], bb[5]};
            g2[i] = pcreg::cull_gap2(tb, tb + 3, lo, hi);
        } else {
            g2[i] = pcreg::cull_gap2(tb, tb + 3, bb, bb + 3);
        }
        skips[i] = pcreg::cull_skips(g2[i], D[i]) ? 1 : 0;
    }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("cull_rule")
    src, out = str(d / "cull_rule_shim.cpp"), str(d / "libcull_rule_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "pcreg_amd", "csrc"), src, "-o", out])
    L = C.CDLL(out)
    L.cull_rule_pairs.restype = None
    L.cull_rule_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _host(L, tile, block, D, as_double):
    tile = np.ascontiguousarray(tile, np.float32).reshape(-1, 6)
    block = np.ascontiguousarray(block, np.float32).reshape(-1, 6)
    D = np.ascontiguousarray(D, np.float32)
    n = len(D)
    assert tile.shape == block.shape == (n, 6)
    g2, sk = np.empty(n, np.float64), np.empty(n, np.int32)
    L.cull_rule_pairs(tile.ctypes.data, block.ctypes.data, D.ctypes.data, n, int(as_double), g2.ctypes.data, sk.ctypes.data)
    return g2, sk.astype(bool)


def _ref(tile, block, D):
    """pairwise: the diagonal of knn_cull_ref's [blocks, tiles] tables, 64 pairs at a time"""
    tile = np.asarray(tile, np.float32).reshape(-1, 6)
    block = np.asarray(block, np.float32).reshape(-1, 6)
    g2 = np.concatenate([np.diag(ref.gap2(block[s:s + 64, :3], block[s:s + 64, 3:], tile[s:s + 64])) for s in range(0, len(tile), 64)])
    return g2, ref.skip(g2, np.asarray(D, np.float32).astype(np.float64))


def _check(L, tile, block, D):
    g2r, skr = _ref(tile, block, D)
    for as_double in (0, 1):
        g2, sk = _host(L, tile, block, D, as_double)
        assert g2.view(np.uint64).tolist() == g2r.view(np.uint64).tolist()
        assert sk.tolist() == skr.tolist()
    return g2r, skr


def test_the_hand_made_boxes(shim):
    a = 32769 / 65536
    window = 0.25 * (1 - 32 * U)
    origin = [0, 0, 0, 0, 0, 0]                                     # a point box: lo == hi
    cases = [                                                       # (tile box, block box, D, skipped)
        ([0.5, -1, -1, 1, 1, 1], origin, 0.25, False),              # G2 == D: the strict '>' keeps it
        ([a, 0, 0, 2, 1, 1], origin, np.float32(a * a), False),     # D = fl32(G2) < G2, inside the 32u window
        ([0.5, 0, 0, 1, 1, 1], origin, np.nextafter(np.float32(window), np.float32(0)), True),   # just below the window
        ([0.5, 0, 0, 1, 1, 1], origin, np.float32(window), False),  # on the window's lower end
        ([5e-16, 0, 0, 1, 1, 1], origin, 0.0, False),               # G2 = 2.5e-31 <= 1e-30: no bound
        ([2e-15, 0, 0, 1, 1, 1], origin, 0.0, True),
        ([0.5, 0.5, 0.5, 0.5, 0.5, 0.5], origin, 0.5, True),        # point against point: G2 = 0.75
        ([0.5, 0.5, 0.5, 0.5, 0.5, 0.5], origin, 0.75, False),
        ([INF, INF, INF, -INF, -INF, -INF], [-1, -1, -1, 1, 1, 1], 3.0e38, True),    # an empty unit box: infinite gaps
        ([INF, INF, INF, -INF, -INF, -INF], origin, 0.0, True),
        ([2, 0, 0, 3, 1, 1], [-1, -1, -1, 1, 1, 1], 0.0, True),     # D = 0: any gap above the guard skips
        ([1, 0, 0, 3, 1, 1], [-1, -1, -1, 1, 1, 1], 0.0, False),    # ... boxes that touch do not
        ([-3, -3, -3, -2, -2, -2], [-1, -1, -1, 1, 1, 1], 3.0, False),                # the block above the tile: G2 = 3 == D
        ([-3, -3, -3, -2, -2, -2], [-1, -1, -1, 1, 1, 1], 2.9999, True),
    ]
    tile, block = [c[0] for c in cases], [c[1] for c in cases]
    D = np.array([c[2] for c in cases], np.float32)
    g2, sk = _check(shim, tile, block, D)
    assert sk.tolist() == [c[3] for c in cases]
    assert g2[0] == 0.25 and g2[1] == a * a and 0.0 < g2[4] <= 1e-30 < g2[5] and g2[6] == 0.75 and g2[8] == INF and g2[11] == 0.0


def test_random_boxes_with_d_around_the_window(shim):
    rng = np.random.default_rng(20261018)
    n = 4096
    scale = 2.0 ** rng.integers(-40, 40, (n, 1))                    # magnitudes across the exponent range, finite in fp32
    def boxes():
        a, b = rng.normal(size=(n, 3)) * scale, rng.normal(size=(n, 3)) * scale
        return np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1).astype(np.float32)
    tile, block = boxes(), boxes()
    tile[::7, 3:] = tile[::7, :3]                                   # some points, some boxes that overlap on an axis
    block[::5, 3:] = block[::5, :3]
    block[::11, 0] = tile[::11, 0]; block[::11, 3] = tile[::11, 3]
    assert np.isfinite(tile).all() and np.isfinite(block).all()
    g2, _ = _ref(tile, block, np.zeros(n, np.float32))
    with np.errstate(over="ignore"):
        D = (g2 * (1 - 32 * U)).astype(np.float32)                  # the window's lower end, rounded to fp32 ...
    steps = rng.integers(-4, 5, n)                                  # ... and up to four fp32 ulps to either side
    for k in range(1, 5):
        D = np.where(steps >= k, np.nextafter(D, np.float32(INF)), D)
        D = np.where(steps <= -k, np.nextafter(D, np.float32(0)), D)
    D = np.where(np.isfinite(D), D, np.float32(3.0e38)).astype(np.float32)        # the callers' precondition: a finite D
    _, sk = _check(shim, tile, block, D)
    assert 0.2 * n < sk.sum() < 0.8 * n                             # both verdicts are exercised
