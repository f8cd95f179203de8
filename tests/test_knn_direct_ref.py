"""The direct-answer rule that ships (pcreg_amd/csrc/direct_rule.hpp, DESIGN 4.1 "Direct answers"), compiled for the host,
against the restatement of tests/knn_direct_ref.py: the radius bit for bit, the cell ranges and the finiteness verdict exactly.
Then the property the search relies on, over random and adversarial (q, m, dk) triples: whenever the fp32 chain distance of
q and m is <= dk, m's ordering-grid cell lies in q's range on every axis.  The chain distance comes from the same host program
(fmaf, -ffp-contract=off), which is the oracle's arithmetic.  The header is plain C++17 without a HIP include: no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import knn_direct_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = np.inf

SHIM = r"""
#include "direct_rule.hpp"
extern "C" void direct_ranges(const float* q, const float* dk, const float* s0, float inv_s, int top, int n, int* fin, int* lo, int* hi, double* rho) {
    for (int i = 0; i < n; ++i) {
        pcreg::DirectRange r{};
        fin[i] = pcreg::direct_range(q + 3 * i, dk[i], s0, inv_s, top, &r) ? 1 : 0;
        for (int c = 0; c < 3; ++c) { lo[3 * i + c] = fin[i] ? r.lo[c] : 0; hi[3 * i + c] = fin[i] ? r.hi[c] : 0; }
        rho[i] = fin[i] ? pcreg::direct_radius(dk[i]) : 0.0;
    }
}
extern "C" void order_cells(const float* v, const float* s0, float inv_s, int top, int n, int* out) {
    for (int i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) out[3 * i + c] = (int)pcreg::order_cell(v[3 * i + c], s0[c], inv_s, (float)top);
}
extern "C" void chain_d2(const float* q, const float* m, int n, float* d) {
    for (int i = 0; i < n; ++i) {
        const float dx = q[3 * i] - m[3 * i], dy = q[3 * i + 1] - m[3 * i + 1], dz = q[3 * i + 2] - m[3 * i + 2];
        d[i] = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    }
}
extern "C" void caps(int* out) { out[0] = pcreg::kDirectCells; out[1] = pcreg::kDirectRows; }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("direct_rule")
    src, out = str(d / "direct_rule_shim.cpp"), str(d / "libdirect_rule_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "pcreg_amd", "csrc"), src, "-o", out])
    L = C.CDLL(out)
    vp, i = C.c_void_p, C.c_int
    L.direct_ranges.restype = L.order_cells.restype = L.chain_d2.restype = L.caps.restype = None
    L.direct_ranges.argtypes = [vp, vp, vp, C.c_float, i, i, vp, vp, vp, vp]
    L.order_cells.argtypes = [vp, vp, C.c_float, i, i, vp]
    L.chain_d2.argtypes = [vp, vp, i, vp]
    L.caps.argtypes = [vp]
    return L


def _f(a):
    return np.ascontiguousarray(a, F32)


def _ranges(L, q, dk, s0, inv_s, top=ref.TOP):
    q, dk, s0 = _f(q).reshape(-1, 3), _f(dk).reshape(-1), _f(s0)
    n = len(dk)
    fin, lo, hi, rho = np.empty(n, np.int32), np.empty((n, 3), np.int32), np.empty((n, 3), np.int32), np.empty(n, np.float64)
    L.direct_ranges(q.ctypes.data, dk.ctypes.data, s0.ctypes.data, C.c_float(float(inv_s)), top, n, fin.ctypes.data, lo.ctypes.data,
                    hi.ctypes.data, rho.ctypes.data)
    return fin.astype(bool), lo.astype(np.int64), hi.astype(np.int64), rho


def _cells(L, v, s0, inv_s, top=ref.TOP):
    v, s0 = _f(v).reshape(-1, 3), _f(s0)
    out = np.empty((len(v), 3), np.int32)
    L.order_cells(v.ctypes.data, s0.ctypes.data, C.c_float(float(inv_s)), top, len(v), out.ctypes.data)
    return out.astype(np.int64)


def _chain(L, q, m):
    q, m = _f(q).reshape(-1, 3), _f(m).reshape(-1, 3)
    d = np.empty(len(q), F32)
    L.chain_d2(q.ctypes.data, m.ctypes.data, len(q), d.ctypes.data)
    return d


def _same_as_ref(L, q, dk, s0, inv_s):
    """the host program against the restatement, bit for bit -> (fin, lo, hi)"""
    fin, lo, hi, rho = _ranges(L, q, dk, s0, inv_s)
    rfin, rlo, rhi = ref.cell_range(q, dk, s0, inv_s)
    assert fin.tolist() == rfin.tolist()
    assert lo.tolist() == rlo.tolist() and hi.tolist() == rhi.tolist()
    want = np.where(rfin, ref.radius(np.where(rfin, _f(dk).reshape(-1), F32(0))), 0.0)
    assert rho.view(np.uint64).tolist() == want.view(np.uint64).tolist()
    return fin, lo, hi


def _holds(L, q, m, dk, s0, inv_s, need=1):
    """the property on every triple; -> how many triples had chain distance <= dk (at least `need`)"""
    q, m, dk = _f(q).reshape(-1, 3), _f(m).reshape(-1, 3), _f(dk).reshape(-1)
    fin, lo, hi = _same_as_ref(L, q, dk, s0, inv_s)
    with np.errstate(over="ignore", invalid="ignore"):
        d = _chain(L, q, m)
    mc = _cells(L, m, s0, inv_s)
    np.testing.assert_array_equal(mc, np.stack([ref.cell(m[:, c], _f(s0)[c], inv_s) for c in range(3)], axis=1))
    within = fin & (d <= dk)
    inside = np.all((mc >= lo) & (mc <= hi), axis=1)
    bad = np.flatnonzero(within & ~inside)
    assert len(bad) == 0, f"{len(bad)} rows within dk outside the range, first: q {q[bad[0]]!r} m {m[bad[0]]!r} dk {dk[bad[0]]!r}"
    assert within.sum() >= need, "premise: triples within dk"
    return int(within.sum())


def test_the_caps_are_the_restatements(shim):
    out = np.empty(2, np.int32)
    shim.caps(out.ctypes.data)
    assert out.tolist() == [ref.CELLS, ref.ROWS] == [27, 512]


def test_cell_expression_is_monotone(shim):
    rng = np.random.default_rng(5)
    for s0, inv_s in ((0.0, 0.63), (-3.5, 1e-3), (7.0, 0.0), (1e-30, np.float32(np.inf)), (0.0, 3e38), (2.0, 1.1754944e-38)):
        v = np.sort(np.concatenate([rng.normal(0, 50, 3000), rng.normal(s0, 1e-3, 500), [s0, -INF, INF, -3.4e38, 3.4e38, 0.0],
                                    np.nextafter(F32(s0), F32(INF), dtype=F32)[None], (s0 + np.arange(66) / max(inv_s, 1e-30))[:66]]).astype(F32))
        c = ref.cell(v, F32(s0), inv_s)
        assert np.all(np.diff(c) >= 0), (s0, inv_s)
        got = _cells(shim, np.repeat(v[:, None], 3, axis=1), [s0, s0, s0], inv_s)
        assert got[:, 0].tolist() == c.tolist()


def test_random_triples(shim):
    rng = np.random.default_rng(20261020)
    n = 20000
    s0 = np.array([-12.0, 3.0, 40.0], F32)
    inv_s = F32(64.0 / 101.0)
    q = (rng.random((n, 3)) * [110.0, 110.0, 110.0] + s0 - 4.0).astype(F32)
    step = rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-4, 1, (n, 1)))
    m = (q + step).astype(F32)
    d = _chain(shim, q, m)
    # dk around the pair's own distance: below (the row does not count), equal, a few ulps and a few percent above
    k = rng.integers(0, 5, n)
    dk = np.select([k == 0, k == 1, k == 2, k == 3], [np.nextafter(d, F32(0)), d, np.nextafter(d, F32(INF)), d * F32(1.03)], d * F32(0.5)).astype(F32)
    got = _holds(shim, q, m, dk, s0, inv_s, need=n // 2)
    assert got < n, "premise: some triples beyond dk"


def test_row_exactly_at_dk_and_dk_zero(shim):
    rng = np.random.default_rng(7)
    s0, inv_s = np.zeros(3, F32), F32(0.6336)
    q = (rng.random((4000, 3)) * 100.0).astype(F32)
    m = (q + rng.normal(0, 0.7, q.shape)).astype(F32)
    m[:500] = q[:500]                                              # coincident: dk = 0
    m[500:1000, 1:] = q[500:1000, 1:]                              # one axis carries the whole distance
    d = _chain(shim, q, m)
    assert np.all(d[:500] == 0)
    assert _holds(shim, q, m, d, s0, inv_s, need=4000) == 4000
    fin, lo, hi = _same_as_ref(shim, q[:500], d[:500], s0, inv_s)
    assert fin.all() and np.all(hi - lo <= 1), "dk = 0: the range is the query's cell, or two where it sits within rho of a face"


def test_bound_on_a_cell_edge_and_one_ulp_to_either_side(shim):
    """q_c - rho exactly on a cell edge (and q_c + rho), one ulp below and above: the row on the bound's float is found"""
    s0 = np.zeros(3, F32)
    inv_s = F32(0.5)                                               # cells of edge 2: edges at the even numbers
    qs, ms, dks = [], [], []
    for edge in (2.0, 8.0, 30.0, 126.0):
        for dist in (0.25, 0.5, 1.0, 1.75):
            for side in (-1.0, 1.0):
                q0 = F32(edge - side * dist)                       # the bound q + side * dist lies exactly on `edge`
                for wiggle in (-1, 0, 1):
                    qc = q0 if wiggle == 0 else np.nextafter(q0, F32(INF if wiggle > 0 else -INF))
                    for mw in (-1, 0, 1):                          # the row on the edge, one ulp inside the next cell, one ulp before it
                        mc = F32(edge) if mw == 0 else np.nextafter(F32(edge), F32(INF if mw > 0 else -INF))
                        qs.append([qc, 50.0, 50.0]); ms.append([mc, 50.0, 50.0])
                        dks.append(dist * dist)                    # the square of the nominal gap: exact in fp32
    q, m = _f(qs), _f(ms)
    d = _chain(shim, q, m)
    n = len(d)
    # dk = the pair's own distance and one ulp above it: every row counts; one ulp below: none does; the nominal square: some do
    for dk, need, most in ((d, n, n), (np.nextafter(d, F32(INF)), n, n), (np.nextafter(d, F32(0)), 0, 0), (_f(dks), n // 4, n - 1)):
        assert need <= _holds(shim, q, m, dk, s0, inv_s, need=need) <= most
    # the bounds themselves: on the edge the lower bound's cell is the edge's own cell, one ulp below it the cell before
    lo_f, hi_f = ref.bounds(_f([[4.0, 4.0, 4.0]]), _f([1.0]))
    assert lo_f[0, 0] < F32(3.0) < F32(5.0) < hi_f[0, 0], "the slack moves the bounds off the exact q -+ sqrt(dk)"
    assert F32(3.0) - lo_f[0, 0] < 1e-5 and hi_f[0, 0] - F32(5.0) < 1e-5


def test_subnormal_differences(shim):
    tiny = F32(1e-45)
    s0, inv_s = np.zeros(3, F32), F32(0.64)
    base = _f([[1e-38, 0, 0], [0, 0, 0], [3e-39, -2e-39, 1e-39], [2.0, 2.0, 2.0], [1e-20, 1e-20, 1e-20]])
    q = np.repeat(base, 40, axis=0)
    rng = np.random.default_rng(9)
    scale = np.repeat(_f([1e-39, 1e-44, 3e-39, 1e-22, 1e-23]), 40)[:, None]
    m = (q + rng.normal(size=q.shape) * scale).astype(F32)
    m[::5] = q[::5] + tiny
    d = _chain(shim, q, m)
    assert (d == 0).sum() > 40, "premise: squares that underflow to zero"
    assert _holds(shim, q, m, d, s0, inv_s, need=len(q)) == len(q)
    assert _holds(shim, q, m, np.zeros(len(q), F32), s0, inv_s, need=40) > 40
    # across a cell face at a subnormal distance: the face at 0 of an origin that is itself tiny
    s1 = _f([2e-39, 2e-39, 2e-39])
    q2 = _f([[2e-39, 1.0, 1.0]] * 3)
    m2 = _f([[1.9e-39, 1.0, 1.0], [2.1e-39, 1.0, 1.0], [2e-39, 1.0, 1.0]])
    assert _holds(shim, q2, m2, _chain(shim, q2, m2), s1, F32(0.64), need=3) == 3


def test_inv_s_zero_and_the_clamped_ends(shim):
    rng = np.random.default_rng(11)
    q = (rng.random((2000, 3)) * 100.0).astype(F32)
    m = (q + rng.normal(0, 1.0, q.shape)).astype(F32)
    d = _chain(shim, q, m)
    # a model without extent: inv_s = 0, every coordinate falls into cell 0
    fin, lo, hi = _same_as_ref(shim, q, d, np.zeros(3, F32), 0.0)
    assert fin.all() and not lo.any() and not hi.any()
    assert _holds(shim, q, m, d, np.zeros(3, F32), 0.0, need=2000) == 2000
    # queries and rows on and beyond both ends of the grid: cells clamp at 0 and 63
    s0, inv_s = _f([10.0, 10.0, 10.0]), F32(64.0 / 80.0)
    ends = np.concatenate([rng.uniform(5.0, 11.0, (700, 3)), rng.uniform(89.0, 96.0, (700, 3)), rng.uniform(-500.0, 600.0, (600, 3))]).astype(F32)
    me = (ends + rng.normal(0, 1.5, ends.shape)).astype(F32)
    de = _chain(shim, ends, me)
    assert _holds(shim, ends, me, de, s0, inv_s, need=2000) == 2000
    fin, lo, hi = _same_as_ref(shim, ends, de, s0, inv_s)
    assert (lo == 0).any() and (hi == 63).any() and (hi == 0).all(axis=1).any() and (lo == 63).all(axis=1).any()
    # coordinates at the end of fp32 with the largest seed distances: rho (at most 1.9e19) is below half a float64 ulp there,
    # the bounds are the coordinates themselves (no float lies beyond them) and the cells clamp
    fmax = np.finfo(F32).max
    big = _f([[fmax, -fmax, 0.0]])
    fin, lo, hi = _same_as_ref(shim, big, _f([3.0e38]), s0, inv_s)
    assert fin.all() and lo[0].tolist() == [63, 0, 0] and hi[0].tolist() == [63, 0, 63]
    lo_f, hi_f = ref.bounds(big, _f([3.0e38]))
    assert hi_f[0, 0] == fmax and lo_f[0, 1] == -fmax and lo_f[0, 2] < -1e19 and hi_f[0, 2] > 1e19


def test_not_finite_is_not_eligible(shim):
    q = _f([[1, 2, 3], [np.nan, 2, 3], [1, INF, 3], [1, 2, -INF], [1, 2, 3], [1, 2, 3], [1, 2, 3]])
    dk = _f([1.0, 1.0, 1.0, 1.0, INF, np.nan, -1.0])
    fin, lo, hi = _same_as_ref(shim, q, dk, np.zeros(3, F32), F32(0.5))
    assert fin.tolist() == [True, False, False, False, False, False, False]


def test_eligibility_counts_cells_and_rows():
    """ref.eligible on a hand-made grid: 4 x 4 x 4 cells of edge 1, known occupancies"""
    rows = np.array([[0.5, 0.5, 0.5]] * 600 + [[1.5, 0.5, 0.5]] * 3 + [[3.5, 3.5, 3.5]] * 2, F32)
    e = ref.eligible(_f([[1.5, 0.5, 0.5], [1.5, 0.5, 0.5], [3.5, 3.5, 3.5], [2.0, 2.0, 2.0], [np.nan, 0, 0]]), _f([0.01, 0.36, 0.01, 2.0, 0.01]),
                     rows, np.zeros(3, F32), 1.0, top=3)
    assert e["cells"].tolist() == [1, 3 * 2 * 2, 1, 64, 1]
    assert e["rows"].tolist() == [3, 603, 2, -1, -1]
    assert e["ok"].tolist() == [True, False, True, False, False]
