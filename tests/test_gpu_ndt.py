"""The normal-distributions transform on the GPU (ndt.hip + ndt_gauss.hpp + plane_fit.hpp) against tests/ndt_ref.py.

THE TABLE: cells, counts and the means' bits; C bit for bit against gauss64 (the float64 restatement of ndt_gauss.hpp) and within
BOUND_C of the longdouble reference; a 40-row cloud of voxels with exactly 5 and 6 rows, six identical rows, six collinear rows
and NaN rows; the 2^21 refusal; n = 0.
THE STEP: n_pairs exactly; T_out bit for bit the restated product of T and the T_step the device reports; T_step within BOUND of
the reference (the 28 sums and the scaled Cholesky in longdouble) where the reference's smallest pivot is at least PIVOT; sum_e
within 1e-12 relative; the same bits twice and on two streams (the launcher has no batching).  The pair rule on a grid with exact
boundaries; exactly 5 and 6 pairs across the chunk boundary; Q = 0, B = 0 and a table without Gaussians with a canary behind the
stated workspace; every argument error; three steps at both tiers and step by step against the reference; five NDT steps against
five point-to-point steps; refine_trials(ndt=).

BOUND, 1e-9 in the Frobenius norm, is tests/test_gpu_refit_plane.py's in the same role: the same solve on the same scene, about
170 units from the coordinate origin.  BOUND_C is 100 times the worst |C - C_ref|_F / |C_ref|_F that gauss64 -- whose bits the
device must give -- shows over the main scene's 124 Gaussians, 1.644e-15 (tests/test_ndt_ref.py prints it), and not below 1e-13;
the floor of the eigenvalues bounds every C's condition number by 100, so other clouds sit in the same range."""
import ctypes as C

import numpy as np
import pytest
import torch

import ndt_ref
import plane_ref
import refit_ref
from test_gpu_range import _dev, _soa
from test_gpu_refit import _m44, _same, _t16

pytestmark = pytest.mark.gpu
BOUND = 1e-9
BOUND_C = max(100 * 1.644e-15, 1e-13)
PIVOT = 1e-2
STEP = 4.0
E_ARG = 1


def _model(pts, step, min_points=6):
    from pcreg_amd.device import NdtModel
    return NdtModel(_soa(pts), step, min_points)


def _refit(nm, q, Td, neighbors=1, outlier_ratio=0.55, steps=1, out=None):
    """-> T_out [B, 4, 4], T_step [B, 4, 4], n_pairs, sum_e, empty as numpy"""
    got = nm.refit(q, Td, neighbors=neighbors, outlier_ratio=outlier_ratio, steps=steps, out=out)
    torch.cuda.synchronize()
    T_out, T_step, n, s, e = (t.cpu().numpy() for t in got)
    return _m44(T_out), _m44(T_step), n, s, e


def _check(got, T, want, what=""):
    """one call against ndt_ref.step on the bits of T that the device was given -> the worst |T_step - reference|"""
    T_out, T_step, n, s, e = got
    np.testing.assert_array_equal(n, want["n_pairs"])
    np.testing.assert_array_equal(e != 0, want["empty"])
    assert set(np.unique(e).tolist()) <= {0, 1}
    worst = 0.0
    for b in range(len(T)):
        rel = abs(s[b] - want["sum_e"][b]) / want["sum_e"][b] if want["sum_e"][b] else abs(s[b])
        assert rel <= 1e-12, (what, b, s[b], want["sum_e"][b])
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any(), b              # all 32 numbers are 0.0
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        assert want["pivot"][b] >= PIVOT, (what, b, want["pivot"][b])         # the premise of the bound
        err = float(np.linalg.norm(T_step[b] - want["T_step"][b]))
        print(f"  {what} b = {b}: n_pairs {n[b]}, |T_step - reference| = {err:.3e} ({err / BOUND:.1e} of the bound), sum_e off by {rel:.1e} "
              f"({rel / 1e-12:.1e} of the bound), smallest pivot {want['pivot'][b]:.3f}")
        assert err < BOUND, (what, b, err)
        worst = max(worst, err)
    return worst


def _table_is(nm, tab):
    """the device's table against the reference's: everything to the bit, C also against the longdouble reference"""
    g = nm.gaussians()
    assert nm.n_voxels == tab["n_voxels"] and nm.n_gaussians == len(tab["cells"])
    np.testing.assert_array_equal(g["cells"], tab["cells"])
    np.testing.assert_array_equal(g["counts"], tab["counts"])
    np.testing.assert_array_equal(g["lo"].view(np.uint32), tab["lo"].view(np.uint32))
    np.testing.assert_array_equal(g["origin"].view(np.uint32), tab["origin"].view(np.uint32))
    np.testing.assert_array_equal(g["means"].view(np.uint64), tab["means"].view(np.uint64))
    np.testing.assert_array_equal(g["C"].view(np.uint64), tab["C"].view(np.uint64))
    if not len(tab["cells"]):
        return 0.0
    w = np.array([1, 2 ** 0.5, 2 ** 0.5, 1, 2 ** 0.5, 1])                          # the Frobenius norm of the symmetric matrix
    rel = np.linalg.norm((g["C"].astype(ndt_ref.LD) - tab["C_ref"]).astype(np.float64) * w, axis=1) / np.linalg.norm(tab["C_ref"].astype(np.float64) * w, axis=1)
    print(f"worst |C - C_ref|_F / |C_ref|_F over {len(rel)} Gaussians: {rel.max():.3e} ({rel.max() / BOUND_C:.1e} of the bound)")
    assert rel.max() <= BOUND_C
    return float(rel.max())


@pytest.fixture(scope="module")
def main():
    sc = plane_ref.scene()
    tab = ndt_ref.table(sc["model"], STEP, 6)
    nm = _model(sc["model"], STEP)
    yield sc, tab, nm
    nm.close()


# ---------------------------------------------------------------------------------------------------------------- the table
def test_the_main_scenes_table(main):
    sc, tab, nm = main
    assert tab["n_voxels"] == 131 and len(tab["cells"]) == 124                     # the premise (tests/test_ndt_ref.py)
    _table_is(nm, tab)


def small_cloud():
    """40 rows at step 1 with lo = (0, 0, 0): voxel (0,0,0) 1 row (pins lo), (1,0,0) exactly 5 rows, (2,0,0) exactly 6 rows, (3,0,0) six
    identical rows, (4,0,0) six collinear rows, (5,0,0) 7 rows in general position, 9 rows with a NaN or an infinite coordinate,
    shuffled"""
    rng = np.random.default_rng(17)
    gen = lambda c, n: np.array([c, 0, 0]) + rng.integers(8, 56, (n, 3)) / 64.0
    line = np.array([4, 0, 0]) + 0.125 + np.arange(6)[:, None] * np.array([0.125, 0.0625, 0.03125])
    dead = gen(2, 9)
    dead[np.arange(9), rng.integers(0, 3, 9)] = [np.nan, np.inf, -np.inf] * 3
    rows = np.vstack([np.zeros((1, 3)), gen(1, 5), gen(2, 6), np.repeat(gen(3, 1), 6, axis=0), line, gen(5, 7), dead])
    assert len(rows) == 40
    return rows[rng.permutation(40)].astype(np.float32)


def test_a_small_cloud_of_edge_voxels():
    pts = small_cloud()
    tab = ndt_ref.table(pts, 1.0, 6)
    assert tab["n_voxels"] == 6 and tab["voxel_counts"].tolist() == [1, 5, 6, 6, 6, 7]               # premises: the NaN rows are in no voxel
    assert tab["cells"].tolist() == [[2, 0, 0], [4, 0, 0], [5, 0, 0]] and tab["counts"].tolist() == [6, 6, 7]
    nm = _model(pts, 1.0)
    try:
        _table_is(nm, tab)
    finally:
        nm.close()
    nm = _model(pts, 1.0, min_points=5)                                                              # the voxel of 5 rows joins
    try:
        tab5 = ndt_ref.table(pts, 1.0, 5)
        assert tab5["cells"][:, 0].tolist() == [1, 2, 4, 5]
        _table_is(nm, tab5)
    finally:
        nm.close()


def test_a_cloud_of_two_to_the_21_cells_is_refused_and_one_cell_less_is_not():
    from pcreg_amd._lib import PcregError
    ok = np.array([[0, 0, 0], [0, 2 ** 21 - 0.5, 0]], np.float32)                                    # cells 0 .. 2^21 - 1 along y
    nm = _model(ok, 1.0, 3)
    try:
        assert (nm.n_voxels, nm.n_gaussians) == (2, 0)
    finally:
        nm.close()
    with pytest.raises(PcregError) as e:
        _model(np.array([[0, 0, 0], [0, 2 ** 21, 0]], np.float32), 1.0, 3)
    assert e.value.code == E_ARG


def test_an_empty_cloud_and_a_cloud_without_live_rows():
    for pts in (np.zeros((0, 3), np.float32), np.full((7, 3), np.nan, np.float32)):
        nm = _model(pts, 1.0)
        try:
            assert (nm.n_voxels, nm.n_gaussians) == (0, 0)
            g = nm.gaussians()
            assert g["cells"].shape == (0, 3) and not g["lo"].any() and not g["origin"].any()
            got = _refit(nm, _soa(np.ones((5, 3))), _t16(np.eye(4)[None]), 7)
            assert got[4].tolist() == [1] and got[2].tolist() == [0] and got[3].tolist() == [0.0] and not got[0].any() and not got[1].any()
        finally:
            nm.close()


# ----------------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("neighbors", [1, 7])
def test_the_step_on_the_main_scene(main, neighbors):
    sc, tab, nm = main
    surf, T = sc["surf"], sc["T"]
    q, Td = _soa(surf), _t16(T)
    want = ndt_ref.step(surf, tab, T, neighbors)
    got = _refit(nm, q, Td, neighbors)
    worst = _check(got, T, want, f"neighbors = {neighbors}")
    print(f"neighbors = {neighbors}: n_pairs {got[2].tolist()}, empty {got[4].tolist()}, worst |T_step - reference| {worst:.3e} = {worst / BOUND:.1e} of the bound")
    assert got[4].tolist() == [0, 0, 0, 0, 1, 1]
    _same(_refit(nm, q, Td, neighbors), got)                                                         # twice
    # the unweighted form and another ratio
    for ratio in (0.0, 0.2):
        _check(_refit(nm, q, Td, neighbors, ratio), T, ndt_ref.step(surf, tab, T, neighbors, ratio), f"neighbors = {neighbors}, ratio = {ratio}")


def test_two_streams_on_one_handle(main):
    """each call with its own workspace and outputs; the dirty workspaces change nothing"""
    from pcreg_amd._lib import lib
    L = lib()
    sc, tab, nm = main
    q, Td = _soa(sc["surf"]), _t16(sc["T"])
    halves = ((q[:, :2000].contiguous(), Td[:4].contiguous(), 1), (q[:, 400:].contiguous(), Td[2:].contiguous(), 7))
    want = []
    for a, b, nb in halves:
        out = nm.refit(a, b, neighbors=nb, steps=2)
        torch.cuda.synchronize()
        want.append(tuple(t.cpu().numpy() for t in out))
    outs = []
    for a, b, nb in halves:
        Qh, Bh = a.shape[1], b.shape[0]
        d64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=_dev())
        i32 = lambda: torch.full((Bh,), -7, dtype=torch.int32, device=_dev())
        outs.append((d64(Bh, 16), d64(Bh, 16), i32(), d64(Bh), i32(),
                     torch.full((int(L.pcreg_dev_ndt_refit_workspace(Qh, Bh)),), 0xA5, dtype=torch.uint8, device=_dev()), d64(Bh, 16)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        for s, (a, b, nb), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
            with torch.cuda.stream(s):
                nm.refit(a, b, neighbors=nb, steps=2, out=o)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        _same(tuple(t.cpu().numpy() for t in o[:5]), w)


def pair_rule_scene():
    """step 0.5 and lo = (0, 0, 0), so every boundary is exact.  Gaussian voxels A = (1,1,1), B = (3,1,1) and D = (1,0,1), 8 rows each on
    multiples of 1/64; the occupied voxel (2,1,1) has 2 rows and (0,0,0) one, which pins lo.  The last cell along x is 3."""
    rng = np.random.default_rng(23)
    vox = lambda c, n: (np.array(c) * 0.5 + rng.integers(2, 30, (n, 3)) / 64.0)
    model = np.vstack([np.zeros((1, 3)), vox((1, 1, 1), 8), vox((3, 1, 1), 8), vox((1, 0, 1), 8), vox((2, 1, 1), 2)]).astype(np.float32)
    queries = [
        ((0.75, 0.75, 0.75), 1, 2),      # inside A: itself; with 7 also D below it (-y)
        ((0.5, 0.75, 0.75), 1, 2),       # exactly on A's lower x boundary: the upper cell, A (and D)
        ((1.0, 0.75, 0.75), 0, 2),       # exactly on the boundary of cells 1 and 2: cell 2, not a Gaussian; its -x and +x neighbours are A and B
        ((1.25, 0.75, 0.75), 0, 2),      # inside the occupied non-Gaussian voxel (2,1,1)
        ((0.75, -0.25, 0.75), 0, 1),     # cell -1 along y: its own cell is out of range, its +y neighbour is D
        ((2.25, 0.75, 0.75), 0, 1),      # cell 4, past the last cell: no such voxel, its -x neighbour is B
        ((0.75, 0.75, 1.0), 0, 1),       # exactly on A's upper z boundary: cell (1,1,2), its -z neighbour is A
        ((np.nan, 0.75, 0.75), 0, 0),    # a non-finite coordinate: no pair
        ((0.75, np.inf, 0.75), 0, 0),
        ((9.0, 9.0, 9.0), 0, 0),         # far off
    ]
    return model, queries


def test_the_pair_rule_on_exact_boundaries():
    model, queries = pair_rule_scene()
    tab = ndt_ref.table(model, 0.5, 6)
    assert tab["cells"].tolist() == [[1, 0, 1], [1, 1, 1], [3, 1, 1]] and tab["n_voxels"] == 5 and not tab["lo"].any()      # premises
    q_all = np.array([p for p, _a, _b in queries], np.float32)
    nan_T = np.eye(4); nan_T[3, 0] = np.nan
    T = np.stack([np.eye(4), np.zeros((4, 4)), nan_T])
    nm = _model(model, 0.5)
    try:
        _table_is(nm, tab)
        for nb in (1, 7):
            for i, (p, n1, n7) in enumerate(queries):                                                # one query at a time: its own pairs
                got = _refit(nm, _soa(q_all[i:i + 1]), _t16(T), nb)
                want = ndt_ref.step(q_all[i:i + 1], tab, T, nb)
                assert got[2].tolist() == [n1 if nb == 1 else n7, 0, 0] == want["n_pairs"].tolist(), (p, nb, got[2])
                assert got[4].tolist() == [1, 1, 1]
            got = _refit(nm, _soa(q_all), _t16(T), nb)                                               # all at once
            _check(got, T, ndt_ref.step(q_all, tab, T, nb), f"pair rule, neighbors = {nb}")
            assert got[2].tolist() == [sum(q[1 if nb == 1 else 2] for q in queries), 0, 0]
    finally:
        nm.close()


def few_pairs_scene(k):
    """a model of 6000 rows in [0, 8)^3 -- 64 voxels of step 2, every one a Gaussian -- and 2500 queries far outside the grid except
    exactly k inside it; two of the k are queries 2047 and 2048, on both sides of the chunk boundary"""
    rng = np.random.default_rng(80 + k)
    model = rng.uniform(0, 8, (6000, 3)).astype(np.float32)
    surf = (rng.uniform(0, 8, (2500, 3)) + 100.0).astype(np.float32)
    at = sorted([2047, 2048] + rng.choice(2000, k - 2, replace=False).tolist())
    surf[at] = rng.uniform(1, 7, (k, 3)).astype(np.float32)
    return model, surf, at


@pytest.mark.parametrize("k", [5, 6])
def test_exactly_k_pairs_across_the_chunk_boundary(k):
    model, surf, at = few_pairs_scene(k)
    tab = ndt_ref.table(model, 2.0, 6)
    T = np.eye(4)[None]
    want = ndt_ref.step(surf, tab, T, 1)
    assert len(tab["cells"]) == 64 and want["n_pairs"].tolist() == [k] and want["empty"].tolist() == [k < 6]            # premises
    assert ndt_ref.pairs(tab, surf, 1)[0].tolist() == at
    nm = _model(model, 2.0)
    try:
        _check(_refit(nm, _soa(surf), _t16(T), 1), T, want, f"k = {k}")
    finally:
        nm.close()


def _raw(nm, q, Q, ldq, Td, B, neighbors, ratio, outs, ws, ws_bytes, handle=None):
    from pcreg_amd._lib import lib
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    T_out, T_step, n, s, e = outs
    return lib().pcreg_dev_ndt_refit_f32(nm.handle if handle is None else handle, ptr(q), Q, ldq, ptr(Td), B, neighbors, ratio, ptr(T_out), ptr(T_step),
                                         ptr(n), ptr(s), ptr(e), ptr(ws), C.c_size_t(ws_bytes), None)


def _outs(B):
    return (torch.full((max(B, 1), 16), -7.0, dtype=torch.float64, device=_dev()), torch.full((max(B, 1), 16), -7.0, dtype=torch.float64, device=_dev()),
            torch.full((max(B, 1),), -7, dtype=torch.int32, device=_dev()), torch.full((max(B, 1),), -7.0, dtype=torch.float64, device=_dev()),
            torch.full((max(B, 1),), -7, dtype=torch.int32, device=_dev()))


def test_the_edges_keep_inside_the_stated_workspace(main):
    from pcreg_amd._lib import lib
    L = lib()
    sc, tab, nm = main
    rng = np.random.default_rng(9)
    sparse = _model(rng.uniform(0, 100, (200, 3)).astype(np.float32), 4.0)                            # no voxel holds six rows
    tail = 4096
    try:
        assert sparse.n_voxels > 100 and sparse.n_gaussians == 0
        q = _soa(sc["surf"])
        Q = q.shape[1]
        for h, Qc, B in ((nm, 0, 6), (nm, Q, 0), (sparse, Q, 5000), (sparse, 0, 3)):
            Td = torch.eye(4, dtype=torch.float64, device=_dev()).reshape(1, 16).repeat(max(B, 1), 1).contiguous()
            need = int(L.pcreg_dev_ndt_refit_workspace(Qc, B))
            P = B * max((Qc + 2047) // 2048, 1)
            assert need == (224 * P + 255) // 256 * 256 + (4 * P + 255) // 256 * 256                 # the header's formula
            ws = torch.full((need + tail,), 0x5A, dtype=torch.uint8, device=_dev())
            outs = _outs(B)
            assert _raw(h, q if Qc else None, Qc, max(Qc, 1), Td, B, 7, 0.55, outs, ws, need) == 0
            torch.cuda.synchronize()
            assert bool((ws[need:] == 0x5A).all()), (Qc, B)
            T_out, T_step, n, s, e = outs
            if B == 0:                                                                               # nothing is written
                assert bool((T_out == -7.0).all()) and e.tolist() == [-7] and n.tolist() == [-7]
            else:
                assert e.tolist() == [1] * B and n.tolist() == [0] * B and s.tolist() == [0.0] * B and not T_out.any() and not T_step.any()
    finally:
        sparse.close()


def test_every_argument_error(main):
    from pcreg_amd._lib import PcregError, lib
    L = lib()
    sc, tab, nm = main
    q, Td = _soa(sc["surf"]), _t16(sc["T"])
    Q, B = q.shape[1], Td.shape[0]
    need = int(L.pcreg_dev_ndt_refit_workspace(Q, B))
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    o = _outs(B)
    assert _raw(nm, q, Q, Q, Td, B, 1, 0.55, o, ws, need) == 0                                       # the call the cases below spoil
    bad = [dict(neighbors=0), dict(neighbors=2), dict(neighbors=27), dict(ratio=1.0), dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio=float("inf")),
           dict(Q=-1), dict(B=-1), dict(ldq=Q - 1), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1), dict(ws_bytes=need - 1), dict(ws=None), dict(q=None),
           dict(Td=None), dict(handle=C.c_void_p()), dict(outs=(Td,) + o[1:]),
           dict(outs=(None,) + o[1:]), dict(outs=o[:2] + (None,) + o[3:]), dict(outs=o[:3] + (None,) + o[4:]), dict(outs=o[:4] + (None,))]
    for case in bad:
        a = dict(q=q, Q=Q, ldq=Q, Td=Td, B=B, neighbors=1, ratio=0.55, outs=o, ws=ws, ws_bytes=need, handle=None)
        a.update(case)
        rc = _raw(nm, a["q"], a["Q"], a["ldq"], a["Td"], a["B"], a["neighbors"], a["ratio"], a["outs"], a["ws"], a["ws_bytes"], a["handle"])
        assert rc == E_ARG, (case, rc)
    assert _raw(nm, q, Q, Q, Td, B, 1, 0.55, o[:1] + (None,) + o[2:], ws, need) == 0                 # T_step is optional
    assert L.pcreg_dev_ndt_refit_workspace(-1, 1) == 0 and L.pcreg_dev_ndt_refit_workspace(1, -1) == 0
    torch.cuda.synchronize()
    pts = _soa(sc["model"][:100])
    h = C.c_void_p()
    for args in ((pts.data_ptr(), 100, 100, 0.0, 6), (pts.data_ptr(), 100, 100, float("nan"), 6), (pts.data_ptr(), 100, 100, float("inf"), 6),
                 (pts.data_ptr(), 100, 100, -1.0, 6), (pts.data_ptr(), 100, 100, 4.0, 2), (pts.data_ptr(), 100, 99, 4.0, 6), (pts.data_ptr(), -1, 100, 4.0, 6),
                 (None, 100, 100, 4.0, 6)):
        assert L.pcreg_dev_ndt_create(args[0], args[1], args[2], args[3], args[4], None, C.byref(h)) == E_ARG and not h.value, args
    assert L.pcreg_dev_ndt_create(pts.data_ptr(), 100, 100, 4.0, 6, None, None) == E_ARG
    for kw in (dict(neighbors=3), dict(outlier_ratio=1.0), dict(steps=0)):
        with pytest.raises(ValueError):
            nm.refit(q, Td, **kw)
    with pytest.raises((PcregError, ValueError)):
        _model(sc["model"], 0.0)


def test_three_steps_on_the_device_at_the_host_tier_and_against_the_reference(main):
    import pcreg_amd as pc
    sc, tab, nm = main
    surf, T = sc["surf"], sc["T"]
    q, Td = _soa(surf), _t16(T)
    for nb in (1, 7):
        three = _refit(nm, q, Td, nb, steps=3)
        cur, singles = Td, []
        for k in range(3):
            out = nm.refit(q, cur, neighbors=nb)
            cur = out[0].clone()                                           # fed back on the device
            torch.cuda.synchronize()
            singles.append(tuple(t.cpu().numpy() for t in out))
        last = singles[-1]
        _same(three, (_m44(last[0]), _m44(last[1])) + last[2:])
        with pc.NdtModel(sc["model"], STEP) as h:
            assert (h.n_voxels, h.n_gaussians) == (nm.n_voxels, nm.n_gaussians)
            a, b = h.gaussians(), nm.gaussians()
            _same(tuple(a[key] for key in sorted(a)), tuple(b[key] for key in sorted(b)))
            r = h.refit(surf, T, neighbors=nb, steps=3)
            _same((r["T"], r["n_pairs"], r["sum_e"], r["empty"]), (three[0], three[2], three[3], three[4] != 0))
        T_in = T
        for k in range(3):                                                 # every step against the reference on the bits the device gave that step
            got = (_m44(singles[k][0]), _m44(singles[k][1])) + singles[k][2:]
            worst = _check(got, T_in, ndt_ref.step(surf, tab, T_in, nb), f"neighbors = {nb}, step {k + 1}")
            print(f"neighbors = {nb}, step {k + 1}: n_pairs {got[2].tolist()}, worst |T_step - reference| {worst:.3e}")
            T_in = got[0]
        assert (singles[2][4] == [0, 0, 0, 0, 1, 1]).all()                 # a failed candidate stays failed


def test_five_ndt_steps_against_five_point_to_point_steps(main):
    """what the feature is for: from the largest perturbation, the RMS distance of the moved surface from its true place.  The
    references give 0.017 against 0.49 (tests/test_ndt_ref.py)."""
    from pcreg_amd.device import PreparedModel
    sc, tab, nm = main
    surf, T, cloud = sc["surf"], sc["T"][3:4], sc["cloud"]
    q, Td = _soa(surf), _t16(T)
    ndt = _refit(nm, q, Td, 1, steps=5)
    m = _soa(sc["model"])
    pm = PreparedModel(m)
    try:
        point = pm.refit_transforms(q, Td, float(np.float32(1.5) ** 2), steps=5)
        torch.cuda.synchronize()
        assert ndt[4].tolist() == [0] and point[4].cpu().tolist() == [0]
        a = plane_ref.rms_to_truth(surf, ndt[0][0], cloud)
        b = plane_ref.rms_to_truth(surf, _m44(point[0].cpu().numpy())[0], cloud)
        print(f"RMS distance from the truth: start {plane_ref.rms_to_truth(surf, T[0], cloud):.4f}, five NDT steps {a:.4f}, five point-to-point steps {b:.4f}")
        assert a <= b / 4.0
    finally:
        pm.close()


def test_refine_trials_with_an_ndt_table_keeps_the_orientation_and_the_failed_trial(main):
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials
    sc, tab, nm = main
    surf, T = sc["surf"], sc["T"]
    q = _soa(surf)
    result = dict(trial=np.array([4, 9, 11]), transforms=[pc.invertTF(T[1]), None, pc.invertTF(T[3])])
    inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
    direct = _refit(nm, q, _t16(inv), 7, 0.3, steps=2)
    out, summary = refine_trials(result, None, q, None, steps=2, ndt=nm, neighbors=7, outlier_ratio=0.3)
    assert len(out) == 3 and out[1] is None and direct[4].tolist() == [0, 1, 0]
    for t in (0, 2):
        np.testing.assert_array_equal(out[t], pc.invertTF(direct[0][t]))
    np.testing.assert_array_equal(summary["n_pairs"], direct[2])
    np.testing.assert_array_equal(summary["sum_e"].view(np.uint64), direct[3].view(np.uint64))
    assert refine_trials(dict(trial=[], transforms=[]), None, q, None, ndt=nm)[0] == []
