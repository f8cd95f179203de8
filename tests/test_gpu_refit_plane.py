"""Candidate transforms refitted by the point-to-plane step (knn_score.hip + plane_fit.hpp) on the GPU.

n_close and the bits of sum_d2 against score_transforms on the same inputs; n_plane, empty, T_step and sum_res2 against
tests/plane_ref.py (score_ref's pairs, the 28 sums and the scaled Cholesky in longdouble, the composition restated entry by
entry); the same bits twice, with culling off and in three batches; the sign of the normals and NaN normals; exactly k = 0 .. 7
plane pairs, two of them across the chunk boundary; flat and parallel models; the edges and the argument errors; three steps on
the device, at the host tier and against the reference step by step; normals computed on the device chained into the refit;
five plane steps against five point-to-point steps; refine_trials; two streams on one handle.

The bound on T_step, 1e-9 in the Frobenius norm, is tests/test_gpu_refit.py's BOUND in the same role.  It is asserted only where
the smallest pivot of the reference's scaled matrix is at least 1e-2 (asserted as the premise; tests/test_plane_ref.py shows it
for the main scene without a GPU): a nearly unconstrained direction is ill-conditioned in any arithmetic.  The worst measured
value on the main scene is 2.6e-14 (r = 1.5 and +inf; 2.0e-14 at r = 0.5), 2.6e-5 of the bound: the rounding of o + t in
T_step's last column at coordinates near 170, where half an ulp is 1.4e-14.  sum_res2 is held to 1e-12 relative."""
import os

import numpy as np
import pytest
import torch

import plane_ref
import refit_ref
from test_gpu_range import _dev, _prepared, _soa, _stats
from test_gpu_refit import _m44, _same, _score, _t16

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
BOUND = 1e-9
PIVOT = 1e-2
R15 = np.float32(1.5) ** 2
RADII = [np.float32(0.0), np.float32(0.5) ** 2, R15, np.float32(np.inf)]


def _nrm(normals, ld=None):
    """[M, 3] -> the [3, M] tensor PreparedModel.normals returns (a view of a [3, ld] one when ld is given)"""
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    if ld is None:
        return _soa(n)
    wide = torch.full((3, ld), 1e30, dtype=torch.float32, device=_dev())
    wide[:, :len(n)] = _soa(n)
    return wide[:, :len(n)]


def _plane(pm, q, Td, r2, nrm, steps=1, out=None):
    """-> T_out [B, 4, 4], T_step [B, 4, 4], n_close, sum_d2, n_plane, sum_res2, empty as numpy"""
    got = pm.refit_plane(q, Td, r2, nrm, steps=steps, out=out)
    torch.cuda.synchronize()
    T_out, T_step, n, s, npl, res, e = (t.cpu().numpy() for t in got)
    return _m44(T_out), _m44(T_step), n, s, npl, res, e


def _check(got, T, want, what=""):
    """checks 1 and 2 for one call: `want` is plane_ref.step on the bits of T and of the normals that the device was given"""
    T_out, T_step, n, s, npl, res, e = got
    np.testing.assert_array_equal(n, want["n_close"])
    np.testing.assert_array_equal(npl, want["n_plane"])
    np.testing.assert_array_equal(e != 0, want["empty"])
    assert set(np.unique(e).tolist()) <= {0, 1}
    worst = 0.0
    for b in range(len(T)):
        assert abs(res[b] - want["sum_res2"][b]) <= 1e-12 * want["sum_res2"][b], (what, b, res[b], want["sum_res2"][b])
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any(), b              # all 32 numbers are 0.0
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        assert want["pivot"][b] >= PIVOT, (what, b, want["pivot"][b])         # the premise of the bound
        err = float(np.linalg.norm(T_step[b] - want["T_step"][b]))
        print(f"  {what} b = {b}: n_plane {npl[b]}, |T_step - reference| = {err:.3e} ({err / BOUND:.1e} of the bound), smallest pivot {want['pivot'][b]:.3f}")
        assert err < BOUND, (what, b, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("r2", RADII, ids=["r0", "r0.5", "r1.5", "rinf"])
def test_counts_are_scorings_bits_and_the_fit_is_the_references(r2, debug_set):
    """checks 1, 2 and 3 on the main scene"""
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    Q = len(surf)
    want = plane_ref.scene_ref(r2, threads=CORES)
    pm, _t = _prepared(model)
    try:
        q, Td, nrm = _soa(surf), _t16(T), _nrm(sc["normals"])
        got = _plane(pm, q, Td, r2, nrm)
        n, s = _score(pm, q, Td, r2)
        np.testing.assert_array_equal(got[2], n)                                           # 1
        np.testing.assert_array_equal(got[3].view(np.uint64), s.view(np.uint64))
        worst = _check(got, T, want, f"r2 = {float(r2):.4g}")                              # 1, 2
        print(f"r2 = {float(r2):.4g}: n_close {got[2].tolist()}, n_plane {got[4].tolist()}, empty {got[6].tolist()}, worst |T_step - reference| "
              f"{worst:.3e} = {worst / BOUND:.1e} of the bound")
        if r2 == R15:
            assert got[6].tolist() == [0, 0, 0, 0, 1, 1]
        _same(_plane(pm, q, Td, r2, nrm), got)                                             # 3: twice
        debug_set("knn_nocull", 1)
        g0 = _plane(pm, q, Td, r2, nrm)
        debug_set("knn_nocull", 0)
        _same(g0, got)
        debug_set("knn_stats", 1)
        _stats(reset=True)
        debug_set("score_batch_slots", 2 * Q)
        g1 = _plane(pm, q, Td, r2, nrm)
        st = _stats(reset=True)
        debug_set("score_batch_slots", 0)
        assert st[0] == 3, st                                                              # premise: 2 + 2 + 2 transforms
        _same(g1, got)
    finally:
        pm.close()


def test_the_sign_cannot_matter_and_nan_rows_offer_no_plane():
    """check 4"""
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"], sc["T"], sc["normals"]
    rng = np.random.default_rng(41)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _plane(pm, q, Td, R15, _nrm(normals))
        half = normals.copy()
        half[rng.random(len(model)) < 0.5] *= np.float32(-1)
        assert (half != normals).any(axis=1).sum() > 1000
        _same(_plane(pm, q, Td, R15, _nrm(-normals)), got)
        _same(_plane(pm, q, Td, R15, _nrm(half)), got)
        tenth = normals.copy()
        drop = rng.choice(len(model), len(model) // 10, replace=False)
        tenth[drop, rng.integers(0, 3, len(drop))] = np.nan                                # one component is enough
        tenth[drop[:50]] = np.inf
        want = plane_ref.step(surf, model, tenth, T, R15, threads=CORES)
        assert (want["n_plane"][:4] < want["n_close"][:4]).all() and (want["n_plane"][:4] > 2000).all()      # premise: rows were dropped
        g = _plane(pm, q, Td, R15, _nrm(tenth))
        _check(g, T, want, "a tenth NaN")
        np.testing.assert_array_equal(g[2], got[2])
        np.testing.assert_array_equal(g[3].view(np.uint64), got[3].view(np.uint64))
        g = _plane(pm, q, Td, R15, _nrm(np.full_like(normals, np.nan)))
        assert g[4].tolist() == [0] * 6 and g[6].tolist() == [1] * 6 and g[5].tolist() == [0.0] * 6 and not g[0].any() and not g[1].any()
        np.testing.assert_array_equal(g[2], got[2])                                        # n_close is still scoring's
        np.testing.assert_array_equal(g[3].view(np.uint64), got[3].view(np.uint64))
    finally:
        pm.close()


def _few(k):
    """a model of 3000 rows in [-20, 20]^3 with random unit normals (general position) and a cloud of 2500 points of which exactly k
    lie near a model row (N(0, 0.05^2) off it), the rest model rows shifted out of reach; for k >= 2 two of the k are queries
    2047 and 2048, on both sides of the chunk boundary"""
    rng = np.random.default_rng(60 + k)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    normals = rng.normal(size=(3000, 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(np.float32)
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.float32(100.0)).astype(np.float32)
    at = sorted(([2047, 2048] if k >= 2 else []) + rng.choice(2000, max(k - 2, 0) if k >= 2 else k, replace=False).tolist())
    rows = rng.choice(3000, k, replace=False)
    for i, r in zip(at, rows):
        surf[i] = model[r] + rng.normal(0, 0.05, 3).astype(np.float32)
    return model, normals, surf, at, rows


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 6, 7])
def test_exactly_k_plane_pairs(k):
    """check 5: r = 0.5 under the identity, and a second candidate that meets nothing"""
    model, normals, surf, at, rows = _few(k)
    far = np.eye(4)
    far[3, :3] = [0.0, 300.0, 0.0]
    T = np.stack([np.eye(4), far])
    r2 = np.float32(0.5) ** 2
    want = plane_ref.step(surf, model, normals, T, r2, threads=CORES)
    assert want["n_close"].tolist() == [k, 0] and want["n_plane"].tolist() == [k, 0] and np.flatnonzero(want["hit"][0]).tolist() == at      # premise
    assert want["idx"][0][at].tolist() == rows.tolist()
    assert want["empty"].tolist() == [k < 6, True]
    if k >= 2:
        assert 2047 in at and 2048 in at
    pm, _t = _prepared(model)
    try:
        got = _plane(pm, _soa(surf), _t16(T), r2, _nrm(normals))
        _check(got, T, want, f"k = {k}")
    finally:
        pm.close()


def _lattice(z, n=64):
    g = np.arange(n, dtype=np.float64) * 0.5
    a, b = (v.ravel() for v in np.meshgrid(g, g))
    return np.column_stack([a, b, np.full_like(a, z)])


@pytest.mark.parametrize("case", ["flat", "parallel", "tilted"])
def test_models_that_leave_a_direction_free_are_empty(case):
    """check 6: all normals equal.  flat / parallel: normals (0, 0, 1), so J_2 = J_3 = J_4 = 0 and A_22 = 0 exactly; tilted: a plane
    with the normal (1, 2, 2) / 3, where every A_ii is positive and it is a pivot that vanishes"""
    rng = np.random.default_rng(71)
    if case == "parallel":
        model = np.vstack([_lattice(0.0, 45), _lattice(5.0, 45)])
    else:
        model = _lattice(0.0)
    n = np.array([0.0, 0.0, 1.0])
    surf = model[rng.choice(len(model), 2500, replace=False)] + np.column_stack([rng.normal(0, 0.05, (2500, 2)), rng.normal(0, 0.02, 2500)])
    if case == "tilted":                                  # rotate the whole scene so that z goes to (1, 2, 2) / 3
        n = np.array([1.0, 2.0, 2.0]) / 3.0
        a = np.cross([0.0, 0.0, 1.0], n); a /= np.linalg.norm(a)
        Rz = np.column_stack([a, np.cross(n, a), n])      # columns: the images of x, y, z
        model, surf = model @ Rz.T, surf @ Rz.T
    model, surf = model.astype(np.float32), surf.astype(np.float32)
    normals = np.tile(n.astype(np.float32), (len(model), 1))
    T = np.stack([np.eye(4), plane_ref.about(plane_ref.rigid([0.004, -0.003, 0.005], [0.02, -0.01, 0.03]), model.mean(axis=0).astype(np.float64))])
    want = plane_ref.step(surf, model, normals, T, R15, threads=CORES)
    assert (want["n_plane"] == 2500).all() and want["empty"].all()                         # the reference's verdict
    pm, _t = _prepared(model)
    try:
        got = _plane(pm, _soa(surf), _t16(T), R15, _nrm(normals))
        _check(got, T, want, case)
        assert got[6].tolist() == [1, 1] and got[4].tolist() == [2500, 2500] and (got[5] > 0).all()
    finally:
        pm.close()


def test_edges_and_argument_errors():
    """check 7"""
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, PcregError, check, lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"][:300], sc["T"][:4], sc["normals"]
    M = len(model)
    want = plane_ref.step(surf, model, normals, T, R15, threads=CORES)
    pm, _t = _prepared(model)
    pm0, _t0 = _prepared(model[:0])
    try:
        q, Td, nrm = _soa(surf), _t16(T), _nrm(normals)
        got = _plane(pm, q, Td, R15, nrm)
        _check(got, T, want, "300 queries")
        # ldq > Q and ldn > M: the queries are columns 100 .. 399 of a wider buffer, the normals the first M of 5000 columns
        wide = torch.full((3, 1000), 1e30, dtype=torch.float32, device=_dev())
        wide[:, 100:400] = q
        qw, nw = wide[:, 100:400], _nrm(normals, ld=5000)
        assert qw.stride(0) == 1000 and nw.stride(0) == 5000
        _same(_plane(pm, qw, Td, R15, nw), got)
        # Q = 0, and a model without rows: every transform empty, the counts and sums 0
        n0 = torch.zeros((3, 0), dtype=torch.float32, device=_dev())
        for g in (_plane(pm, _soa(surf[:0]), Td, R15, nrm), _plane(pm0, q, Td, R15, n0), _plane(pm0, _soa(surf[:0]), Td, R15, n0)):
            assert g[2].tolist() == [0] * 4 and g[3].tolist() == [0.0] * 4 and g[4].tolist() == [0] * 4 and g[5].tolist() == [0.0] * 4
            assert g[6].tolist() == [1] * 4 and not g[0].any() and not g[1].any()
        # B = 0 through the C ABI: nothing is written into canary-filled outputs
        canary_d = torch.full((48,), -7.0, dtype=torch.float64, device=_dev())
        canary_i = torch.full((12,), -7, dtype=torch.int32, device=_dev())
        ws0 = torch.empty(int(L.pcreg_dev_model_refit_plane_workspace(300, 0, M)), dtype=torch.uint8, device=_dev())
        check(L.pcreg_dev_model_refit_plane_f32(pm.handle, q.data_ptr(), 300, 300, None, 0, 1.0, nrm.data_ptr(), M, canary_d.data_ptr(),
                                                canary_d[16:].data_ptr(), canary_i.data_ptr(), canary_d[32:].data_ptr(), canary_i[4:].data_ptr(),
                                                canary_d[40:].data_ptr(), canary_i[8:].data_ptr(), ws0.data_ptr(), ws0.numel(), None))
        torch.cuda.synchronize()
        assert canary_d.tolist() == [-7.0] * 48 and canary_i.tolist() == [-7] * 12
        assert pm.refit_plane(q, Td[:0], R15, nrm)[0].shape == (0, 16)
        # T_step = NULL: the other outputs are the same bits
        To = torch.empty((4, 16), dtype=torch.float64, device=_dev())
        n, npl, e = (torch.empty(4, dtype=torch.int32, device=_dev()) for _ in range(3))
        s, res = (torch.empty(4, dtype=torch.float64, device=_dev()) for _ in range(2))
        need = int(L.pcreg_dev_model_refit_plane_workspace(300, 4, M))
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(Q=300, ldq=300, B=4, r2=float(R15), wsb=need, qp=q.data_ptr(), tp=Td.data_ptr(), h=pm.handle, op=To.data_ptr(), ep=e.data_ptr(),
                 nr=nrm.data_ptr(), ldn=M, pp=npl.data_ptr(), rp=res.data_ptr()):
            return L.pcreg_dev_model_refit_plane_f32(h, qp, Q, ldq, tp, B, r2, nr, ldn, op, None, n.data_ptr(), s.data_ptr(), pp, rp, ep, ws.data_ptr(), wsb, None)
        assert call() == PCREG_OK
        torch.cuda.synchronize()
        _same((_m44(To.cpu().numpy()),) + tuple(t.cpu().numpy() for t in (n, s, npl, res, e)), (got[0],) + got[2:])
        for kw in (dict(r2=float("nan")), dict(r2=-1.0), dict(r2=float("-inf")), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1, wsb=1 << 40), dict(B=-1),
                   dict(Q=-1), dict(ldq=299), dict(wsb=need - 1), dict(qp=None), dict(tp=None), dict(h=None), dict(op=None), dict(ep=None),
                   dict(pp=None), dict(rp=None), dict(nr=None), dict(ldn=M - 1), dict(ldn=-1), dict(op=Td.data_ptr())):
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        assert call(r2=float("inf")) == PCREG_OK and call(r2=0.0) == PCREG_OK and call(ldn=M) == PCREG_OK
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            pm.refit_plane(q, Td, -1.0, nrm)
        with pytest.raises(ValueError):
            pm.refit_plane(q, Td, 1.0, nrm, steps=0)
        with pytest.raises(TypeError):
            pm.refit_plane(q, Td.float(), 1.0, nrm)
        with pytest.raises(TypeError):
            pm.refit_plane(q, Td, 1.0, nrm[:, :100])
        # the host tier
        with pc.Model(model) as h:
            out, ss, rr = np.zeros((4, 16)), np.zeros(4), np.zeros(4)
            nn, pp, ee = (np.zeros(4, np.int32) for _ in range(3))
            T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
            qs, ns = np.asfortranarray(surf), np.asfortranarray(normals)
            args = lambda steps=1, r2=float(R15), nr=ns.ctypes.data, ldn=M, k=6: (h._h, qs.ctypes.data, 300, 300, T16.ctypes.data, 4, r2, steps, nr, ldn, k,
                                                                                 out.ctypes.data, nn.ctypes.data, ss.ctypes.data, pp.ctypes.data,
                                                                                 rr.ctypes.data, ee.ctypes.data)
            f = L.pcreg_model_refit_plane_f32
            assert f(*args(0)) == PCREG_E_ARG and f(*args(-1)) == PCREG_E_ARG
            assert f(*args(1, float("nan"))) == PCREG_E_ARG and f(*args(1, -1.0)) == PCREG_E_ARG
            assert f(*args(ldn=M - 1)) == PCREG_E_ARG and f(*args(ldn=-1)) == PCREG_E_ARG
            for k in (2, 33, 0, -1):
                assert f(*args(nr=None, k=k)) == PCREG_E_ARG, k
            assert f(*args(k=-5)) == PCREG_OK                                              # normals given: k is ignored
            _same((_m44(out), nn, ss, pp, rr, ee), (got[0],) + got[2:])
            with pytest.raises(ValueError):
                h.refit_plane(surf, T, 1.0, steps=0)
            with pytest.raises(ValueError):
                h.refit_plane(surf, T, 1.0, k=2)
            with pytest.raises(ValueError):
                h.refit_plane(surf, T, 1.0, normals=normals[:100])
            with pytest.raises((ValueError, PcregError)):
                h.refit_plane(surf, T, -1.0)
            r = h.refit_plane(surf, T, R15, normals=normals)
            _same((r["T"], r["n_close"], r["sum_d2"], r["n_plane"], r["sum_res2"], r["empty"]), (got[0],) + got[2:6] + (got[6] != 0,))
            np.testing.assert_array_equal(r["plane_rmse"][:4], np.sqrt(got[5] / got[4]))
        with pc.Model(model[:0]) as h0:                                                    # a model without rows at the host tier
            r = h0.refit_plane(surf, T, R15)
            assert r["empty"].all() and not r["T"].any() and not r["n_plane"].any() and np.isnan(r["plane_rmse"]).all()
    finally:
        pm.close()
        pm0.close()


def test_a_model_without_rows_writes_nothing_behind_the_workspace():
    """more transforms than one batch holds (B Q = 4.8 Mi slots against a workspace for S = 3.6 Mi) on a model without rows, and with
    Q = 0 on one with rows: every transform empty, and 8 MiB of canary right behind the stated workspace size stay as they were.
    (Nothing but the walk may write the per-slot row block, which holds one batch.)"""
    from pcreg_amd._lib import check, lib
    L = lib()
    Q, B, tail = 600_000, 8, 8 << 20
    assert B * Q > 4 << 20 and (4 << 20) // Q < B                          # premise: more than one batch
    sc = plane_ref.scene()
    pm, _t = _prepared(sc["model"])
    pm0, _t0 = _prepared(sc["model"][:0])
    try:
        q = torch.zeros((3, Q), dtype=torch.float32, device=_dev())
        Td = _t16(np.tile(np.eye(4), (B, 1, 1)))
        nrm = _nrm(sc["normals"])
        for h, M, Qc, nr in ((pm0, 0, Q, torch.zeros((3, 1), dtype=torch.float32, device=_dev())), (pm, pm.M, 0, nrm)):
            need = int(L.pcreg_dev_model_refit_plane_workspace(Qc, B, M))
            ws = torch.full((need + tail,), 0x5A, dtype=torch.uint8, device=_dev())
            To, Ts = (torch.full((B, 16), -7.0, dtype=torch.float64, device=_dev()) for _ in range(2))
            n, npl, e = (torch.full((B,), -7, dtype=torch.int32, device=_dev()) for _ in range(3))
            s, res = (torch.full((B,), -7.0, dtype=torch.float64, device=_dev()) for _ in range(2))
            check(L.pcreg_dev_model_refit_plane_f32(h.handle, q.data_ptr() if Qc else None, Qc, max(Qc, 1), Td.data_ptr(), B, float(R15), nr.data_ptr(),
                                                    max(M, 1), To.data_ptr(), Ts.data_ptr(), n.data_ptr(), s.data_ptr(), npl.data_ptr(), res.data_ptr(),
                                                    e.data_ptr(), ws.data_ptr(), need, None))
            torch.cuda.synchronize()
            assert bool((ws[need:] == 0x5A).all()), (M, Qc)
            assert e.tolist() == [1] * B and n.tolist() == [0] * B and npl.tolist() == [0] * B and s.tolist() == [0.0] * B and res.tolist() == [0.0] * B
            assert not To.any() and not Ts.any()
    finally:
        pm.close()
        pm0.close()


def test_three_steps_on_the_device_at_the_host_tier_and_against_the_reference():
    """check 8"""
    import pcreg_amd as pc
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"], sc["T"], sc["normals"]
    pm, _t = _prepared(model)
    try:
        q, Td, nrm = _soa(surf), _t16(T), _nrm(normals)
        three = _plane(pm, q, Td, R15, nrm, steps=3)
        cur, singles = Td, []
        for k in range(3):
            out = pm.refit_plane(q, cur, R15, nrm)
            cur = out[0].clone()                                           # fed back on the device
            torch.cuda.synchronize()
            singles.append(tuple(t.cpu().numpy() for t in out))
        last = singles[-1]
        _same(three, (_m44(last[0]), _m44(last[1])) + last[2:])
        with pc.Model(model) as h:
            r = h.refit_plane(surf, T, R15, steps=3, normals=normals)
            _same((r["T"], r["n_close"], r["sum_d2"], r["n_plane"], r["sum_res2"], r["empty"]), (three[0],) + three[2:6] + (three[6] != 0,))
            # normals computed inside the call (k = 8) against the same call on Model.normals(8)
            own = h.normals(8)
            a, b = h.refit_plane(surf, T, R15, steps=3, k=8), h.refit_plane(surf, T, R15, steps=3, normals=own)
            assert sorted(a) == sorted(b)
            _same(tuple(np.asarray(a[key]) for key in sorted(a)), tuple(np.asarray(b[key]) for key in sorted(b)))
            assert not a["empty"][:4].any()
        # every step against the reference's step on the bits the device gave that step
        T_in = T
        for k in range(3):
            want = plane_ref.step(surf, model, normals, T_in, R15, threads=CORES)
            got = (_m44(singles[k][0]), _m44(singles[k][1])) + singles[k][2:]
            worst = _check(got, T_in, want, f"step {k + 1}")
            print(f"step {k + 1}: n_plane {got[4].tolist()}, plane RMSE {np.sqrt(got[5][:4] / got[4][:4]).tolist()}, worst |T_step - reference| {worst:.3e}")
            T_in = got[0]
        assert (singles[2][6] == [0, 0, 0, 0, 1, 1]).all()                 # a failed candidate stays failed
    finally:
        pm.close()


def test_normals_from_the_device_chain_into_the_refit():
    """check 9: pm.normals(8) straight into pm.refit_plane, against the reference on those normals"""
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        nrm = pm.normals(8)
        got = _plane(pm, q, Td, R15, nrm)
        host_normals = np.ascontiguousarray(nrm.cpu().numpy().T)
        assert np.isfinite(host_normals).all()
        want = plane_ref.step(surf, model, host_normals, T, R15, threads=CORES)
        worst = _check(got, T, want, "device normals")
        print(f"device normals: worst |T_step - reference| {worst:.3e}")
        assert got[6].tolist() == [0, 0, 0, 0, 1, 1]
    finally:
        pm.close()


def test_five_plane_steps_against_five_point_to_point_steps():
    """check 10, what the feature is for: from the largest perturbation at r = 1.5, the RMS distance of the moved surface from its
    true place.  The references' own ratio is at most 1/6 (tests/test_plane_ref.py), so 1/4 leaves the device a margin."""
    sc = plane_ref.scene()
    model, surf, T, cloud = sc["model"], sc["surf"], sc["T"][3:4], sc["cloud"]
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        plane = _plane(pm, q, Td, R15, _nrm(sc["normals"]), steps=5)
        point = pm.refit_transforms(q, Td, R15, steps=5)
        torch.cuda.synchronize()
        assert plane[6].tolist() == [0] and point[4].cpu().tolist() == [0]
        a = plane_ref.rms_to_truth(surf, plane[0][0], cloud)
        b = plane_ref.rms_to_truth(surf, _m44(point[0].cpu().numpy())[0], cloud)
        print(f"RMS distance from the truth: start {plane_ref.rms_to_truth(surf, T[0], cloud):.4f}, five plane steps {a:.4f}, five point-to-point steps {b:.4f}")
        assert a <= b / 4.0
    finally:
        pm.close()


def test_refine_trials_with_normals_keeps_the_orientation_and_the_failed_trial():
    """check 11"""
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, nrm = _soa(surf), _nrm(sc["normals"])
        result = dict(trial=np.array([4, 9, 11]), transforms=[pc.invertTF(T[1]), None, pc.invertTF(T[3])])
        inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
        direct = _plane(pm, q, _t16(inv), R15, nrm, steps=2)
        out, summary = refine_trials(result, pm, q, 1.5, steps=2, normals=nrm)
        assert len(out) == 3 and out[1] is None and direct[6].tolist() == [0, 1, 0]
        for t in (0, 2):
            np.testing.assert_array_equal(out[t], pc.invertTF(direct[0][t]))
        np.testing.assert_array_equal(summary["n_close"], direct[2])
        np.testing.assert_array_equal(summary["sum_d2"].view(np.uint64), direct[3].view(np.uint64))
        assert summary["n_close"][1] == 0 and np.isnan(summary["rmse"][1]) and len(summary["fitness"]) == 3
        # without normals: the point-to-point path, bit for bit what refit_transforms gives
        plain, psum = refine_trials(result, pm, q, 1.5, steps=2)
        p2p = pm.refit_transforms(q, _t16(inv), R15, steps=2)
        torch.cuda.synchronize()
        for t in (0, 2):
            np.testing.assert_array_equal(plain[t], pc.invertTF(_m44(p2p[0].cpu().numpy())[t]))
        assert plain[1] is None
        np.testing.assert_array_equal(psum["sum_d2"].view(np.uint64), p2p[3].cpu().numpy().view(np.uint64))
        assert refine_trials(dict(trial=[], transforms=[]), pm, q, 1.5, normals=nrm)[0] == []
    finally:
        pm.close()


def test_two_streams_on_one_handle():
    """check 12: each call with its own workspace and outputs"""
    from pcreg_amd._lib import lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, Td, nrm = _soa(surf), _t16(T), _nrm(sc["normals"])
        halves = ((q[:, :2000].contiguous(), Td[:4].contiguous()), (q[:, 400:].contiguous(), Td[2:].contiguous()))
        want = []
        for a, b in halves:
            out = pm.refit_plane(a, b, R15, nrm, steps=2)
            torch.cuda.synchronize()
            want.append(tuple(t.cpu().numpy() for t in out))
        outs = []
        for a, b in halves:
            Qh, Bh = a.shape[1], b.shape[0]
            d64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=_dev())
            i32 = lambda: torch.empty(Bh, dtype=torch.int32, device=_dev())
            outs.append((d64(Bh, 16), d64(Bh, 16), i32(), d64(Bh), i32(), d64(Bh), i32(),
                         torch.empty(int(L.pcreg_dev_model_refit_plane_workspace(Qh, Bh, pm.M)), dtype=torch.uint8, device=_dev()), d64(Bh, 16)))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, (a, b), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.refit_plane(a, b, R15, nrm, steps=2, out=o)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            _same(tuple(t.cpu().numpy() for t in o[:7]), w)
    finally:
        pm.close()
