"""Candidate transforms refitted by the plane-to-plane (generalized ICP) step (knn_score.hip + gicp_pair.hpp) on the GPU.

n_close and the bits of sum_d2 against score_transforms on the same inputs; n_pairs, empty, T_step and sum_res2 against
tests/gicp_ref.py (score_ref's pairs, S, its inverse and the 28 sums in longdouble, plane_ref's fit, the composition restated
entry by entry); the same bits twice, with culling off, in three batches and with padded leading dimensions; the sign of either
set of normals and NaN normals on either side; exactly k = 0 .. 7 pairs, two of them across the chunk boundary; a flat model,
where the point-to-plane step is empty and this one is not; three steps on the device, at the host tier and against the
reference step by step, with both sets of normals computed in the call; refine_trials; the argument errors; two streams on one
handle.

The bound on T_step, 1e-9 in the Frobenius norm, is tests/test_gpu_refit.py's BOUND in the same role.  It is asserted only where
the smallest pivot of the reference's scaled matrix is at least 1e-2 (asserted as the premise; tests/test_gicp_ref.py shows it
for the main scene and for the flat model without a GPU).

The bound on sum_res2 is relative: 8 x the worst relative error of the float64 restatement's sum_res2 against the longdouble
reference over the main scene's radii and epsilon in {1e-3, 1e-2}, and not below 1e-12 (the plane refit's bound).  Measured on
the CPU by tests/test_gicp_ref.py: 3.99e-15, so 8 x that is 3.2e-14 and the bound is 1e-12."""
import os

import numpy as np
import pytest
import torch

import gicp_ref
import plane_ref
import refit_ref
from test_gicp_ref import SUM_RES2_BOUND, flat_scene
from test_gpu_range import _dev, _prepared, _soa, _stats
from test_gpu_refit import _m44, _same, _score, _t16

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
BOUND = 1e-9
PIVOT = 1e-2
RES2 = 1e-12
R15 = np.float32(1.5) ** 2
RADII = [np.float32(0.0), np.float32(0.5) ** 2, R15, np.float32(np.inf)]
assert RES2 == SUM_RES2_BOUND


def _nrm(normals, ld=None):
    """[N, 3] -> the [3, N] tensor PreparedModel.normals returns (a view of a [3, ld] one, its padding 1e30, when ld is given)"""
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    if ld is None:
        return _soa(n)
    wide = torch.full((3, ld), 1e30, dtype=torch.float32, device=_dev())
    wide[:, :len(n)] = _soa(n)
    return wide[:, :len(n)]


def _gicp(pm, q, Td, r2, nrm, nq, epsilon=1e-3, steps=1, out=None):
    """-> T_out [B, 4, 4], T_step [B, 4, 4], n_close, sum_d2, n_pairs, sum_res2, empty as numpy"""
    got = pm.refit_gicp(q, Td, r2, nrm, nq, epsilon=epsilon, steps=steps, out=out)
    torch.cuda.synchronize()
    T_out, T_step, n, s, npr, res, e = (t.cpu().numpy() for t in got)
    return _m44(T_out), _m44(T_step), n, s, npr, res, e


def _check(got, T, want, what=""):
    """one call against `want`, gicp_ref.step on the bits of T and of the normals that the device was given -> the worst errors"""
    T_out, T_step, n, s, npr, res, e = got
    np.testing.assert_array_equal(n, want["n_close"])
    np.testing.assert_array_equal(npr, want["n_pairs"])
    np.testing.assert_array_equal(e != 0, want["empty"])
    assert set(np.unique(e).tolist()) <= {0, 1}
    worst, worst_res = 0.0, 0.0
    for b in range(len(T)):
        rel = abs(res[b] - want["sum_res2"][b]) / want["sum_res2"][b] if want["sum_res2"][b] > 0 else abs(res[b])
        worst_res = max(worst_res, rel)
        assert rel <= RES2, (what, b, res[b], want["sum_res2"][b])
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any(), b              # all 32 numbers are 0.0
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        assert want["pivot"][b] >= PIVOT, (what, b, want["pivot"][b])         # the premise of the bound
        err = float(np.linalg.norm(T_step[b] - want["T_step"][b]))
        print(f"  {what} b = {b}: n_pairs {npr[b]}, |T_step - reference| = {err:.3e} ({err / BOUND:.1e} of the bound), sum_res2 off by {rel:.2e} "
              f"relative, smallest pivot {want['pivot'][b]:.3f}")
        assert err < BOUND, (what, b, err)
        worst = max(worst, err)
    return worst, worst_res


@pytest.mark.parametrize("r2", RADII, ids=["r0", "r0.5", "r1.5", "rinf"])
def test_counts_are_scorings_bits_and_the_fit_is_the_references(r2, debug_set):
    """checks 1 and 2 on the main scene"""
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    Q, M = len(surf), len(model)
    sn = gicp_ref.surface_normals()
    want = gicp_ref.scene_ref(r2, threads=CORES)
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _nrm(sc["normals"]), _nrm(sn)
        got = _gicp(pm, q, Td, r2, nrm, nq)
        n, s = _score(pm, q, Td, r2)
        np.testing.assert_array_equal(got[2], n)                                           # 1
        np.testing.assert_array_equal(got[3].view(np.uint64), s.view(np.uint64))
        worst, worst_res = _check(got, T, want, f"r2 = {float(r2):.4g}")
        print(f"r2 = {float(r2):.4g}: n_close {got[2].tolist()}, n_pairs {got[4].tolist()}, empty {got[6].tolist()}, worst |T_step - reference| "
              f"{worst:.3e} = {worst / BOUND:.1e} of the bound, worst relative error of sum_res2 {worst_res:.3e} = {worst_res / RES2:.1e} of its bound")
        if r2 == R15:
            assert got[6].tolist() == [0, 0, 0, 0, 1, 1]
            want2 = gicp_ref.scene_ref(r2, 1e-2, threads=CORES)                            # the other epsilon
            _check(_gicp(pm, q, Td, r2, nrm, nq, epsilon=1e-2), T, want2, "epsilon = 1e-2")
        _same(_gicp(pm, q, Td, r2, nrm, nq), got)                                          # 2: twice
        debug_set("knn_nocull", 1)
        g0 = _gicp(pm, q, Td, r2, nrm, nq)
        debug_set("knn_nocull", 0)
        _same(g0, got)
        debug_set("knn_stats", 1)
        _stats(reset=True)
        debug_set("score_batch_slots", 2 * Q)
        g1 = _gicp(pm, q, Td, r2, nrm, nq)
        st = _stats(reset=True)
        debug_set("score_batch_slots", 0)
        assert st[0] == 3, st                                                              # premise: 2 + 2 + 2 transforms
        _same(g1, got)
        nw, nqw = _nrm(sc["normals"], ld=M + 904), _nrm(sn, ld=Q + 572)                    # ldn > M and ldnq > Q, the padding 1e30
        assert nw.stride(0) == M + 904 and nqw.stride(0) == Q + 572
        _same(_gicp(pm, q, Td, r2, nw, nqw), got)
    finally:
        pm.close()


def test_the_signs_cannot_matter_and_nan_normals_drop_their_pairs():
    """check 3"""
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"], sc["T"], sc["normals"]
    sn = gicp_ref.surface_normals()
    rng = np.random.default_rng(41)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _gicp(pm, q, Td, R15, _nrm(normals), _nrm(sn))
        half, halfq = normals.copy(), sn.copy()
        half[rng.random(len(model)) < 0.5] *= np.float32(-1)
        halfq[rng.random(len(surf)) < 0.5] *= np.float32(-1)
        assert (half != normals).any(axis=1).sum() > 1000 and (halfq != sn).any(axis=1).sum() > 800
        for a, b in ((-normals, sn), (normals, -sn), (half, sn), (normals, halfq), (half, halfq)):
            _same(_gicp(pm, q, Td, R15, _nrm(a), _nrm(b)), got)
        tenth, tenthq = normals.copy(), sn.copy()
        drop = rng.choice(len(model), len(model) // 10, replace=False)
        tenth[drop, rng.integers(0, 3, len(drop))] = np.nan                                # one component is enough
        tenth[drop[:50]] = np.inf
        dropq = rng.choice(len(surf), len(surf) // 10, replace=False)
        tenthq[dropq, rng.integers(0, 3, len(dropq))] = np.nan
        tenthq[dropq[:50]] = -np.inf
        for a, b, what in ((tenth, sn, "model normals a tenth NaN"), (normals, tenthq, "query normals a tenth NaN"), (tenth, tenthq, "both a tenth NaN")):
            want = gicp_ref.step(surf, model, a, b, T, R15, threads=CORES)
            assert (want["n_pairs"][:4] < want["n_close"][:4]).all() and (want["n_pairs"][:4] > 1800).all()      # premise: pairs were dropped
            g = _gicp(pm, q, Td, R15, _nrm(a), _nrm(b))
            _check(g, T, want, what)
            np.testing.assert_array_equal(g[2], got[2])
            np.testing.assert_array_equal(g[3].view(np.uint64), got[3].view(np.uint64))
        for a, b in ((np.full_like(normals, np.nan), sn), (normals, np.full_like(sn, np.nan))):
            g = _gicp(pm, q, Td, R15, _nrm(a), _nrm(b))
            assert g[4].tolist() == [0] * 6 and g[6].tolist() == [1] * 6 and g[5].tolist() == [0.0] * 6 and not g[0].any() and not g[1].any()
            np.testing.assert_array_equal(g[2], got[2])                                    # n_close is still scoring's
            np.testing.assert_array_equal(g[3].view(np.uint64), got[3].view(np.uint64))
    finally:
        pm.close()


def _few(k):
    """tests/test_gpu_refit_plane.py's: a model of 3000 rows in [-20, 20]^3 with random unit normals and a cloud of 2500 points of which
    exactly k lie near a model row, the rest out of reach; for k >= 2 two of the k are queries 2047 and 2048, on both sides of the
    chunk boundary.  The cloud has random unit normals too."""
    rng = np.random.default_rng(60 + k)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    normals = rng.normal(size=(3000, 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(np.float32)
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.float32(100.0)).astype(np.float32)
    at = sorted(([2047, 2048] if k >= 2 else []) + rng.choice(2000, max(k - 2, 0) if k >= 2 else k, replace=False).tolist())
    rows = rng.choice(3000, k, replace=False)
    for i, r in zip(at, rows):
        surf[i] = model[r] + rng.normal(0, 0.05, 3).astype(np.float32)
    qn = rng.normal(size=(2500, 3))
    qn = (qn / np.linalg.norm(qn, axis=1)[:, None]).astype(np.float32)
    return model, normals, surf, qn, at, rows


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 6, 7])
def test_exactly_k_pairs(k):
    """check 4: r = 0.5 under the identity, and a second candidate that meets nothing"""
    model, normals, surf, qn, at, rows = _few(k)
    far = np.eye(4)
    far[3, :3] = [0.0, 300.0, 0.0]
    T = np.stack([np.eye(4), far])
    r2 = np.float32(0.5) ** 2
    want = gicp_ref.step(surf, model, normals, qn, T, r2, threads=CORES)
    assert want["n_close"].tolist() == [k, 0] and want["n_pairs"].tolist() == [k, 0] and np.flatnonzero(want["hit"][0]).tolist() == at      # premise
    assert want["idx"][0][at].tolist() == rows.tolist()
    assert want["empty"][1] and (k >= 6 or want["empty"][0])
    if k >= 2:
        assert 2047 in at and 2048 in at
    if k >= 6:
        print(f"k = {k}: the reference's verdict empty = {bool(want['empty'][0])}, smallest pivot {want['pivot'][0]:.4f}")
        assert not want["empty"][0]                                                        # every pair pulls in three directions: six suffice
    pm, _t = _prepared(model)
    try:
        got = _gicp(pm, _soa(surf), _t16(T), r2, _nrm(normals), _nrm(qn))
        np.testing.assert_array_equal(got[4], want["n_pairs"])
        np.testing.assert_array_equal(got[6] != 0, want["empty"])
        if k < 6 or want["pivot"][0] >= PIVOT:
            _check(got, T, want, f"k = {k}")
        else:                                                                              # a fit, but not one the bound's premise covers
            np.testing.assert_array_equal(got[0][0].view(np.uint64), refit_ref.compose(T[0], got[1][0]).view(np.uint64))
    finally:
        pm.close()


def test_a_flat_model_is_empty_for_the_plane_step_and_not_for_this_one():
    """check 5: z = const and normals (0, 0, 1) on both sides; in-plane sliding is free for the point-to-plane step and held here"""
    fl = flat_scene()
    model, pts, T = fl["model"], fl["pts"], fl["T"]
    r2 = np.float32(1.0)
    want = gicp_ref.step(pts, model, fl["normals"], fl["qnormals"], T, r2, threads=CORES)
    assert not want["empty"].any() and (want["pivot"] >= PIVOT).all()                      # (tests/test_gicp_ref.py shows it without a GPU)
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(pts), _t16(T), _nrm(fl["normals"]), _nrm(fl["qnormals"])
        plane = pm.refit_plane(q, Td, r2, nrm)
        torch.cuda.synchronize()
        assert plane[6].cpu().tolist() == [1, 1] and plane[4].cpu().tolist() == [600, 600]
        got = _gicp(pm, q, Td, r2, nrm, nq)
        worst, worst_res = _check(got, T, want, "flat")
        assert got[6].tolist() == [0, 0] and got[4].tolist() == [600, 600]
        print(f"flat model: worst |T_step - reference| {worst:.3e}, sum_res2 off by {worst_res:.2e} relative")
    finally:
        pm.close()


def test_three_steps_on_the_device_at_the_host_tier_and_against_the_reference():
    """check 6"""
    import pcreg_amd as pc
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"], sc["T"], sc["normals"]
    sn = gicp_ref.surface_normals()
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _nrm(normals), _nrm(sn)
        three = _gicp(pm, q, Td, R15, nrm, nq, steps=3)
        cur, singles = Td, []
        for k in range(3):
            out = pm.refit_gicp(q, cur, R15, nrm, nq)
            cur = out[0].clone()                                           # fed back on the device
            torch.cuda.synchronize()
            singles.append(tuple(t.cpu().numpy() for t in out))
        last = singles[-1]
        _same(three, (_m44(last[0]), _m44(last[1])) + last[2:])
        keys = ("T", "n_close", "sum_d2", "n_pairs", "sum_res2", "empty")
        with pc.Model(model) as h, pc.Model(surf) as hs:
            r = h.refit_gicp(surf, T, R15, steps=3, normals=normals, query_normals=sn)
            _same(tuple(r[key] for key in keys), (three[0],) + three[2:6] + (three[6] != 0,))
            # both sets of normals computed inside the call (k = 8) against the same call on Model.normals(8) of either cloud
            own, own_q = h.normals(8), hs.normals(8)
            a = h.refit_gicp(surf, T, R15, steps=3, k=8)
            for kw in (dict(normals=own, query_normals=own_q), dict(normals=own, k=8), dict(query_normals=own_q, k=8)):
                b = h.refit_gicp(surf, T, R15, steps=3, **kw)
                assert sorted(a) == sorted(b)
                _same(tuple(np.asarray(a[key]) for key in sorted(a)), tuple(np.asarray(b[key]) for key in sorted(b)))
            assert not a["empty"][:4].any() and a["empty"][4:].all()
        # every step against the reference's step on the bits the device gave that step
        T_in = T
        for k in range(3):
            want = gicp_ref.step(surf, model, normals, sn, T_in, R15, threads=CORES)
            got = (_m44(singles[k][0]), _m44(singles[k][1])) + singles[k][2:]
            worst, worst_res = _check(got, T_in, want, f"step {k + 1}")
            print(f"step {k + 1}: n_pairs {got[4].tolist()}, worst |T_step - reference| {worst:.3e}, sum_res2 off by {worst_res:.2e} relative")
            T_in = got[0]
        assert (singles[2][6] == [0, 0, 0, 0, 1, 1]).all()                 # a failed candidate stays failed
    finally:
        pm.close()


def test_refine_trials_with_both_normals_runs_this_step():
    """check 7"""
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, nrm, nq = _soa(surf), _nrm(sc["normals"]), _nrm(gicp_ref.surface_normals())
        result = dict(trial=np.array([4, 9, 11]), transforms=[pc.invertTF(T[1]), None, pc.invertTF(T[3])])
        inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
        for eps in (1e-3, 1e-2):
            direct = _gicp(pm, q, _t16(inv), R15, nrm, nq, epsilon=eps, steps=2)
            out, summary = refine_trials(result, pm, q, 1.5, steps=2, normals=nrm, surface_normals=nq, epsilon=eps)
            assert len(out) == 3 and out[1] is None and direct[6].tolist() == [0, 1, 0]
            for t in (0, 2):
                np.testing.assert_array_equal(out[t], pc.invertTF(direct[0][t]))
            np.testing.assert_array_equal(summary["n_close"], direct[2])
            np.testing.assert_array_equal(summary["sum_d2"].view(np.uint64), direct[3].view(np.uint64))
        # with the model's normals alone: still the point-to-plane step
        plane = pm.refit_plane(q, _t16(inv), R15, nrm, steps=2)
        torch.cuda.synchronize()
        out, _summary = refine_trials(result, pm, q, 1.5, steps=2, normals=nrm)
        for t in (0, 2):
            np.testing.assert_array_equal(out[t], pc.invertTF(_m44(plane[0].cpu().numpy())[t]))
        assert not np.array_equal(out[0], pc.invertTF(direct[0][0]))
        assert refine_trials(dict(trial=[], transforms=[]), pm, q, 1.5, normals=nrm, surface_normals=nq)[0] == []
    finally:
        pm.close()


def test_edges_and_argument_errors():
    """check 8"""
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, PcregError, check, lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T, normals = sc["model"], sc["surf"][:300], sc["T"][:4], sc["normals"]
    sn = gicp_ref.surface_normals()[:300]
    M = len(model)
    want = gicp_ref.step(surf, model, normals, sn, T, R15, threads=CORES)
    pm, _t = _prepared(model)
    pm0, _t0 = _prepared(model[:0])
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _nrm(normals), _nrm(sn)
        got = _gicp(pm, q, Td, R15, nrm, nq)
        _check(got, T, want, "300 queries")
        # Q = 0, and a model without rows: every transform empty, the counts and sums 0
        n0 = torch.zeros((3, 0), dtype=torch.float32, device=_dev())
        for g in (_gicp(pm, _soa(surf[:0]), Td, R15, nrm, n0), _gicp(pm0, q, Td, R15, n0, nq), _gicp(pm0, _soa(surf[:0]), Td, R15, n0, n0)):
            assert g[2].tolist() == [0] * 4 and g[3].tolist() == [0.0] * 4 and g[4].tolist() == [0] * 4 and g[5].tolist() == [0.0] * 4
            assert g[6].tolist() == [1] * 4 and not g[0].any() and not g[1].any()
        # B = 0 through the C ABI: nothing is written into canary-filled outputs
        canary_d = torch.full((48,), -7.0, dtype=torch.float64, device=_dev())
        canary_i = torch.full((12,), -7, dtype=torch.int32, device=_dev())
        assert L.pcreg_dev_model_refit_gicp_workspace(300, 4, M) == L.pcreg_dev_model_refit_plane_workspace(300, 4, M)
        ws0 = torch.empty(int(L.pcreg_dev_model_refit_gicp_workspace(300, 0, M)), dtype=torch.uint8, device=_dev())
        check(L.pcreg_dev_model_refit_gicp_f32(pm.handle, q.data_ptr(), 300, 300, None, 0, 1.0, nrm.data_ptr(), M, nq.data_ptr(), 300, 1e-3,
                                               canary_d.data_ptr(), canary_d[16:].data_ptr(), canary_i.data_ptr(), canary_d[32:].data_ptr(),
                                               canary_i[4:].data_ptr(), canary_d[40:].data_ptr(), canary_i[8:].data_ptr(), ws0.data_ptr(), ws0.numel(), None))
        torch.cuda.synchronize()
        assert canary_d.tolist() == [-7.0] * 48 and canary_i.tolist() == [-7] * 12
        assert pm.refit_gicp(q, Td[:0], R15, nrm, nq)[0].shape == (0, 16)
        # T_step = NULL: the other outputs are the same bits
        To = torch.empty((4, 16), dtype=torch.float64, device=_dev())
        n, npr, e = (torch.empty(4, dtype=torch.int32, device=_dev()) for _ in range(3))
        s, res = (torch.empty(4, dtype=torch.float64, device=_dev()) for _ in range(2))
        need = int(L.pcreg_dev_model_refit_gicp_workspace(300, 4, M))
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(Q=300, ldq=300, B=4, r2=float(R15), wsb=need, qp=q.data_ptr(), tp=Td.data_ptr(), h=pm.handle, op=To.data_ptr(), ep=e.data_ptr(),
                 nr=nrm.data_ptr(), ldn=M, pp=npr.data_ptr(), rp=res.data_ptr(), qn=nq.data_ptr(), ldnq=300, eps=1e-3):
            return L.pcreg_dev_model_refit_gicp_f32(h, qp, Q, ldq, tp, B, r2, nr, ldn, qn, ldnq, eps, op, None, n.data_ptr(), s.data_ptr(), pp, rp, ep,
                                                    ws.data_ptr(), wsb, None)
        assert call() == PCREG_OK
        torch.cuda.synchronize()
        _same((_m44(To.cpu().numpy()),) + tuple(t.cpu().numpy() for t in (n, s, npr, res, e)), (got[0],) + got[2:])
        for kw in (dict(r2=float("nan")), dict(r2=-1.0), dict(r2=float("-inf")), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1, ldnq=(4 << 20) + 1, wsb=1 << 40),
                   dict(B=-1), dict(Q=-1), dict(ldq=299), dict(wsb=need - 1), dict(qp=None), dict(tp=None), dict(h=None), dict(op=None), dict(ep=None),
                   dict(pp=None), dict(rp=None), dict(nr=None), dict(ldn=M - 1), dict(ldn=-1), dict(op=Td.data_ptr()),
                   dict(qn=None), dict(ldnq=299), dict(ldnq=-1), dict(eps=float("nan")), dict(eps=0.0), dict(eps=-1e-3), dict(eps=1.0000001),
                   dict(eps=float("inf"))):
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        assert call(r2=float("inf")) == PCREG_OK and call(r2=0.0) == PCREG_OK and call(eps=1.0) == PCREG_OK and call(eps=5e-324) == PCREG_OK
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            pm.refit_gicp(q, Td, -1.0, nrm, nq)
        with pytest.raises(ValueError):
            pm.refit_gicp(q, Td, 1.0, nrm, nq, steps=0)
        with pytest.raises(ValueError):
            pm.refit_gicp(q, Td, 1.0, nrm, nq, epsilon=0.0)
        with pytest.raises(TypeError):
            pm.refit_gicp(q, Td.float(), 1.0, nrm, nq)
        with pytest.raises(TypeError):
            pm.refit_gicp(q, Td, 1.0, nrm[:, :100], nq)
        with pytest.raises(TypeError):
            pm.refit_gicp(q, Td, 1.0, nrm, nq[:, :100])
        # the host tier
        with pc.Model(model) as h:
            out, ss, rr = np.zeros((4, 16)), np.zeros(4), np.zeros(4)
            nn, pp, ee = (np.zeros(4, np.int32) for _ in range(3))
            T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
            qs, ns, nqs = np.asfortranarray(surf), np.asfortranarray(normals), np.asfortranarray(sn)

            def args(steps=1, r2=float(R15), nr=ns.ctypes.data, ldn=M, qn=nqs.ctypes.data, ldnq=300, k=6, eps=1e-3):
                return (h._h, qs.ctypes.data, 300, 300, T16.ctypes.data, 4, r2, steps, nr, ldn, qn, ldnq, k, eps, out.ctypes.data, nn.ctypes.data,
                        ss.ctypes.data, pp.ctypes.data, rr.ctypes.data, ee.ctypes.data)
            f = L.pcreg_model_refit_gicp_f32
            assert f(*args(0)) == PCREG_E_ARG and f(*args(-1)) == PCREG_E_ARG
            assert f(*args(1, float("nan"))) == PCREG_E_ARG and f(*args(1, -1.0)) == PCREG_E_ARG
            assert f(*args(ldn=M - 1)) == PCREG_E_ARG and f(*args(ldn=-1)) == PCREG_E_ARG
            assert f(*args(ldnq=299)) == PCREG_E_ARG and f(*args(ldnq=-1)) == PCREG_E_ARG
            for eps in (float("nan"), 0.0, -0.5, 1.5):
                assert f(*args(eps=eps)) == PCREG_E_ARG, eps
            for k in (2, 33, 0, -1):
                assert f(*args(nr=None, k=k)) == PCREG_E_ARG and f(*args(qn=None, k=k)) == PCREG_E_ARG, k
            assert f(*args(k=-5)) == PCREG_OK                                              # both given: k is ignored
            _same((_m44(out), nn, ss, pp, rr, ee), (got[0],) + got[2:])
            with pytest.raises(ValueError):
                h.refit_gicp(surf, T, 1.0, steps=0)
            with pytest.raises(ValueError):
                h.refit_gicp(surf, T, 1.0, k=2)
            with pytest.raises(ValueError):
                h.refit_gicp(surf, T, 1.0, epsilon=2.0)
            with pytest.raises(ValueError):
                h.refit_gicp(surf, T, 1.0, normals=normals[:100])
            with pytest.raises(ValueError):
                h.refit_gicp(surf, T, 1.0, query_normals=sn[:100])
            with pytest.raises((ValueError, PcregError)):
                h.refit_gicp(surf, T, -1.0)
            r = h.refit_gicp(surf, T, R15, normals=normals, query_normals=sn)
            _same((r["T"], r["n_close"], r["sum_d2"], r["n_pairs"], r["sum_res2"], r["empty"]), (got[0],) + got[2:6] + (got[6] != 0,))
            np.testing.assert_array_equal(r["pair_rmse"][:4], np.sqrt(got[5] / got[4]))
            r = h.refit_gicp(surf[:0], T, R15)                                             # no queries at the host tier, normals and all
            assert r["empty"].all() and not r["T"].any() and not r["n_pairs"].any()
        with pc.Model(model[:0]) as h0:                                                    # a model without rows at the host tier
            r = h0.refit_gicp(surf, T, R15)
            assert r["empty"].all() and not r["T"].any() and not r["n_pairs"].any() and np.isnan(r["pair_rmse"]).all()
    finally:
        pm.close()
        pm0.close()


def test_two_streams_on_one_handle():
    """check 8: each call with its own workspace and outputs"""
    from pcreg_amd._lib import lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _nrm(sc["normals"]), _nrm(gicp_ref.surface_normals())
        halves = ((q[:, :2000].contiguous(), Td[:4].contiguous(), nq[:, :2000].contiguous()), (q[:, 400:].contiguous(), Td[2:].contiguous(), nq[:, 400:].contiguous()))
        want = []
        for a, b, c in halves:
            out = pm.refit_gicp(a, b, R15, nrm, c, steps=2)
            torch.cuda.synchronize()
            want.append(tuple(t.cpu().numpy() for t in out))
        outs = []
        for a, b, _c in halves:
            Qh, Bh = a.shape[1], b.shape[0]
            d64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=_dev())
            i32 = lambda: torch.empty(Bh, dtype=torch.int32, device=_dev())
            outs.append((d64(Bh, 16), d64(Bh, 16), i32(), d64(Bh), i32(), d64(Bh), i32(),
                         torch.empty(int(L.pcreg_dev_model_refit_gicp_workspace(Qh, Bh, pm.M)), dtype=torch.uint8, device=_dev()), d64(Bh, 16)))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, (a, b, c), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.refit_gicp(a, b, R15, nrm, c, steps=2, out=o)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            _same(tuple(t.cpu().numpy() for t in o[:7]), w)
    finally:
        pm.close()
