"""Candidate transforms refitted on their close dense pairs (knn_score.hip + ransac.hip) on the GPU.

n_close and the bits of sum_d2 against score_transforms on the same inputs; empty, T_step and T_out against tests/refit_ref.py
(score_ref's pairs, the oracle's estimateTransform in double, the composition restated entry by entry); the same bits twice, with
culling off and in three batches; exactly k = 0 .. 5 pairs, three of them across a chunk boundary; a rank-deficient set; the edges
(ldq > Q, Q = 0, B = 0, a model without rows, no T_step, the workspace formula, argument errors); three steps on the device, at the
host tier and against the reference step by step; refine_trials; two streams on one handle; the synth(120 000, 3000) case.

The bound on T_step, 1e-9 in the Frobenius norm, is the one test_estimate_transform_indexed_against_the_oracle and the
distance-refine test use at these coordinate magnitudes (tens of units, thousands of pairs); two oracle fits of the main scene's
pairs in ascending and in shuffled order differ by 1.1e-15 at most, seven orders below it.  It is asserted only where the centred
cross-covariance of the pairs has its smallest singular value above 1e-3 of its largest (computed here with numpy and asserted
as the premise): the rotation of a nearly rank-deficient set is ill-conditioned in any arithmetic."""
import os

import numpy as np
import pytest
import torch

import refit_ref
import score_ref
from oracle.pcreg_oracle import estimateTransform, eul2rotm, invertTF
from test_gpu_range import _dev, _prepared, _soa, _stats

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
BOUND = 1e-9
R15 = np.float32(1.5) ** 2
RADII = [np.float32(0.0), np.float32(0.5) ** 2, R15, np.float32(np.inf)]


def _rigid(eul, shift):
    T = np.eye(4)
    T[:3, :3] = eul2rotm(eul)
    T[3, :3] = shift
    return T


def _t16(T):
    """[B, 4, 4] -> the [B, 16] block on the device, each transform column-major"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    return torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)).to(_dev())


def _m44(t16):
    """the [B, 16] block -> [B, 4, 4] as quickTF uses them"""
    return np.ascontiguousarray(np.asarray(t16, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))


def _refit(pm, q, Td, r2, steps=1):
    """-> T_out [B, 4, 4], T_step [B, 4, 4], n_close, sum_d2, empty as numpy"""
    out = pm.refit_transforms(q, Td, r2, steps=steps)
    torch.cuda.synchronize()
    T_out, T_step, n, s, e = (t.cpu().numpy() for t in out)
    return _m44(T_out), _m44(T_step), n, s, e


def _score(pm, q, Td, r2):
    out = pm.score_transforms(q, Td, r2)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same(a, b):
    """the bits of everything"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _check(got, T, want, model, r2, what=""):
    """assertions 2, 3 and 4 for one call: `want` is refit_ref.step on the bits of T that the device was given"""
    T_out, T_step, n, s, e = got
    np.testing.assert_array_equal(n, want["n_close"])
    np.testing.assert_array_equal(e != 0, want["empty"])
    assert set(np.unique(e).tolist()) <= {0, 1}
    worst = 0.0
    for b in range(len(T)):
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any(), b              # all 32 numbers are 0.0
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        if np.isfinite(r2):
            sv = refit_ref.cross_covariance_singular_values(model, want["idx"][b], want["tq"][b])
            assert sv[-1] > 1e-3 * sv[0], (what, b, sv)                        # the premise of the bound
            err = float(np.linalg.norm(T_step[b] - want["T_step"][b]))
            print(f"  {what} b = {b}: n_close {n[b]}, |T_step - oracle| = {err:.3e}, singular values {sv}")
            assert err < BOUND, (what, b, err)
            worst = max(worst, err)
    return worst


_SCENE = {}


def _scene():
    """the main scene: 3000 model rows in [-20, 20]^3, 2200 of them plus N(0, 0.02^2) and 300 uniform points moved by the rigid G;
    candidates invertTF(G) times four perturbations, the empty transform and one with a NaN entry.  The reference's step is
    computed once per radius and shared."""
    if _SCENE:
        return _SCENE
    rng = np.random.default_rng(7)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    on = model[rng.choice(3000, 2200, replace=False)].astype(np.float64) + rng.normal(0, 0.02, (2200, 3))
    cloud = np.vstack([on, rng.uniform(-20, 20, (300, 3))])
    G = _rigid([0.3, -0.2, 0.5], [4, -3, 2])
    surf = (cloud @ G[:3, :3] + G[3, :3]).astype(np.float32)
    back = invertTF(G)
    pert = [np.eye(4), _rigid([0.004, -0.003, 0.005], [0.05, -0.04, 0.03]), _rigid([0.01, 0.008, -0.012], [0.15, 0.1, -0.12]),
            _rigid([0.03, -0.02, 0.025], [0.4, -0.3, 0.35])]
    T = np.stack([back @ p for p in pert] + [np.zeros((4, 4)), back.copy()])
    T[5, 1, 2] = np.nan
    _SCENE.update(model=model, surf=surf, T=T, ref={})
    return _SCENE


def _scene_ref(r2):
    sc = _scene()
    key = float(r2)
    if key not in sc["ref"]:
        sc["ref"][key] = refit_ref.step(sc["surf"], sc["model"], sc["T"], r2, threads=CORES)
    return sc["ref"][key]


def test_the_scene_is_what_the_checks_need():
    """premises, from the reference alone: two chunks, five query blocks, six tiles; thousands of pairs for the four rigid
    candidates at r = 1.5 and none for the empty and the NaN one; the oracle's own sensitivity to the order of the pairs"""
    sc = _scene()
    Q, M = len(sc["surf"]), len(sc["model"])
    assert (Q + 2047) // 2048 == 2 and (Q + 511) // 512 == 5 and (M + 511) // 512 == 6
    want = _scene_ref(R15)
    print("close points per candidate", want["n_close"].tolist())
    assert (want["n_close"][:4] > 2000).all() and (want["n_close"][4:] == 0).all()
    assert want["empty"].tolist() == [False] * 4 + [True] * 2
    rng = np.random.default_rng(1)
    for b in range(4):
        hit = np.flatnonzero(want["hit"][b])
        sh = rng.permutation(hit)
        a = estimateTransform(sc["model"][want["idx"][b][sh]].astype(np.float64), want["tq"][b][sh].astype(np.float64))
        d = float(np.linalg.norm(a - want["T_step"][b]))
        print(f"  b = {b}: ascending against shuffled pairs in the oracle: {d:.3e}")
        assert d < 1e-13


@pytest.mark.parametrize("r2", RADII, ids=["r0", "r0.5", "r1.5", "rinf"])
def test_counts_are_scorings_bits_and_the_fit_is_the_oracles(r2, debug_set):
    """assertions 1-5 on the main scene"""
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    Q = len(surf)
    want = _scene_ref(r2)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _refit(pm, q, Td, r2)
        n, s = _score(pm, q, Td, r2)
        np.testing.assert_array_equal(got[2], n)                                           # 1
        np.testing.assert_array_equal(got[3].view(np.uint64), s.view(np.uint64))
        worst = _check(got, T, want, model, r2, f"r2 = {float(r2):.4g}")                   # 2, 3, 4
        print(f"r2 = {float(r2):.4g}: n_close {got[2].tolist()}, empty {got[4].tolist()}, worst |T_step - oracle| {worst:.3e}")
        if r2 == R15:
            assert got[4].tolist() == [0, 0, 0, 0, 1, 1]
        _same(_refit(pm, q, Td, r2), got)                                                  # 5: twice
        debug_set("knn_nocull", 1)
        g0 = _refit(pm, q, Td, r2)
        debug_set("knn_nocull", 0)
        _same(g0, got)
        debug_set("knn_stats", 1)
        _stats(reset=True)
        debug_set("score_batch_slots", 2 * Q)
        g1 = _refit(pm, q, Td, r2)
        st = _stats(reset=True)
        debug_set("score_batch_slots", 0)
        assert st[0] == 3, st                                                              # premise: 2 + 2 + 2 transforms
        _same(g1, got)
    finally:
        pm.close()


def _few(k):
    """a model of 3000 rows and a cloud of 2500 points of which exactly k are copies of model rows, the rest model rows shifted
    out of reach; k = 3 puts the copies at queries 5, 2047 and 2048, on both sides of the chunk boundary"""
    rng = np.random.default_rng(20 + k)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.float32(100.0)).astype(np.float32)
    at = [5, 2047, 2048] if k == 3 else sorted(rng.choice(2500, k, replace=False).tolist())
    rows = rng.choice(3000, k, replace=False)
    for i, r in zip(at, rows):
        surf[i] = model[r]
    return model, surf, at, rows


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_exactly_k_pairs(k):
    """assertion 6: r2 = 0 under the identity and a second, slightly moved candidate that meets nothing"""
    model, surf, at, rows = _few(k)
    T = np.stack([np.eye(4), _rigid([0.001, 0.0, 0.0], [0.01, 0.0, 0.0])])
    want = refit_ref.step(surf, model, T, 0.0, threads=CORES)
    assert want["n_close"].tolist() == [k, 0] and np.flatnonzero(want["hit"][0]).tolist() == at          # premise
    assert want["idx"][0][at].tolist() == rows.tolist()
    assert want["empty"].tolist() == [k < 3, True]
    pm, _t = _prepared(model)
    try:
        got = _refit(pm, _soa(surf), _t16(T), 0.0)
        _check(got, T, want, model, 0.0, f"k = {k}")
        if k == 3:                                      # the oracle's synthetic-fourth-point branch, on three pairs from two chunks
            assert at == [5, 2047, 2048]
            S = estimateTransform(model[rows].astype(np.float64), surf[at].astype(np.float64))
            assert np.linalg.norm(got[1][0] - S) < BOUND
    finally:
        pm.close()


def test_hits_in_a_plane_through_the_origin_are_empty():
    """assertion 7: rank(pts1) < 3 (estimateTransform.m:11)"""
    rng = np.random.default_rng(31)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    flat = rng.choice(3000, 60, replace=False)
    model[flat, 2] = 0.0
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.float32(100.0)).astype(np.float32)
    at = np.sort(rng.choice(2500, 60, replace=False))
    surf[at] = model[flat]
    T = np.eye(4)[None]
    want = refit_ref.step(surf, model, T, 0.0, threads=CORES)
    assert want["n_close"].tolist() == [60] and want["empty"].tolist() == [True]                          # the oracle premise
    assert estimateTransform(model[flat].astype(np.float64), model[flat].astype(np.float64)) is None
    pm, _t = _prepared(model)
    try:
        got = _refit(pm, _soa(surf), _t16(T), 0.0)
        assert got[2].tolist() == [60] and got[4].tolist() == [1] and not got[0].any() and not got[1].any()
    finally:
        pm.close()


def test_edges_and_argument_errors():
    """assertion 8"""
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, PcregError, check, lib
    L = lib()
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"][:300], sc["T"][:4]
    want = refit_ref.step(surf, model, T, R15, threads=CORES)
    pm, _t = _prepared(model)
    pm0, _t0 = _prepared(model[:0])
    try:
        q, Td = _soa(surf), _t16(T)
        got = _refit(pm, q, Td, R15)
        _check(got, T, want, model, R15, "300 queries")
        # ldq > Q: the queries are columns 100 .. 399 of a wider buffer
        wide = torch.full((3, 1000), 1e30, dtype=torch.float32, device=_dev())
        wide[:, 100:400] = q
        qw = wide[:, 100:400]
        assert qw.stride(0) == 1000
        _same(_refit(pm, qw, Td, R15), got)
        # Q = 0, and a model without rows: every transform empty, the counts 0
        for g in (_refit(pm, _soa(surf[:0]), Td, R15), _refit(pm0, q, Td, R15), _refit(pm0, _soa(surf[:0]), Td, R15)):
            assert g[2].tolist() == [0] * 4 and g[3].tolist() == [0.0] * 4 and g[4].tolist() == [1] * 4 and not g[0].any() and not g[1].any()
        # B = 0 through the C ABI: nothing is written into canary-filled outputs
        canary_d = torch.full((32,), -7.0, dtype=torch.float64, device=_dev())
        canary_i = torch.full((8,), -7, dtype=torch.int32, device=_dev())
        need0 = int(L.pcreg_dev_model_refit_workspace(300, 0, pm.M))
        ws0 = torch.empty(need0, dtype=torch.uint8, device=_dev())
        check(L.pcreg_dev_model_refit_f32(pm.handle, q.data_ptr(), 300, 300, None, 0, 1.0, canary_d.data_ptr(), canary_d[16:].data_ptr(),
                                          canary_i.data_ptr(), canary_d.data_ptr(), canary_i[4:].data_ptr(), ws0.data_ptr(), ws0.numel(), None))
        torch.cuda.synchronize()
        assert canary_d.tolist() == [-7.0] * 32 and canary_i.tolist() == [-7] * 8
        assert pm.refit_transforms(q, Td[:0], R15)[0].shape == (0, 16)
        # T_step = NULL: the other outputs are the same bits
        To = torch.empty((4, 16), dtype=torch.float64, device=_dev())
        n = torch.empty(4, dtype=torch.int32, device=_dev())
        s = torch.empty(4, dtype=torch.float64, device=_dev())
        e = torch.empty(4, dtype=torch.int32, device=_dev())
        need = int(L.pcreg_dev_model_refit_workspace(300, 4, pm.M))
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(Q=300, ldq=300, B=4, r2=float(R15), wsb=need, qp=q.data_ptr(), tp=Td.data_ptr(), h=pm.handle, op=To.data_ptr(), ep=e.data_ptr()):
            return L.pcreg_dev_model_refit_f32(h, qp, Q, ldq, tp, B, r2, op, None, n.data_ptr(), s.data_ptr(), ep, ws.data_ptr(), wsb, None)
        assert call() == PCREG_OK
        torch.cuda.synchronize()
        _same((_m44(To.cpu().numpy()), n.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()), (got[0], got[2], got[3], got[4]))
        for kw in (dict(r2=float("nan")), dict(r2=-1.0), dict(r2=float("-inf")), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1, wsb=1 << 40), dict(B=-1),
                   dict(Q=-1), dict(ldq=299), dict(wsb=need - 1), dict(qp=None), dict(tp=None), dict(h=None), dict(op=None), dict(ep=None),
                   dict(op=Td.data_ptr())):                                   # ... and T_out aliasing T_dev
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        assert call(r2=float("inf")) == PCREG_OK and call(r2=0.0) == PCREG_OK
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            pm.refit_transforms(q, Td, -1.0)
        with pytest.raises(ValueError):
            pm.refit_transforms(q, Td, 1.0, steps=0)
        with pytest.raises(TypeError):
            pm.refit_transforms(q, Td.float(), 1.0)
        # the host tier: steps = 0 is an argument error at the C entry and in Python
        with pc.Model(model) as h:
            out, nn, ss, ee = np.zeros((4, 16)), np.zeros(4, np.int32), np.zeros(4), np.zeros(4, np.int32)
            T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
            qs = np.asfortranarray(surf)
            args = lambda steps, r2=float(R15): (h._h, qs.ctypes.data, 300, 300, T16.ctypes.data, 4, r2, steps, out.ctypes.data, nn.ctypes.data,
                                                 ss.ctypes.data, ee.ctypes.data)
            assert L.pcreg_model_refit_f32(*args(0)) == PCREG_E_ARG and L.pcreg_model_refit_f32(*args(-1)) == PCREG_E_ARG
            assert L.pcreg_model_refit_f32(*args(1, float("nan"))) == PCREG_E_ARG and L.pcreg_model_refit_f32(*args(1, -1.0)) == PCREG_E_ARG
            assert L.pcreg_model_refit_f32(*args(1)) == PCREG_OK
            _same((_m44(out), nn, ss, ee), (got[0], got[2], got[3], got[4]))
            with pytest.raises(ValueError):
                h.refit_transforms(surf, T, 1.0, steps=0)
            with pytest.raises((ValueError, PcregError)):
                h.refit_transforms(surf, T, -1.0)
    finally:
        pm.close()
        pm0.close()
    # include/pcreg.h: scoring's nb, S and P; 131 328 + 2 roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256)
    # + roundup(216 P, 256)
    up = lambda x: (x + 255) // 256 * 256
    for Q, B in ((0, 0), (1, 1), (2500, 6), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        nb = max(1, min(B, (4 << 20) // max(Q, 1)))
        S, P = max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)
        formula = 131_328 + 2 * up(12 * S) + 2 * up(4 * S) + up(8 * P) + up(4 * P) + up(216 * P)
        assert L.pcreg_dev_model_refit_workspace(Q, B, 0) == L.pcreg_dev_model_refit_workspace(Q, B, 1 << 20) == formula, (Q, B)
        assert formula == L.pcreg_dev_model_score_workspace(Q, B, 0) + up(12 * S) + up(216 * P)
    assert "131 328 + 2 roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256) + roundup(216 P, 256) bytes" in \
        open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcreg.h")).read()


def test_three_steps_on_the_device_at_the_host_tier_and_against_the_reference():
    """assertion 9"""
    import pcreg_amd as pc
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        three = _refit(pm, q, Td, R15, steps=3)
        cur, singles = Td, []
        for k in range(3):
            out = pm.refit_transforms(q, cur, R15)
            cur = out[0].clone()                                           # fed back on the device
            torch.cuda.synchronize()
            singles.append(tuple(t.cpu().numpy() for t in out))
        last = singles[-1]
        _same(three, (_m44(last[0]), _m44(last[1])) + last[2:])
        with pc.Model(model) as h:
            r = h.refit_transforms(surf, T, R15, steps=3)
        _same((r["T"], r["n_close"], r["sum_d2"], r["empty"]), (three[0], three[2], three[3], three[4] != 0))
        # every step against the reference's step on the bits the device gave that step
        T_in = T
        for k in range(3):
            want = refit_ref.step(surf, model, T_in, R15, threads=CORES)
            got = (_m44(singles[k][0]), _m44(singles[k][1])) + singles[k][2:]
            worst = _check(got, T_in, want, model, R15, f"step {k + 1}")
            print(f"step {k + 1}: n_close {got[2].tolist()}, worst |T_step - oracle| {worst:.3e}")
            T_in = got[0]
        assert (singles[2][4] == [0, 0, 0, 0, 1, 1]).all()                 # a failed candidate stays failed
        # one step lowers the inlier RMSE of the three perturbed candidates: first in the reference, then on the device
        first = _scene_ref(R15)
        after = score_ref.score(surf, model, first["T_out"][:4], R15, threads=CORES)
        ref_before = np.sqrt(first["sum_d2"][:4] / first["n_close"][:4])
        ref_after = np.sqrt(after[3] / after[2])
        print("reference RMSE before", ref_before.tolist(), "after one step", ref_after.tolist())
        assert (ref_after[1:] < ref_before[1:]).all()                      # the premise
        n0, s0 = _score(pm, q, Td, R15)
        n1, s1 = _score(pm, q, _t16(_m44(singles[0][0])), R15)
        before, now = np.sqrt(s0[:4] / n0[:4]), np.sqrt(s1[:4] / n1[:4])
        print("device RMSE before", before.tolist(), "after one step", now.tolist())
        assert (now[1:] < before[1:]).all()
    finally:
        pm.close()


def test_refine_trials_keeps_the_orientation_and_the_failed_trial():
    """assertion 10"""
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials, score_trials
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q = _soa(surf)
        result = dict(trial=np.array([4, 9, 11]), transforms=[pc.invertTF(T[1]), None, pc.invertTF(T[3])])
        inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
        direct = _refit(pm, q, _t16(inv), R15, steps=2)
        out, summary = refine_trials(result, pm, q, 1.5, steps=2)
        assert len(out) == 3 and out[1] is None and direct[4].tolist() == [0, 1, 0]
        for t in (0, 2):
            np.testing.assert_array_equal(out[t], pc.invertTF(direct[0][t]))
            assert np.linalg.norm(pc.invertTF(out[t]) - direct[0][t]) < 1e-12          # the round trip
        np.testing.assert_array_equal(summary["n_close"], direct[2])
        np.testing.assert_array_equal(summary["sum_d2"].view(np.uint64), direct[3].view(np.uint64))
        assert summary["n_close"][1] == 0 and np.isnan(summary["rmse"][1]) and len(summary["fitness"]) == 3
        # the refined trials score better than the trials
        was = score_trials(result, pm, q, 1.5)
        now = score_trials(dict(trial=result["trial"], transforms=out), pm, q, 1.5)
        assert (now["rmse"][[0, 2]] < was["rmse"][[0, 2]]).all()
        assert refine_trials(dict(trial=[], transforms=[]), pm, q, 1.5)[0] == []
    finally:
        pm.close()


def test_two_streams_on_one_handle():
    """assertion 11: each call with its own workspace and outputs"""
    from pcreg_amd._lib import lib
    L = lib()
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        halves = ((q[:, :2000].contiguous(), Td[:4].contiguous()), (q[:, 400:].contiguous(), Td[2:].contiguous()))
        want = []
        for a, b in halves:
            out = pm.refit_transforms(a, b, R15, steps=2)
            torch.cuda.synchronize()
            want.append(tuple(t.cpu().numpy() for t in out))
        outs = []
        for a, b in halves:
            Qh, Bh = a.shape[1], b.shape[0]
            outs.append((torch.empty((Bh, 16), dtype=torch.float64, device=_dev()), torch.empty((Bh, 16), dtype=torch.float64, device=_dev()),
                         torch.empty(Bh, dtype=torch.int32, device=_dev()), torch.empty(Bh, dtype=torch.float64, device=_dev()),
                         torch.empty(Bh, dtype=torch.int32, device=_dev()),
                         torch.empty(int(L.pcreg_dev_model_refit_workspace(Qh, Bh, pm.M)), dtype=torch.uint8, device=_dev()),
                         torch.empty((Bh, 16), dtype=torch.float64, device=_dev())))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, (a, b), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.refit_transforms(a, b, R15, steps=2, out=o)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            _same(tuple(t.cpu().numpy() for t in o[:5]), w)
    finally:
        pm.close()


def test_the_synth_case(debug_set):
    """assertion 12: tests/test_gpu_score.py's synth(120 000, 3000) case (2500 of its surface points and 500 model rows), the
    identity and the small motion at r = 1.5: assertions 1, 3 and 5"""
    from bench import synth
    model, surf, _ = synth(120_000, 3000)
    model, surf = np.asarray(model, np.float32), np.asarray(surf, np.float32)[:2500]
    own = np.random.default_rng(4).choice(len(model), 500, replace=False)
    surf = np.vstack([surf, model[own]]).astype(np.float32)
    Q = len(surf)
    T = np.tile(np.eye(4), (2, 1, 1))
    a = np.array([0.004, -0.003, 0.005])
    T[1, :3, :3] += np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T[1, 3, :3] = [0.05, -0.04, 0.03]
    want = refit_ref.step(surf, model, T, R15, threads=CORES)
    assert (want["n_close"] > Q // 2).all() and not want["empty"].any()
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _refit(pm, q, Td, R15)
        n, s = _score(pm, q, Td, R15)
        np.testing.assert_array_equal(got[2], n)
        np.testing.assert_array_equal(got[3].view(np.uint64), s.view(np.uint64))
        worst = _check(got, T, want, model, R15, "synth")
        print(f"synth: n_close {got[2].tolist()}, worst |T_step - oracle| {worst:.3e}")
        _same(_refit(pm, q, Td, R15), got)
        debug_set("knn_nocull", 1)
        g0 = _refit(pm, q, Td, R15)
        debug_set("knn_nocull", 0)
        _same(g0, got)
        debug_set("knn_stats", 1)
        _stats(reset=True)
        debug_set("score_batch_slots", Q)
        g1 = _refit(pm, q, Td, R15)
        st = _stats(reset=True)
        debug_set("score_batch_slots", 0)
        assert st[0] == 2, st
        _same(g1, got)
    finally:
        pm.close()
