"""Candidate transforms refitted by the coherent-point-drift step (cpd.hip + cpd_fit.hpp) on the GPU.

The reference is tests/cpd_ref.py: step_ld, the contract in longdouble.  THE BOUND of every inexact output is 8 x E_method, where
E_method = |step32 - step_ld| is recomputed here on the CPU for the very inputs of the call (step32: the contract's fp32
arithmetic restated in numpy with a correctly rounded exp2 and sequential sums), per OUTPUT: the worst over the call's candidates
(tests/cpd_ref.py: method_error says why), and never below E_FLOOR = 2^-49, what the double arithmetic after the fp32 sums costs by
itself (with w = 0 the two CPU computations give Np to the last bit).  The
device's exp2 may be a unit or two in the last place off, and its fp32 sums are slices and its double sums trees where step32's are
sequences; both are of the order of the rounding E_method already contains, and 8 is the margin for them.
EMPTY is exact wherever step_ld and step32 give the same verdict; where the two CPU computations of one contract disagree, the
verdict lies inside the method error (a handful of queries decide the candidate) and either is accepted.
Exact besides: n_live; sum_d2, the bits score_transforms gives at r2 = +inf; T_out, the restated product of T and the reported T_step.

MEASURED on one MI355X, the worst share of the bound: 0.157 over the main scene's six cases (sum_res2 at w = 0, sigma2 = 1), 0.181
over the edges (Np at Q = 2049, M = 3), 0.125 for the surface 1000 units away; the trajectory after 1, 5, 10 and 20 steps is
6.3e-10, 3.0e-8, 4.7e-8 and 3.3e-9 relative from the reference's, against the 1e-3 it is held to (DESIGN 4.27 has the table)."""
import os

import numpy as np
import pytest
import torch

import cpd_ref
import plane_ref
import refit_ref
from test_gpu_range import _dev, _prepared, _soa
from test_gpu_refit import _m44, _same, _score, _t16

pytestmark = pytest.mark.gpu
FACTOR = 8.0
INF = np.float32(np.inf)
KEYS = ("sigma2_out", "Np", "sum_res2")


def _cpd(pm, q, Td, sigma2, w, steps=1, out=None):
    """-> T_out [B, 4, 4], T_step [B, 4, 4], sigma2_out, Np, sum_res2, sum_d2, n_live, empty as numpy"""
    got = pm.refit_cpd(q, Td, sigma2=sigma2, outlier=w, steps=steps, out=out)
    torch.cuda.synchronize()
    T_out, T_step, sig, Np, res, s, n, e = (t.cpu().numpy() for t in got)
    return _m44(T_out), _m44(T_step), sig, Np, res, s, n, e


def _check(got, T, ld, s32, what=""):
    """one call against the two CPU computations on the bits of T that the device was given -> the worst share of the bound"""
    T_out, T_step, sig, Np, res, s, n, e = got
    np.testing.assert_array_equal(n, ld["n_live"])
    assert set(np.unique(e).tolist()) <= {0, 1}
    agree = ld["empty"] == s32["empty"]
    np.testing.assert_array_equal((e != 0)[agree], ld["empty"][agree])
    both, E, _draws = cpd_ref.method_error(ld, s32)
    dev = dict(sigma2_out=sig, Np=Np, sum_res2=res)
    worst = 0.0
    for b in range(len(T)):
        assert all(np.isfinite(x[b]).all() for x in (T_out, T_step, sig, Np, res)), (what, b)
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any() and sig[b] == 0.0, (what, b)     # 32 zeros and sigma2_out = 0
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        assert abs(np.linalg.det(T_step[b][:3, :3]) - 1.0) < 1e-12 and sig[b] > 0
        if not both[b]:
            continue
        shares = {"T_step": float(np.linalg.norm(T_step[b] - ld["T_step"][b])) / (FACTOR * E["T_step"])}
        for k in KEYS:
            shares[k] = abs(dev[k][b] - ld[k][b]) / abs(ld[k][b]) / (FACTOR * E[k])
        print(f"  {what} b = {b}: " + ", ".join(f"{k} {v:.3f} of its bound ({FACTOR * E[k]:.2e})" for k, v in shares.items()))
        for k, v in shares.items():
            assert v <= 1.0, (what, b, k, v)
        worst = max(worst, *shares.values())
    return worst


@pytest.mark.parametrize("w", cpd_ref.OUTLIERS, ids=["w0", "w0.1"])
@pytest.mark.parametrize("si", [0, 1, 2], ids=["initial", "one", "tiny"])
def test_the_main_scene(w, si):
    """check 1"""
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    s2 = cpd_ref.scene_sigma2s()[si]
    ld, s32 = cpd_ref.scene_case(w, s2)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _cpd(pm, q, Td, s2, w)
        _n, s = _score(pm, q, Td, INF)
        np.testing.assert_array_equal(got[5].view(np.uint64), s.view(np.uint64))             # the shift is scoring's nearest distance
        worst = _check(got, T, ld, s32, f"w = {w}, sigma2 = {s2:.4g}")
        print(f"w = {w}, sigma2_in = {s2:.4g}: n_live {got[6].tolist()}, empty {got[7].tolist()}, Np {got[3].tolist()}, sigma2_out {got[2].tolist()}, "
              f"the worst share of the bound {worst:.3f}")
        assert got[7].tolist()[4:] == [1, 1] and got[6].tolist() == [2500] * 4 + [0, 0]
        if w == 0:
            assert np.abs(got[3][:4] - 2500).max() <= 2500 * 2.0 ** -50                      # p_i = 1 for every live query
    finally:
        pm.close()


def test_the_same_bits_whatever_the_call(debug_set):
    """check 2: repeated, at any position, for B = 1 as for B = 6, in other batches, on two streams at once"""
    from pcreg_amd._lib import lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    Q = len(surf)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _cpd(pm, q, Td, 1.0, 0.1, steps=2)
        assert got[7].tolist() == [0, 0, 0, 0, 1, 1]
        _same(_cpd(pm, q, Td, 1.0, 0.1, steps=2), got)
        order = [3, 5, 0, 4, 2, 1]
        moved = _cpd(pm, q, _t16(T[order]), 1.0, 0.1, steps=2)
        _same(moved, tuple(x[order] for x in got))
        for b in range(6):
            _same(_cpd(pm, q, _t16(T[b:b + 1]), 1.0, 0.1, steps=2), tuple(x[b:b + 1] for x in got))
        debug_set("score_batch_slots", 2 * Q)                                                # three batches of two transforms
        _same(_cpd(pm, q, Td, 1.0, 0.1, steps=2), got)
        debug_set("score_batch_slots", 0)
        sig = torch.tensor([1.0, 0.0, 2.5, 1.0, 1.0, 1.0], dtype=torch.float64, device=_dev())   # a variance per candidate
        per = _cpd(pm, q, Td, sig, 0.1)
        for b, v in enumerate(sig.tolist()):
            _same(tuple(x[b:b + 1] for x in per), _cpd(pm, q, _t16(T[b:b + 1]), v, 0.1))
        halves = ((q[:, :2000].contiguous(), Td[:4].contiguous()), (q[:, 400:].contiguous(), Td[2:].contiguous()))
        want, outs = [], []
        for a, b in halves:
            want.append(_cpd(pm, a, b, 0.0, 0.1, steps=2))
            Qh, Bh = a.shape[1], b.shape[0]
            d64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=_dev())
            i32 = lambda: torch.empty(Bh, dtype=torch.int32, device=_dev())
            outs.append((d64(Bh, 16), d64(Bh, 16), d64(Bh), d64(Bh), d64(Bh), d64(Bh), i32(), i32(),
                         torch.empty(int(L.pcreg_dev_model_refit_cpd_workspace(Qh, Bh, pm.M)), dtype=torch.uint8, device=_dev()), d64(Bh, 16)))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, (a, b), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.refit_cpd(a, b, sigma2=0.0, outlier=0.1, steps=2, out=o)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            _same((_m44(o[0].cpu().numpy()), _m44(o[1].cpu().numpy())) + tuple(t.cpu().numpy() for t in o[2:8]), w)
    finally:
        pm.close()


def test_a_surface_a_thousand_units_away():
    """check 3, the 0 / 0 case: every Gaussian underflows unless the shift by dmin is applied"""
    sc = plane_ref.scene()
    model, surf = sc["model"], sc["surf"]
    far = sc["T"][0].copy()
    far[3, 0] += 1000.0
    T = far[None]
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        ld, s32 = cpd_ref.step_ld(surf, model, T, 1e-4, 0.0), cpd_ref.step32(surf, model, T, 1e-4, 0.0)
        got = _cpd(pm, q, Td, 1e-4, 0.0)
        assert got[7].tolist() == [0] and got[6].tolist() == [2500] and abs(got[3][0] - 2500) <= 2500 * 2.0 ** -50
        worst = _check(got, T, ld, s32, "1000 units away, w = 0")
        p2p = refit_ref.step(surf, model, T, np.inf)
        _both, E, _draws = cpd_ref.method_error(ld, s32)
        gap = float(np.linalg.norm(got[1][0] - p2p["T_step"][0]))
        print(f"w = 0: the worst share of the bound {worst:.3f}; |T_step - point-to-point step| = {gap:.3e}, {gap / (FACTOR * E['T_step']):.3f} of the bound")
        assert gap <= FACTOR * E["T_step"]
        got = _cpd(pm, q, Td, 1e-4, 0.1)                                                     # exp(dmin h) overflows: g = 0, the right limit
        assert got[7].tolist() == [1] and got[3].tolist() == [0.0] and got[4].tolist() == [0.0] and got[2].tolist() == [0.0]
        assert not got[0].any() and not got[1].any() and got[6].tolist() == [2500] and np.isfinite(got[5]).all()
    finally:
        pm.close()


def _edge_scene(Q, M):
    model = plane_ref.sheet_samples(M, 100 + M, lo=10.0, hi=30.0).astype(np.float32)
    cloud = plane_ref.sheet_samples(Q, 200 + Q, lo=12.0, hi=28.0)
    c = cloud.mean(axis=0)
    surf = cloud.astype(np.float32)
    T = np.stack([plane_ref.about(plane_ref.rigid(*p), c) for p in plane_ref.PERTURBATIONS[2:]])
    if M > 3:
        model[M // 2, 1] = np.inf                                                            # one dead row
    if Q >= 3:
        surf[Q // 2, 2] = np.nan                                                             # one dead query (Q = 3: Ql = 2, empty)
    return model, surf, T


@pytest.mark.parametrize("M", [3, 63, 64, 65, 4097])
def test_edges(M):
    """check 4: every Q against this M; the bytes after the stated workspace stay as they were"""
    from pcreg_amd._lib import lib
    L = lib()
    for Q in (1, 3, 2048, 2049):
        model, surf, T = _edge_scene(Q, M)
        ld, s32 = cpd_ref.step_ld(surf, model, T, 4.0, 0.1), cpd_ref.step32(surf, model, T, 4.0, 0.1)
        dead = int(Q >= 3)
        assert ld["n_live"].tolist() == [Q - dead] * 2                                       # premise
        if Q - dead < 3:
            assert ld["empty"].all() and s32["empty"].all()
        pm, _t = _prepared(model)
        try:
            q, Td = _soa(surf), _t16(T)
            need = int(L.pcreg_dev_model_refit_cpd_workspace(Q, 2, M))
            buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=_dev())
            d64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=_dev())
            i32 = lambda: torch.empty(2, dtype=torch.int32, device=_dev())
            out = (d64(2, 16), d64(2, 16), d64(2), d64(2), d64(2), d64(2), i32(), i32(), buf[:need], None)
            got = _cpd(pm, q, Td, 4.0, 0.1, out=out)
            assert (buf[need:] == 0xA5).all().item()
            worst = _check(got, T, ld, s32, f"Q = {Q}, M = {M}")
            print(f"Q = {Q}, M = {M}: n_live {got[6].tolist()}, empty {got[7].tolist()}, the worst share of the bound {worst:.3f}")
            _same(_cpd(pm, q, Td, 4.0, 0.1), got)
        finally:
            pm.close()


def test_twenty_steps_follow_the_references_trajectory():
    """check 5: the host tier, `steps` steps in one call, against tests/cpd_ref.py: trajectory()"""
    import pcreg_amd as pc
    sc = plane_ref.scene()
    want = cpd_ref.trajectory()
    with pc.Model(sc["model"]) as h:
        for n, w in zip(cpd_ref.TRAJECTORY_STEPS, want):
            r = h.refit_cpd(sc["surf"], sc["T"][3:4], sigma2=0.0, outlier=0.1, steps=n)
            assert not r["empty"][0]
            rms = plane_ref.rms_to_truth(sc["surf"], r["T"][0], sc["cloud"])
            print(f"{n} steps: RMS to truth {rms:.6f}, the reference's {w:.6f}, off by {abs(rms - w) / w:.2e} relative")
            assert abs(rms - w) <= 1e-3 * w


def test_host_tier_and_device_tier_agree():
    import pcreg_amd as pc
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        got = _cpd(pm, _soa(surf), _t16(T), 0.0, 0.1, steps=3)
        with pc.Model(model) as h:
            r = h.refit_cpd(surf, T, sigma2=0.0, outlier=0.1, steps=3)
        _same((r["T"], r["sigma2"], r["Np"], r["sum_res2"], r["sum_d2"], r["n_live"], r["empty"]), (got[0],) + got[2:7] + (got[7] != 0,))
    finally:
        pm.close()


def test_refine_trials_with_cpd_runs_this_step():
    """check 6: the orientation and the failed trial are kept, as with ndt="""
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    try:
        q = _soa(surf)
        result = dict(trial=np.array([4, 9, 11]), transforms=[pc.invertTF(T[1]), None, pc.invertTF(T[3])])
        inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
        direct = _cpd(pm, q, _t16(inv), 2.0, 0.2, steps=2)
        out, summary = refine_trials(result, pm, q, None, steps=2, cpd=dict(sigma2=2.0, outlier=0.2))
        assert len(out) == 3 and out[1] is None and direct[7].tolist() == [0, 1, 0]
        for t in (0, 2):
            np.testing.assert_array_equal(out[t], pc.invertTF(direct[0][t]))
        for k, i in (("sigma2", 2), ("Np", 3), ("sum_res2", 4), ("sum_d2", 5)):
            np.testing.assert_array_equal(summary[k].view(np.uint64), direct[i].view(np.uint64))
        np.testing.assert_array_equal(summary["n_live"], direct[6])
        dflt, _s = refine_trials(result, pm, q, None, cpd={})                                # the defaults: the initial variance, w = 0.1
        np.testing.assert_array_equal(dflt[0], pc.invertTF(_cpd(pm, q, _t16(inv), 0.0, 0.1)[0][0]))
        assert refine_trials(dict(trial=[], transforms=[]), pm, q, None, cpd={})[0] == []
    finally:
        pm.close()


def test_edges_and_argument_errors():
    """check 7, and the degenerate sizes"""
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, check, lib
    L = lib()
    sc = plane_ref.scene()
    model, surf, T = sc["model"], sc["surf"][:300], sc["T"][:4]
    M = len(model)
    pm, _t = _prepared(model)
    pm0, _t0 = _prepared(model[:0])
    try:
        q, Td = _soa(surf), _t16(T)
        got = _cpd(pm, q, Td, 1.0, 0.1)
        assert got[7].tolist() == [0] * 4
        for g in (_cpd(pm, _soa(surf[:0]), Td, 1.0, 0.1), _cpd(pm0, q, Td, 1.0, 0.1), _cpd(pm0, _soa(surf[:0]), Td, 1.0, 0.1)):
            assert g[7].tolist() == [1] * 4 and g[6].tolist() == [0] * 4 and not any(x.any() for x in g[:6])
        for bad in (-1.0, float("nan")):                                                     # a negative or NaN variance: that candidate is empty
            sig = torch.tensor([1.0, bad, 1.0, 1.0], dtype=torch.float64, device=_dev())
            g = _cpd(pm, q, Td, sig, 0.1)
            assert g[7].tolist() == [0, 1, 0, 0] and not g[0][1].any() and g[2][1] == 0.0
            _same(tuple(x[[0, 2, 3]] for x in g), tuple(x[[0, 2, 3]] for x in got))
        # B = 0 through the C ABI: nothing is written into canary-filled outputs
        canary_d = torch.full((64,), -7.0, dtype=torch.float64, device=_dev())
        canary_i = torch.full((8,), -7, dtype=torch.int32, device=_dev())
        ws0 = torch.empty(int(L.pcreg_dev_model_refit_cpd_workspace(300, 0, M)), dtype=torch.uint8, device=_dev())
        check(L.pcreg_dev_model_refit_cpd_f32(pm.handle, q.data_ptr(), 300, 300, None, 0, None, 0.1, canary_d.data_ptr(), canary_d[16:].data_ptr(),
                                              canary_d[32:].data_ptr(), canary_d[36:].data_ptr(), canary_d[40:].data_ptr(), canary_d[44:].data_ptr(),
                                              canary_i.data_ptr(), canary_i[4:].data_ptr(), ws0.data_ptr(), ws0.numel(), None))
        torch.cuda.synchronize()
        assert canary_d.tolist() == [-7.0] * 64 and canary_i.tolist() == [-7] * 8
        assert pm.refit_cpd(q, Td[:0])[0].shape == (0, 16)
        # T_step = NULL: the other outputs are the same bits; then every argument error
        To = torch.empty((4, 16), dtype=torch.float64, device=_dev())
        so, Np, res, s = (torch.empty(4, dtype=torch.float64, device=_dev()) for _ in range(4))
        n, e = (torch.empty(4, dtype=torch.int32, device=_dev()) for _ in range(2))
        sig = torch.full((4,), 1.0, dtype=torch.float64, device=_dev())
        need = int(L.pcreg_dev_model_refit_cpd_workspace(300, 4, M))
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(Q=300, ldq=300, B=4, w=0.1, wsb=need, qp=q.data_ptr(), tp=Td.data_ptr(), h=pm.handle, op=To.data_ptr(), sp=sig.data_ptr(),
                 sop=so.data_ptr(), npp=Np.data_ptr(), rp=res.data_ptr(), dp=s.data_ptr(), nlp=n.data_ptr(), ep=e.data_ptr(), wp=ws.data_ptr()):
            return L.pcreg_dev_model_refit_cpd_f32(h, qp, Q, ldq, tp, B, sp, w, op, None, sop, npp, rp, dp, nlp, ep, wp, wsb, None)
        assert call() == PCREG_OK
        torch.cuda.synchronize()
        _same((_m44(To.cpu().numpy()),) + tuple(t.cpu().numpy() for t in (so, Np, res, s, n, e)), (got[0],) + got[2:])
        for kw in (dict(w=float("nan")), dict(w=-0.1), dict(w=1.0), dict(w=float("inf")), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1, wsb=1 << 40), dict(B=-1),
                   dict(Q=-1), dict(ldq=299), dict(wsb=need - 1), dict(qp=None), dict(tp=None), dict(h=None), dict(op=None), dict(sp=None), dict(sop=None),
                   dict(npp=None), dict(rp=None), dict(dp=None), dict(nlp=None), dict(ep=None), dict(wp=None), dict(op=Td.data_ptr())):
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        assert call(w=0.0) == PCREG_OK and call(w=0.999999) == PCREG_OK
        torch.cuda.synchronize()
        for kw in (dict(steps=0), dict(outlier=1.0), dict(outlier=-0.5), dict(outlier=float("nan"))):
            with pytest.raises(ValueError):
                pm.refit_cpd(q, Td, **kw)
        with pytest.raises(TypeError):
            pm.refit_cpd(q, Td.float())
        with pytest.raises(TypeError):
            pm.refit_cpd(q, Td, sigma2=sig[:3])
        # the host tier
        with pc.Model(model) as h:
            out, so_h, np_h, rr, ss = np.zeros((4, 16)), np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4)
            nn, ee = (np.zeros(4, np.int32) for _ in range(2))
            T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
            qs, sg = np.asfortranarray(surf), np.ones(4)

            def args(steps=1, w=0.1, ldq=300, sgp=sg.ctypes.data, B=4):
                return (h._h, qs.ctypes.data, 300, ldq, T16.ctypes.data, B, sgp, w, steps, out.ctypes.data, so_h.ctypes.data, np_h.ctypes.data,
                        rr.ctypes.data, ss.ctypes.data, nn.ctypes.data, ee.ctypes.data)
            f = L.pcreg_model_refit_cpd_f32
            assert f(*args(0)) == PCREG_E_ARG and f(*args(-1)) == PCREG_E_ARG
            for w in (float("nan"), -0.1, 1.0, 2.0):
                assert f(*args(w=w)) == PCREG_E_ARG, w
            assert f(*args(ldq=299)) == PCREG_E_ARG and f(*args(sgp=None)) == PCREG_E_ARG and f(*args(B=-1)) == PCREG_E_ARG
            assert f(*args()) == PCREG_OK
            _same((_m44(out), so_h, np_h, rr, ss, nn, ee), (got[0],) + got[2:])
            for kw in (dict(steps=0), dict(outlier=1.0), dict(outlier=float("nan")), dict(sigma2=[1.0, 2.0])):
                with pytest.raises(ValueError):
                    h.refit_cpd(surf, T, **kw)
            r = h.refit_cpd(surf[:0], T)
            assert r["empty"].all() and not r["T"].any() and not r["n_live"].any()
        with pc.Model(model[:0]) as h0:
            r = h0.refit_cpd(surf, T)
            assert r["empty"].all() and not r["T"].any() and not r["Np"].any()
    finally:
        pm.close()
        pm0.close()
