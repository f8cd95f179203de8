"""Trimmed scoring and refits (knn_trim.hip) on the GPU.

1  keep_ratio = 1.0: every output of the four trimmed calls has the untrimmed call's bits, at every radius, n_within == n_close.
2  Against tests/trim_ref.py at ratios 0.9, 0.6, 0.25 and 1e-6 with r = 1.5 and r2 = +inf: n_within, n_close, the kept set and the bits
   of d2_cut exactly; sum_d2 as tests/test_gpu_score.py compares it; the fits under their own GPU tests' bounds and premises.
3  The last radix pass: 289 distances that differ in their last byte only, with exact ties, for every keep.
4  A run of ties across the chunk boundary, for every budget inside it.
5  Degenerate values: all distances equal for every keep, all zero, 0 .. 4 pairs, distances of +inf.
6  The same bits twice, with culling off, in three batches, in a dirtied workspace.
7  The edges and the argument errors.
8  The partial-overlap scene: the trimmed refit converges where the radius refit stalls (tests/test_trim_ref.py states the bounds as
   properties of the reference), on the device, at the host tier and through refine_trials.

The rigid step's scene is tests/test_gpu_refit.py's; the point-to-plane and plane-to-plane steps are held to the reference on
tests/plane_ref.py's sheet, the scene their own GPU tests' bounds and pivot premise were stated for."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gicp_ref
import plane_ref
import refit_ref
import score_ref
import trim_ref
from test_gpu_range import _dev, _prepared, _soa, _stats
from test_gpu_refit import BOUND, R15, RADII, _few, _m44, _same, _scene, _t16
from test_gpu_refit_gicp import _check as _check_gicp
from test_gpu_refit_plane import _check as _check_plane

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
RATIOS = [0.9, 0.6, 0.25, 1e-6]
INF = np.float32(np.inf)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _np(out):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _score(pm, q, Td, r2, ratio=None):
    """-> n_close, sum_d2, idx, dist (, n_within, d2_cut)"""
    return _np(pm.score_transforms(q, Td, r2, rows=True, keep_ratio=ratio))


def _mats(got):
    return (_m44(got[0]), _m44(got[1])) + tuple(got[2:])


def _refit(pm, q, Td, r2, ratio=None, steps=1):
    """-> T_out, T_step, n_close, sum_d2, empty (, n_within, d2_cut)"""
    return _mats(_np(pm.refit_transforms(q, Td, r2, steps=steps, keep_ratio=ratio)))


def _plane(pm, q, Td, r2, nrm, ratio=None, steps=1):
    """-> T_out, T_step, n_close, sum_d2, n_plane, sum_res2, empty (, n_within, d2_cut)"""
    return _mats(_np(pm.refit_plane(q, Td, r2, nrm, steps=steps, keep_ratio=ratio)))


def _gicp(pm, q, Td, r2, nrm, nq, ratio=None, steps=1):
    if ratio is None:
        return _mats(_np(pm.refit_gicp(q, Td, r2, nrm, nq, steps=steps)))
    return _mats(_np(pm.refit_gicp_trimmed(q, Td, r2, ratio, nrm, nq, steps=steps)))


# ---- the comparators ----------------------------------------------------------------------------------------------------------
def check_trim_outputs(n_within, d2_cut, want):
    assert n_within.dtype == np.int32 and d2_cut.dtype == np.float32
    np.testing.assert_array_equal(n_within, want["n_within"])
    np.testing.assert_array_equal(_bits(d2_cut), _bits(want["d2_cut"]))


def check_score(got, want, Q):
    """the kept set, the counts and the bits of d2_cut exactly; sum_d2 within (Q - 1) 2^-53 fsum, as tests/test_gpu_score.py"""
    n_close, sum_d2, idx, dist, n_within, d2_cut = got
    np.testing.assert_array_equal(idx, want["idx"])
    np.testing.assert_array_equal(_bits(dist), _bits(want["dist"]))
    np.testing.assert_array_equal(n_close, want["n_close"])
    check_trim_outputs(n_within, d2_cut, want)
    for b in range(len(n_close)):
        rs = want["sum_d2"][b]
        if np.isfinite(rs):
            assert abs(sum_d2[b] - rs) <= max(Q - 1, 0) * 2.0 ** -53 * rs, (b, sum_d2[b], rs)
        else:
            assert sum_d2[b] == rs, (b, sum_d2[b], rs)


def check_refit(got, T, want, model, what=""):
    """tests/test_gpu_refit.py's _check on the kept pairs: the bound on T_step is asserted under its conditioning premise, which is
    itself asserted wherever at least a hundred pairs are kept"""
    T_out, T_step, n, s, e, n_within, d2_cut = got
    np.testing.assert_array_equal(n, want["n_close"])
    np.testing.assert_array_equal(e != 0, want["empty"])
    check_trim_outputs(n_within, d2_cut, want)
    for b in range(len(T)):
        rs = want["sum_d2"][b]
        assert (abs(s[b] - rs) <= max(len(want["idx"][b]) - 1, 0) * 2.0 ** -53 * rs) if np.isfinite(rs) else s[b] == rs, (what, b, s[b], rs)
        if e[b]:
            assert not T_step[b].any() and not T_out[b].any(), b
            continue
        np.testing.assert_array_equal(T_out[b].view(np.uint64), refit_ref.compose(T[b], T_step[b]).view(np.uint64))
        if not np.isfinite(want["tq"][b][want["hit"][b]]).all() or not np.isfinite(want["dist"][b][want["hit"][b]]).all():
            continue
        sv = refit_ref.cross_covariance_singular_values(model, want["idx"][b], want["tq"][b])
        if n[b] >= 100:
            assert sv[-1] > 1e-3 * sv[0], (what, b, sv)
        if sv[-1] > 1e-3 * sv[0]:
            err = float(np.linalg.norm(T_step[b] - want["T_step"][b]))
            print(f"  {what} b = {b}: kept {n[b]} of {n_within[b]}, |T_step - oracle| = {err:.3e}")
            assert err < BOUND, (what, b, err)


# ---- the scenes and their references, computed once ---------------------------------------------------------------------------
_REF = {}


def _cand(name, surf, model, T, r2):
    """scoring's candidate pairs of a scene at r2; the nearest rows are computed once per scene, whatever the radius"""
    if name not in _REF:
        tq = score_ref.transformed(surf, T)
        _REF[name] = (tq, score_ref.nearest(tq.reshape(-1, 3), model, threads=CORES))
    tq, nn = _REF[name]
    idx, dist = score_ref.within(nn[0], nn[1], r2)
    return tq, idx.reshape(tq.shape[:2]), dist.reshape(tq.shape[:2])


def _want(name, surf, model, T, r2, ratio, method="rigid", **kw):
    key = (name, float(r2), ratio, method)
    if key not in _REF:
        _REF[key] = trim_ref.step_of_pairs(_cand(name, surf, model, T, r2), model, T, ratio, method, **kw)
    return _REF[key]


def _sheet():
    sc = plane_ref.scene()
    return sc["model"], sc["surf"], sc["T"], sc["normals"], gicp_ref.surface_normals()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", RADII, ids=["r0", "r0.5", "r1.5", "rinf"])
def test_ratio_one_is_the_untrimmed_call(r2):
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    pm, _t = _prepared(model)
    pq, _tq = _prepared(surf)
    try:
        q, Td = _soa(surf), _t16(T)
        nrm, nq = pm.normals(8), pq.normals(8)                 # (any normals: the two calls get the same)
        for plain, trimmed, n_at in ((_score(pm, q, Td, r2), _score(pm, q, Td, r2, 1.0), 0),
                                     (_refit(pm, q, Td, r2), _refit(pm, q, Td, r2, 1.0), 2),
                                     (_plane(pm, q, Td, r2, nrm), _plane(pm, q, Td, r2, nrm, 1.0), 2),
                                     (_gicp(pm, q, Td, r2, nrm, nq), _gicp(pm, q, Td, r2, nrm, nq, 1.0), 2)):
            assert len(trimmed) == len(plain) + 2
            _same(trimmed[:-2], plain)
            n_within, d2_cut = trimmed[-2:]
            np.testing.assert_array_equal(n_within, plain[n_at])
            assert n_within.dtype == np.int32 and d2_cut.dtype == np.float32
        n_close, _s, _idx, dist = _score(pm, q, Td, r2)
        n_within, d2_cut = _score(pm, q, Td, r2, 1.0)[-2:]
        for b in range(len(T)):                                 # d2_cut: the largest distance of a pair, +inf where there is none
            want = dist[b][_idx[b] >= 0].max() if n_close[b] else INF
            assert _bits(d2_cut[b:b + 1])[0] == _bits(np.array([want], np.float32))[0], (b, d2_cut[b], want)
        assert n_within[4] == 0 and n_within[5] == 0            # the empty and the NaN candidate
        print(f"r2 = {float(r2):.4g}: n_within {n_within.tolist()}, d2_cut {d2_cut.tolist()}")
    finally:
        pm.close()
        pq.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", [R15, INF], ids=["r1.5", "rinf"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_score_and_rigid_refit_against_the_reference(ratio, r2):
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"], sc["T"]
    Q = len(surf)
    want = _want("scene", surf, model, T, r2, ratio)
    assert (want["n_within"][:4] > 2000).all() and (want["n_within"][4:] == 0).all()                     # premises
    assert all(want["n_close"][b] == trim_ref.keep_count(ratio, want["n_within"][b]) for b in range(6))
    if ratio == 1e-6:
        assert want["n_close"].tolist() == [1, 1, 1, 1, 0, 0] and want["empty"].all()
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _score(pm, q, Td, r2, ratio)
        check_score(got, want, Q)
        assert np.isinf(got[5][4:]).all() and (got[2][4:] == -1).all()
        fit = _refit(pm, q, Td, r2, ratio)
        np.testing.assert_array_equal(_bits(fit[3]), _bits(got[1]))                                      # sum_d2: scoring's bits
        check_refit(fit, T, want, model, f"ratio {ratio} r2 {float(r2):.4g}")
        print(f"ratio {ratio}, r2 = {float(r2):.4g}: n_within {got[4].tolist()}, n_close {got[0].tolist()}, d2_cut {got[5].tolist()}, "
              f"empty {fit[4].tolist()}")
    finally:
        pm.close()


@pytest.mark.parametrize("r2", [R15, INF], ids=["r1.5", "rinf"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_plane_and_gicp_refits_against_the_reference(ratio, r2):
    model, surf, T, normals, sn = _sheet()
    wp = _want("sheet", surf, model, T, r2, ratio, "plane", normals=normals)
    wg = _want("sheet", surf, model, T, r2, ratio, "gicp", normals=normals, qnormals=sn)
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _soa(normals), _soa(sn)
        gp = _plane(pm, q, Td, r2, nrm, ratio)
        check_trim_outputs(gp[7], gp[8], wp)
        _check_plane(gp[:7], T, wp, f"plane, ratio {ratio}")
        gg = _gicp(pm, q, Td, r2, nrm, nq, ratio)
        check_trim_outputs(gg[7], gg[8], wg)
        _check_gicp(gg[:7], T, wg, f"plane-to-plane, ratio {ratio}")
        sums = _score(pm, q, Td, r2, ratio)
        for g in (gp, gg):                                      # n_close and sum_d2: the trimmed scoring's bits
            np.testing.assert_array_equal(g[2], sums[0])
            np.testing.assert_array_equal(_bits(g[3]), _bits(sums[1]))
        print(f"ratio {ratio}, r2 = {float(r2):.4g}: n_within {gp[7].tolist()}, n_close {gp[2].tolist()}, n_plane {gp[4].tolist()}, "
              f"n_pairs {gg[4].tolist()}, empty {gp[6].tolist()} / {gg[6].tolist()}")
    finally:
        pm.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _kept_sets(pm, q, Td, r2, ref_idx, ref_dist, keeps):
    """for every keep of `keeps` (of ref's n_within pairs): the device's kept set, n_within, n_close and d2_cut are the reference's"""
    n = int((ref_idx >= 0).sum())
    for keep in keeps:
        ratio = (keep - 0.25) / n
        assert trim_ref.keep_count(ratio, n) == keep, (keep, n)
        wi, wd, wn, wc = trim_ref.trim(ref_idx, ref_dist, ratio)
        n_close, _s, idx, dist, n_within, d2_cut = _score(pm, q, Td, r2, ratio)
        assert n_within.tolist() == [wn] and n_close.tolist() == [keep], (keep, n_within, n_close)
        np.testing.assert_array_equal(idx[0], wi, err_msg=f"keep {keep}")
        np.testing.assert_array_equal(_bits(dist[0]), _bits(wd))
        assert _bits(d2_cut)[0] == _bits(np.array([wc]))[0], (keep, d2_cut, wc)


def test_the_last_radix_pass_and_exact_ties():
    """every d is exactly 1 + 2 (a^2 + b^2) 2^-23, and (+-a, +-b) / (b, a) tie: 285 patterns share their upper 24 bits and differ in
    the last byte only; the four corners (a^2 + b^2 = 128) carry into bit 8, so the largest keeps also cross the third pass"""
    model = np.array([[0.0, 0.0, 0.0]] + [[200.0 + i, 200.0, 200.0] for i in range(63)], np.float32)     # the pads: d > 100
    ab = np.array([(a, b) for a in range(-8, 9) for b in range(-8, 9)], np.float64)
    surf = np.column_stack([np.ones(289), ab * 2.0 ** -11]).astype(np.float32)
    idx, dist, _n, _s = score_ref.score(surf, model, np.eye(4)[None], 4.0, threads=CORES)
    want_d = (1.0 + 2.0 * (ab ** 2).sum(axis=1) * 2.0 ** -23).astype(np.float32)
    np.testing.assert_array_equal(_bits(dist[0]), _bits(want_d))                                          # premises
    upper = _bits(dist[0]) >> 8
    assert (idx[0] == 0).all() and len(np.unique(dist[0])) < 100
    assert sorted(np.unique(upper, return_counts=True)[1].tolist()) == [4, 285] and (upper[[0, 16, 272, 288]] == upper.max()).all()
    pm, _t = _prepared(model)
    try:
        _kept_sets(pm, _soa(surf), _t16(np.eye(4)[None]), 4.0, idx[0], dist[0], range(1, 290))
    finally:
        pm.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_ties_across_a_chunk_boundary():
    """one query row at positions 2040 .. 2055 of 2500, the cut inside the run: every budget of ties from none to all, so the budget
    ends at index 2047 (eight ties kept) and at 2048 (nine) among the others"""
    rng = np.random.default_rng(41)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.column_stack([rng.uniform(0.01, 1.0, 2500), np.zeros(2500), np.zeros(2500)])).astype(np.float32)
    surf[2040:2056] = model[17] + np.array([0.5, 0.0, 0.0], np.float32)
    T = np.eye(4)[None]
    idx, dist, _n, _s = score_ref.score(surf, model, T, R15, threads=CORES)
    run = np.arange(2040, 2056)
    assert len(set(_bits(dist[0][run]).tolist())) == 1 and (idx[0][run] >= 0).all()                      # premises: one d, all pairs
    others = np.setdiff1d(np.flatnonzero(idx[0] >= 0), run)
    assert not (dist[0][others] == dist[0][2040]).any()
    below = int((dist[0][others] < dist[0][2040]).sum())
    assert 100 < below < len(others) - 100
    pm, _t = _prepared(model)
    try:
        _kept_sets(pm, _soa(surf), _t16(T), R15, idx[0], dist[0], range(below, below + 18))               # 0 .. 16 ties kept, and one past
        keep8 = trim_ref.trim(idx[0], dist[0], (below + 8 - 0.25) / (len(others) + 16))[0]
        assert keep8[2047] >= 0 and keep8[2048] == -1                                                     # the budget ends at 2047 ...
        keep9 = trim_ref.trim(idx[0], dist[0], (below + 9 - 0.25) / (len(others) + 16))[0]
        assert keep9[2048] >= 0 and keep9[2049] == -1                                                     # ... and at 2048
    finally:
        pm.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_all_distances_equal_for_every_keep():
    rng = np.random.default_rng(43)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    T = np.eye(4)[None]
    pm, _t = _prepared(model)
    try:
        for Q, keeps in ((300, range(1, 301)), (2100, [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2046, 2047, 2048, 2049, 2050, 2099, 2100])):
            surf = np.tile(model[5] + np.array([0.25, 0.0, 0.0], np.float32), (Q, 1)).astype(np.float32)
            idx, dist, _n, _s = score_ref.score(surf, model, T, R15, threads=CORES)
            assert len(set(_bits(dist[0]).tolist())) == 1 and (idx[0] >= 0).all()
            _kept_sets(pm, _soa(surf), _t16(T), R15, idx[0], dist[0], keeps)
    finally:
        pm.close()


def test_all_distances_zero():
    rng = np.random.default_rng(44)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    surf = model[rng.choice(3000, 2500, replace=False)]
    T = np.eye(4)[None]
    idx, dist, _n, _s = score_ref.score(surf, model, T, R15, threads=CORES)
    assert not dist[0].any()
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        _kept_sets(pm, q, Td, R15, idx[0], dist[0], [1, 3, 1250, 2047, 2048, 2049, 2499, 2500])
        for ratio in (0.9, 0.5):
            want = trim_ref.step_of_pairs((score_ref.transformed(surf, T), idx, dist), model, T, ratio)
            got = _refit(pm, q, Td, R15, ratio)
            check_refit(got, T, want, model, f"d = 0, ratio {ratio}")
            assert got[6].tolist() == [0.0] and got[3].tolist() == [0.0] and got[4].tolist() == [0]
            assert np.flatnonzero(want["hit"][0]).tolist() == list(range(trim_ref.keep_count(ratio, 2500)))  # the first `keep` queries
    finally:
        pm.close()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_exactly_k_pairs_within_the_radius(k):
    """tests/test_gpu_refit.py's k-pair clouds at r2 = 0: n_within = k, keep by the rule, fewer than three kept pairs are empty"""
    model, surf, at, rows = _few(k)
    T = np.stack([np.eye(4), plane_ref.rigid([0.001, 0.0, 0.0], [0.01, 0.0, 0.0])])
    cand = trim_ref.pairs(surf, model, T, 0.0, threads=CORES)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        for ratio in (1.0, 0.75, 0.5, 1e-6):
            want = trim_ref.step_of_pairs(cand, model, T, ratio)
            keep = trim_ref.keep_count(ratio, k)
            assert want["n_within"].tolist() == [k, 0] and want["n_close"].tolist() == [keep, 0]          # premises
            assert np.flatnonzero(want["hit"][0]).tolist() == at[:keep]                                   # all d = 0: the lowest queries
            assert want["empty"].tolist() == [keep < 3, True]
            check_score(_score(pm, q, Td, 0.0, ratio), want, len(surf))
            got = _refit(pm, q, Td, 0.0, ratio)
            check_refit(got, T, want, model, f"k = {k}, ratio {ratio}")
            assert np.isinf(got[6][1]) and (got[6][0] == 0.0 if k else np.isinf(got[6][0]))
    finally:
        pm.close()


def test_overflowed_distances_pass_only_without_a_radius():
    """queries 1e20 away: d overflows to +inf, which r2 = +inf admits and nothing else; +inf orders last, its ties by query"""
    rng = np.random.default_rng(45)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    surf = (model[rng.choice(3000, 2500, replace=False)] + np.float32(0.1)).astype(np.float32)
    far = [3, 700, 2040, 2047, 2048, 2049, 2300, 2301, 2302, 2499]
    surf[far] = np.float32(1e20)
    T = np.eye(4)[None]
    idx, dist, _n, _s = score_ref.score(surf, model, T, INF, threads=CORES)
    assert np.isinf(dist[0][far]).all() and (idx[0] >= 0).all() and np.isfinite(np.delete(dist[0], far)).all()   # premises
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        _kept_sets(pm, q, Td, INF, idx[0], dist[0], [2489, 2490, 2491, 2493, 2494, 2495, 2499, 2500])
        fi, fd, _n, _s = score_ref.score(surf, model, T, 1e30, threads=CORES)                              # a finite radius: they are no pairs
        assert (fi[0][far] == -1).all()
        _kept_sets(pm, q, Td, np.float32(1e30), fi[0], fd[0], [2489, 2490])
    finally:
        pm.close()


def test_more_transforms_than_one_round_of_the_select_holds():
    """Q = 5 and B = 300: the select's state lives in a dead block of the untrimmed workspace that holds 126 transforms', so the
    batch is trimmed in three rounds; every transform against the reference, the same bits in smaller batches"""
    rng = np.random.default_rng(46)
    model = rng.uniform(-2, 2, (64, 3)).astype(np.float32)
    surf = rng.uniform(-2, 2, (5, 3)).astype(np.float32)
    T = np.tile(np.eye(4), (300, 1, 1))
    T[:, 3, :3] = rng.normal(0, 0.3, (300, 3))
    T[7] = 0.0
    cand = trim_ref.pairs(surf, model, T, INF, threads=CORES)
    want = trim_ref.step_of_pairs(cand, model, T, 0.5)
    assert want["n_within"].tolist() == [5] * 7 + [0] + [5] * 292 and want["n_close"][0] == 3                # premises
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(surf), _t16(T)
        got = _score(pm, q, Td, INF, 0.5)
        check_score(got, want, 5)
        fit = _refit(pm, q, Td, INF, 0.5)
        check_refit(fit, T, want, model, "300 transforms of 5 queries")
    finally:
        pm.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_twice_without_culling_in_batches_and_in_a_dirty_workspace(debug_set):
    model, surf, T6, normals, sn = _sheet()
    T = np.concatenate([T6, T6[:2]])                            # eight transforms
    Q, B = len(surf), 8
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _soa(normals), _soa(sn)
        calls = dict(score=lambda: _score(pm, q, Td, R15, 0.6), refit=lambda: _refit(pm, q, Td, R15, 0.6, steps=2),
                     plane=lambda: _plane(pm, q, Td, R15, nrm, 0.6), gicp=lambda: _gicp(pm, q, Td, R15, nrm, nq, 0.6))
        first = {k: f() for k, f in calls.items()}
        assert first["score"][0][0] == trim_ref.keep_count(0.6, first["score"][4][0]) > 1000
        for k, f in calls.items():
            _same(f(), first[k])                                # twice
        debug_set("knn_nocull", 1)
        for k, f in calls.items():
            _same(f(), first[k])
        debug_set("knn_nocull", 0)
        debug_set("knn_stats", 1)
        _stats(reset=True)
        debug_set("score_batch_slots", 3 * Q)
        got = _score(pm, q, Td, R15, 0.6)
        st = _stats(reset=True)
        assert st[0] == 3, st                                   # premise: 3 + 3 + 2 transforms
        _same(got, first["score"])
        for k in ("refit", "plane", "gicp"):
            _same(calls[k](), first[k])
        debug_set("score_batch_slots", 0)
        debug_set("knn_stats", 0)
        # caller-owned buffers, the workspace filled with 0xFF and with what an untrimmed call and another ratio leave in it
        L = __import__("pcreg_amd._lib", fromlist=["lib"]).lib()
        need = int(L.pcreg_dev_model_score_workspace(Q, B, pm.M))      # (the untrimmed size: the trim needs no more)
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=_dev())
        for fill in (0xFF, 0x00, None):
            if fill is None:
                pm.score_transforms(q, Td, INF, rows=False, out=(new(B, torch.int32), new(B, torch.float64), None, None, ws))
                pm.score_transforms(q, Td, INF, keep_ratio=0.123, out=(new(B, torch.int32), new(B, torch.float64), None, None, new(B, torch.int32),
                                                                          new(B, torch.float32), ws))
            else:
                ws.fill_(fill)
            out = (new(B, torch.int32), new(B, torch.float64), new((B, Q), torch.int32), new((B, Q), torch.float32), new(B, torch.int32),
                   new(B, torch.float32), ws)
            _same(_np(pm.score_transforms(q, Td, R15, rows=True, out=out, keep_ratio=0.6)), first["score"])
    finally:
        pm.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_edges_and_argument_errors():
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, lib
    from pcreg_amd.device import PreparedModel
    sc = _scene()
    model, surf, T = sc["model"], sc["surf"][:300], sc["T"][:4]
    want = trim_ref.step(surf, model, T, R15, 0.6, threads=CORES)
    pm, _t = _prepared(model)
    pm0 = PreparedModel(torch.empty((3, 0), dtype=torch.float32, device=_dev()))
    L = lib()
    try:
        q, Td = _soa(surf), _t16(T)
        got = _refit(pm, q, Td, R15, 0.6)
        check_refit(got, T, want, model, "300 queries")
        sgot = _score(pm, q, Td, R15, 0.6)
        check_score(sgot, want, 300)
        wide = torch.full((3, 1000), 1e30, dtype=torch.float32, device=_dev())                          # ldq > Q
        wide[:, 100:400] = q
        qw = wide[:, 100:400]
        assert qw.stride(0) == 1000
        _same(_refit(pm, qw, Td, R15, 0.6), got)
        _same(_score(pm, qw, Td, R15, 0.6), sgot)
        # Q = 0 and a model without rows: no pairs
        for g in (_refit(pm, _soa(surf[:0]), Td, R15, 0.6), _refit(pm0, q, Td, R15, 0.6), _refit(pm0, _soa(surf[:0]), Td, R15, 0.6)):
            assert not g[0].any() and not g[2].any() and not g[3].any() and g[4].tolist() == [1] * 4
            assert g[5].tolist() == [0] * 4 and np.isposinf(g[6]).all()
        for g in (_score(pm, _soa(surf[:0]), Td, R15, 0.6), _score(pm0, q, Td, R15, 0.6)):
            assert not g[0].any() and not g[1].any() and g[4].tolist() == [0] * 4 and np.isposinf(g[5]).all()
            assert (g[2] == -1).all() and np.isposinf(g[3]).all()
        # B = 0
        g = _refit(pm, q, _t16(np.zeros((0, 4, 4))), R15, 0.6)
        assert [len(a) for a in g] == [0] * 7
        g = _score(pm, q, _t16(np.zeros((0, 4, 4))), R15, 0.6)
        assert len(g) == 6 and len(g[4]) == 0 and g[2].shape == (0, 300)
        # NULL n_within / d2_cut / T_step, and a workspace one byte short, through the C entry
        i32, f64 = torch.int32, torch.float64
        To, n, s, e = (torch.zeros((4, 16), dtype=f64, device=_dev()), torch.zeros(4, dtype=i32, device=_dev()),
                       torch.zeros(4, dtype=f64, device=_dev()), torch.zeros(4, dtype=i32, device=_dev()))
        need = int(L.pcreg_dev_model_refit_workspace(300, 4, pm.M))     # (the untrimmed size: the trim needs no more)
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(kr=0.6, wsb=need, r2=float(R15), ts=None, w=None, cut=None):
            return L.pcreg_dev_model_refit_trimmed_f32(pm.handle, q.data_ptr(), 300, 300, Td.data_ptr(), 4, r2, kr, To.data_ptr(), ts, n.data_ptr(),
                                                       s.data_ptr(), e.data_ptr(), ws.data_ptr(), wsb, None, w, cut)
        assert call() == PCREG_OK
        torch.cuda.synchronize()
        _same((_m44(To.cpu().numpy()), n.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()), (got[0], got[2], got[3], got[4]))
        w = torch.zeros(4, dtype=i32, device=_dev())
        assert call(w=w.data_ptr()) == PCREG_OK                                                          # one of the two alone
        torch.cuda.synchronize()
        np.testing.assert_array_equal(w.cpu().numpy(), got[5])
        for kw in (dict(wsb=need - 1), dict(kr=float("nan")), dict(kr=0.0), dict(kr=-0.5),
                   dict(kr=1.0 + 2.0 ** -52), dict(kr=float("inf")), dict(r2=-1.0)):
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        for bad in (float("nan"), 0.0, -1.0, 1.5):
            with pytest.raises(ValueError):
                pm.refit_transforms(q, Td, R15, keep_ratio=bad)
            with pytest.raises(ValueError):
                pm.score_transforms(q, Td, R15, keep_ratio=bad)
        # the host tier: the same bits, one step
        with pc.Model(model) as h:
            r = h.refit_transforms(surf, T, R15, keep_ratio=0.6)
            _same((r["T"], r["n_close"], r["sum_d2"], r["empty"], r["n_within"], r["d2_cut"]), (got[0], got[2], got[3], got[4] != 0, got[5], got[6]))
            r = h.score_transforms(surf, T, R15, rows=True, keep_ratio=0.6)
            _same((r["n_close"], r["sum_d2"], r["idx"], r["dist"], r["n_within"], r["d2_cut"]), sgot)
            with pytest.raises(ValueError):
                h.refit_transforms(surf, T, R15, keep_ratio=1.5)
            assert "n_within" not in h.refit_transforms(surf, T, R15)
    finally:
        pm.close()
        pm0.close()


def test_host_tier_plane_and_gicp_have_the_device_tiers_bits():
    import pcreg_amd as pc
    model, surf, T, normals, sn = _sheet()
    pm, _t = _prepared(model)
    try:
        q, Td, nrm, nq = _soa(surf), _t16(T), _soa(normals), _soa(sn)
        gp, gg = _plane(pm, q, Td, R15, nrm, 0.6, steps=2), _gicp(pm, q, Td, R15, nrm, nq, 0.6, steps=2)
        with pc.Model(model) as h:
            r = h.refit_plane(surf, T, R15, steps=2, normals=normals, keep_ratio=0.6)
            _same((r["T"], r["n_close"], r["sum_d2"], r["n_plane"], r["sum_res2"], r["empty"], r["n_within"], r["d2_cut"]),
                  (gp[0], gp[2], gp[3], gp[4], gp[5], gp[6] != 0, gp[7], gp[8]))
            r = h.refit_gicp(surf, T, R15, steps=2, normals=normals, query_normals=sn, keep_ratio=0.6)
            _same((r["T"], r["n_close"], r["sum_d2"], r["n_pairs"], r["sum_res2"], r["empty"], r["n_within"], r["d2_cut"]),
                  (gg[0], gg[2], gg[3], gg[4], gg[5], gg[6] != 0, gg[7], gg[8]))
    finally:
        pm.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_trimming_gets_out_of_where_the_radius_stalls():
    """four steps on the partial-overlap scene: trimmed at 0.6 below 0.01 RMS from the truth, the radius alone above 0.2 -- the
    reference's own figures (tests/test_trim_ref.py) -- with the reference's kept counts at every step; the host tier and
    refine_trials give the device tier's bits"""
    import pcreg_amd as pc
    from pcreg_amd.sweep import refine_trials, score_trials
    sc = trim_ref.overlap_scene(7)
    model, surf, T0, r2 = sc["model"], sc["surf"], sc["T0"][None], sc["r2"]
    pm, _t = _prepared(model)
    try:
        q = _soa(surf)
        end = {}
        for ratio in (0.6, None):
            ref = trim_ref.overlap_ref(ratio, 4, threads=CORES)
            cur, rms = T0, []
            for step in range(4):                               # step by step: the counts of every step
                got = _refit(pm, q, _t16(cur), r2, ratio)
                assert got[4].tolist() == [0]
                assert got[2].tolist() == ref[step]["n_close"].tolist(), (ratio, step)
                if ratio is not None:
                    assert got[5].tolist() == ref[step]["n_within"].tolist(), (ratio, step)
                cur = got[0]
                rms.append(trim_ref.overlap_rms(sc, cur[0]))
            print(f"ratio {ratio}: rms per step {[round(v, 4) for v in rms]}")
            four = _refit(pm, q, _t16(T0), r2, ratio, steps=4)
            _same(four, got)                                    # one call of four steps: the fourth single step's bits
            end[ratio] = (rms[-1], four)
        assert end[0.6][0] < 0.01
        assert end[None][0] > 0.2
        four = end[0.6][1]
        with pc.Model(model) as h:
            r = h.refit_transforms(surf, T0, r2, steps=4, keep_ratio=0.6)
        _same((r["T"], r["n_close"], r["sum_d2"], r["empty"], r["n_within"], r["d2_cut"]), (four[0], four[2], four[3], four[4] != 0, four[5], four[6]))
        result = dict(trial=np.array([3]), transforms=[pc.invertTF(T0[0])])
        out, summary = refine_trials(result, pm, q, 1.5, steps=4, keep_ratio=0.6)
        np.testing.assert_array_equal(out[0], pc.invertTF(four[0][0]))
        _same((summary["n_close"], summary["sum_d2"], summary["n_within"], summary["d2_cut"]), (four[2], four[3], four[5], four[6]))
        assert trim_ref.overlap_rms(sc, pc.invertTF(out[0])) < 0.01
        st = score_trials(result, pm, q, 1.5, keep_ratio=0.6)
        one = _score(pm, q, _t16(T0), r2, 0.6)
        _same((st["n_close"], st["sum_d2"], st["n_within"], st["d2_cut"]), (one[0], one[1], one[4], one[5]))
        assert "n_within" not in score_trials(result, pm, q, 1.5)
        with pytest.raises(ValueError):
            refine_trials(result, pm, q, 1.5, keep_ratio=0.6, cpd={})
    finally:
        pm.close()
