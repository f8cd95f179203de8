"""MSAC sphere fitting and extraction on a prepared model (knn_fitsphere.hip) on the GPU against tests/spheres_ref.py.

Per round, from the alive set the returned labels imply: best_trial, best_cost and best_count EQUAL to the reference (exact fmaf
chain, IEEE root, integer sums); spheres and refit_used bit for bit equal to finish64 on the reference's integer sums; labels,
counts and rmse EQUAL to the classification restated from the RETURNED sphere.  No row is excluded anywhere.  Then the sample
table, the radius bounds, the edge clouds, the knife edge, the refit that is not used, determinism, the tiers and the workspace.
tests/test_spheres_ref.py asserts the premises of these scenes on the CPU."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import spheres_ref as ref

pytestmark = pytest.mark.gpu

T = ref.SCENE_T


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _soa(x):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.array(x.T, order="C")))
    return t


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    t = _soa(model)
    return PreparedModel(t), t


def _host(res):
    """a PreparedModel.fit_spheres dict as numpy"""
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out["n_spheres"] = int(out["n_spheres"][0])
    return out


def _run(pm, t, samples=None, **kw):
    if samples is not None:
        samples = torch.from_numpy(np.ascontiguousarray(samples, np.int32)).to(_dev())
    return _host(pm.fit_spheres(t, samples=samples, **kw))


def _fit(model, t, **kw):
    pm, _t = _prepared(model)
    try:
        return _run(pm, t, **kw)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


KEYS_F, KEYS_I = ("spheres", "rmse"), ("labels", "counts", "refit_used", "best_trial", "best_cost", "best_count")
NAMES = ("labels", "spheres", "counts", "rmse", "refit_used", "n_spheres", "best_trial", "best_cost", "best_count")


def _same(a, b):
    return (a["n_spheres"] == b["n_spheres"] and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS_F)
            and all(np.array_equal(a[k], b[k]) for k in KEYS_I))


@functools.lru_cache(maxsize=None)
def _scene(M):
    a = ref.scene(M)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _scene_labels():
    """who is on which sphere of the 1030-row scene, by the reference (shared; nothing writes to it)"""
    M, B, mi = ref.SCENES[0]
    lab = ref.fit_spheres(_scene(M), T, max_spheres=ref.SCENE_P, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)["labels"]
    lab.setflags(write=False)
    return lab


def _check(model, got, t, max_spheres, n_trials, min_inliers=4, seed=0, samples=None, min_radius=0.0, max_radius=math.inf, what=""):
    """every round against the reference, from the alive set the returned labels imply -> the reference's rounds"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    P = max_spheres
    fin = ref.finite_rows(m)
    e = ref.exponent(m)
    lab = got["labels"]
    assert lab.dtype == np.int32 and lab.shape == (len(m),) and not lab[~fin].any() and lab.min(initial=0) >= 0
    assert got["spheres"].shape == (P, 4) and got["best_cost"].dtype == np.int64 and got["refit_used"].dtype == np.int32
    if len(m) == 0:                                                      # no round runs: zeros everywhere
        assert got["n_spheres"] == 0 and not any(got[k].any() for k in KEYS_F + KEYS_I)
        return []
    rounds = []
    n_seen = P
    for p in range(P):
        alive = fin & ((lab == 0) | (lab > p))
        r = ref.round_(m, alive, p, t, n_trials, min_inliers, seed, None if samples is None else np.asarray(samples)[p], min_radius, max_radius, e)
        rounds.append(r)
        print(f"{what} round {p}: device best trial {got['best_trial'][p]} cost {int(got['best_cost'][p])} count {got['best_count'][p]}; "
              f"reference {r['best_trial']} {r['best_cost']} {r['best_count']}")
        assert (got["best_trial"][p], int(got["best_cost"][p]), got["best_count"][p]) == (r["best_trial"], r["best_cost"], r["best_count"]), (what, p)
        if r["stop"]:
            n_seen = p
            break
        want = np.array([*r["centre"], r["R"]], np.float64)
        print(f"{what} round {p}: refit n {int(r['n'])}, max |g| {r['max_g']}, used {r['used']}, sphere {got['spheres'][p].tolist()}, "
              f"reference {want.tolist()}")
        assert got["refit_used"][p] == int(r["used"]), (what, p)
        assert np.array_equal(_bits(got["spheres"][p]), _bits(want)), (what, p)
        c = ref.classify(m, alive, got["spheres"][p, :3], got["spheres"][p, 3], t)
        assert np.array_equal(lab == p + 1, c["mask"]), (what, p)
        assert got["counts"][p] == c["count"] and _bits(got["rmse"][p]) == _bits(c["rmse"]), (what, p)
    assert got["n_spheres"] == n_seen, what
    z = slice(n_seen, P)
    assert not got["spheres"][z].any() and not got["counts"][z].any() and not got["rmse"][z].any() and not got["refit_used"][z].any(), what
    assert lab.max(initial=0) <= n_seen
    zz = slice(min(n_seen + 1, P), P)                                    # the stopping round records its diagnostics
    assert not got["best_trial"][zz].any() and not got["best_cost"][zz].any() and not got["best_count"][zz].any(), what
    return rounds


# ---- 1. the scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, B, mi", (*ref.SCENES, (2051, 300, 100)))
def test_scene_against_the_reference(M, B, mi):
    """three noisy spheres, then a stop: M = 1030 is two 512-row tiles and a 6-row tail (one scoring chunk), 4096 two chunks; 2051 a
    second chunk of 3 rows (the scoring reads a NaN-staged fourth), B = 300 a partial second trial block (the clamped lanes b >= B)"""
    m = _scene(M)
    got = _fit(m, T, max_spheres=ref.SCENE_P, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)
    _check(m, got, T, ref.SCENE_P, B, mi, ref.SCENE_SEED, what=f"scene M = {M}")
    assert got["n_spheres"] == 3 and got["refit_used"][:3].tolist() == [1, 1, 1]
    assert 4 <= got["best_count"][3] < mi
    assert np.abs(got["spheres"][:3, 3] - [5.0, 3.0, 2.0]).max() < 0.01 and (got["rmse"][:3] < 0.03).all()


# ---- 2. a caller's sample table ---------------------------------------------------------------------------------------------------------
def test_sample_table_with_void_trials():
    """an equal pair, an index out of range on either side, four coplanar rows (det == 0) and a row an earlier round removed"""
    m, smp = ref.bad_sample_scene(_scene_labels())
    P, B = smp.shape[:2]
    got = _fit(m, T, max_spheres=P, n_trials=B, min_inliers=40, samples=smp)
    rounds = _check(m, got, T, P, B, 40, samples=smp, what="sample table")
    assert got["n_spheres"] == 3 and not np.isin(got["best_trial"][:3], [0, 1, 2, 3]).any() and got["best_trial"][1] != 4
    for p, r in enumerate(rounds):
        assert r["void"][:4].all() and r["void"][4] == (p > 0)
    # ... and with a base of 1, as the host tiers pass it
    pm, _t = _prepared(m)
    try:
        one = _run(pm, T, max_spheres=P, n_trials=B, min_inliers=40, samples=smp + 1, idx_base=1)
    finally:
        pm.close()
    assert _same(one, got)
    void = np.full((1, 4, 4), 3, np.int32)                                # every trial void: no sphere, trial -1
    none = _fit(m, T, n_trials=4, samples=void)
    assert none["n_spheres"] == 0 and none["best_trial"][0] == -1 and not none["labels"].any()


# ---- 3. the radius bounds -----------------------------------------------------------------------------------------------------------------
def test_radius_bounds():
    m = _scene(1030)
    smp = ref.sample_table(len(m), _scene_labels(), 3, 256, 5)
    kw = dict(min_radius=2.5, max_radius=3.5)
    got = _fit(m, T, max_spheres=3, n_trials=256, min_inliers=40, samples=smp, **kw)
    _check(m, got, T, 3, 256, 40, samples=smp, what="radius 2.5 .. 3.5", **kw)
    assert got["n_spheres"] == 1 and abs(got["spheres"][0, 3] - 3.0) < 0.01           # only the radius-3 sphere, found first
    kw = dict(min_radius=0.0, max_radius=0.01)
    none = _fit(m, T, max_spheres=3, n_trials=256, min_inliers=40, samples=smp, **kw)
    _check(m, none, T, 3, 256, 40, samples=smp, what="radius <= 0.01", **kw)
    assert none["n_spheres"] == 0 and none["best_trial"][0] == -1 and not none["labels"].any()


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows():
    m = np.array(_scene(1030))
    bad = [0, 17, 511, 512, 1029]
    m[bad[0]] = [np.nan, 50, 90]
    m[bad[1]] = [100, np.inf, 90]
    m[bad[2]] = [100, 50, -np.inf]
    m[bad[3]] = [np.nan, np.nan, np.nan]
    m[bad[4]] = [np.inf, np.nan, 95]
    got = _fit(m, T, max_spheres=4, n_trials=256, min_inliers=40, seed=ref.SCENE_SEED)
    _check(m, got, T, 4, 256, 40, ref.SCENE_SEED, what="non-finite rows")
    assert got["n_spheres"] == 3 and not got["labels"][bad].any()
    good = [int(v) for v in np.flatnonzero(_scene_labels() == 1) if v not in bad][:5]
    smp = np.array([[[bad[0], *good[:3]], [good[0], bad[4], good[1], good[2]], good[:4]]], np.int32)
    s = _fit(m, T, n_trials=3, samples=smp)
    rounds = _check(m, s, T, 1, 3, samples=smp, what="non-finite samples")
    assert s["best_trial"][0] == 2 and rounds[0]["void"].tolist() == [True, True, False]


@pytest.mark.parametrize("M", [0, 3, 4])
def test_few_rows(M):
    m = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) + 5)[:M]
    got = _fit(m, 0.1, max_spheres=2, n_trials=32, seed=2)
    _check(m, got, 0.1, 2, 32, 4, 2, what=f"M = {M}")
    assert got["n_spheres"] == (1 if M == 4 else 0) and got["labels"].shape == (M,)
    if M == 4:
        assert got["counts"][0] == 4 and (got["labels"] == 1).all() and got["best_count"][1] == 0 and got["best_trial"][1] == -1


def test_coincident_rows():
    m = np.full((700, 3), 2.5, np.float32)
    got = _fit(m, 0.1, max_spheres=2, n_trials=64)
    rounds = _check(m, got, 0.1, 2, 64, what="coincident")
    assert got["n_spheres"] == 0 and got["best_trial"][0] == -1 and not got["labels"].any() and rounds[0]["void"].all()


def test_knife_edge_rows():
    """rows at exactly radius 9 about (16, 32, 8) and, in pairs on the x axis, rows at R + t (r2 == t2: inliers with q = 2^20), one
    float below (inliers) and one float above (outliers).  min_radius = max_radius = 9 keeps the round's sphere the trial's own exact
    one (the pairs pull the refit's radius off 9), so the final classification meets the same edge as the trial's scoring"""
    m, n = ref.knife_scene()
    t = ref.KNIFE_T
    smp = np.array([[[0, 1, n // 2, n - 1]]], np.int32)
    kw = dict(min_radius=9.0, max_radius=9.0)
    got = _fit(m, t, n_trials=1, samples=smp, **kw)
    _check(m, got, t, 1, 1, samples=smp, what="knife edge", **kw)
    assert got["spheres"][0].tolist() == [*ref.KNIFE_C, 9.0] and got["refit_used"][0] == 0
    assert list(got["labels"][n:]) == [1, 1, 1, 1, 0, 0] and got["counts"][0] == n + 4 and got["best_count"][0] == n + 4
    t2, s = ref.thresholds(t)
    r2 = ref.chain_r2(m[n:], np.array(ref.KNIFE_C, np.float32), np.float32(9.0))
    assert r2[0] == r2[1] == t2 and r2[2] == r2[3] < t2 and (r2[4:] > t2).all()
    q = [int(v) for v in ref.q_of(r2[[0, 2]], s)]
    assert q[0] == ref.QMAX and q[1] < ref.QMAX and got["best_cost"][0] == 2 * (q[0] + q[1]) + 2 * ref.QMAX
    assert _bits(got["rmse"][0]) == _bits(math.sqrt((2 * (q[0] + q[1]) / (n + 4)) * (float(t2) * 2.0 ** -20)))
    free = _fit(m, t, n_trials=1, samples=smp)                             # without the bounds the refit is used
    _check(m, free, t, 1, 1, samples=smp, what="knife edge, refit used")
    assert free["refit_used"][0] == 1 and free["best_cost"][0] == got["best_cost"][0] and free["spheres"][0, 3] > 9.0


def test_refit_not_used_returns_the_trial():
    """radius bounds so tight that the trial's Rf passes and the refit's (float)R does not: the returned sphere is the trial's bits"""
    m = _scene(1030)
    M, B, mi = ref.SCENES[0]
    plain = _fit(m, T, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)
    r0 = ref.round_(m, ref.finite_rows(m), 0, T, B, mi, ref.SCENE_SEED)
    p0, cf, Rf = r0["trial"]
    assert plain["best_trial"][0] == r0["best_trial"] and plain["refit_used"][0] == 1
    kw = dict(min_radius=float(Rf), max_radius=float(Rf))
    got = _fit(m, T, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED, **kw)
    _check(m, got, T, 1, B, mi, ref.SCENE_SEED, what="refit not used", **kw)
    assert got["n_spheres"] == 1 and got["refit_used"][0] == 0 and got["best_trial"][0] == plain["best_trial"][0]
    assert np.array_equal(_bits(got["spheres"][0]), _bits([float(v) for v in cf] + [float(Rf)]))


# ---- 5. identical bits ---------------------------------------------------------------------------------------------------------------
def _buffers(M, P, need, fill=-7):
    i32, f64 = torch.int32, torch.float64
    return (torch.full((M,), fill, dtype=i32, device=_dev()), torch.full((P, 4), float(fill), dtype=f64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((P,), float(fill), dtype=f64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((1,), fill, dtype=i32, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((P,), fill, dtype=torch.int64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((need,), 0x5A, dtype=torch.uint8, device=_dev()))


def test_identical_bits_across_calls_streams_and_a_shuffle():
    from pcreg_amd._lib import lib
    m = _scene(4096)
    M, P, B = len(m), 4, 256
    kw = dict(max_spheres=P, n_trials=B, min_inliers=200, seed=ref.SCENE_SEED)
    pm, _t = _prepared(m)
    try:
        a = _run(pm, T, **kw)
        b = _run(pm, T, **kw)
        assert _same(a, b) and a["n_spheres"] == 3
        need = max(int(lib().pcreg_dev_model_fit_spheres_workspace(M, B)), 256)
        outs = [_buffers(M, P, need) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.fit_spheres(T, out=o, **kw)
        torch.cuda.synchronize()
        for o in outs:
            assert _same(_host(dict(zip(NAMES, o[:9]))), a)
    finally:
        pm.close()
    # a shuffled copy with the sample table mapped through the permutation: the integer sums know no order
    smp = ref.sample_table(M, a["labels"], P, B, 17)
    c = _fit(m, T, samples=smp, **kw)
    rng = np.random.default_rng(17)
    perm = rng.permutation(M)                                          # row j of the copy is row perm[j] of the model
    back = np.empty(M, np.int64)
    back[perm] = np.arange(M)
    d = _fit(m[perm], T, samples=back[smp].astype(np.int32), **kw)
    assert c["n_spheres"] == 3 and np.array_equal(d["labels"][back], c["labels"])
    d2 = dict(d, labels=c["labels"])
    assert _same(d2, c)


# ---- 6. tiers, workspace -----------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    m = _scene(1030)
    smp = ref.sample_table(len(m), _scene_labels(), 2, 64, 4)
    for kw in (dict(max_spheres=5, n_trials=256, min_inliers=40, seed=ref.SCENE_SEED),
               dict(max_spheres=2, n_trials=256, min_inliers=40, min_radius=2.5, max_radius=6.0, seed=3),
               dict(max_spheres=2, n_trials=64, min_inliers=40, samples=smp)):
        want = _fit(m, T, **kw)
        if "samples" in kw:
            kw = dict(kw, samples=smp + 1)                               # the host tiers take 1-based rows
        with pc.Model(m) as h:
            a = h.fit_spheres(T, **kw)
        b = pc.point_fit_spheres(m, T, **kw)
        for got in (a, b):
            assert got["labels"].dtype == np.int32 and got["spheres"].shape == (kw["max_spheres"], 4)
            assert _same(got, want)
        assert want["n_spheres"] >= 1
    e = pc.point_fit_spheres(np.zeros((0, 3)), 0.1, max_spheres=3)
    assert e["n_spheres"] == 0 and e["labels"].shape == (0,) and not e["spheres"].any() and not e["best_count"].any()
    with pytest.raises(ValueError):
        pc.point_fit_spheres(m, 0.0)


def test_workspace_size_is_exact():
    """one byte short is refused as a bad argument; a canary behind the reported size survives"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    m = _scene(4096)
    M, P, B = len(m), 4, 256
    pm, _t = _prepared(m)
    try:
        want = _run(pm, T, max_spheres=P, n_trials=B, min_inliers=200, seed=ref.SCENE_SEED)
        need = int(L.pcreg_dev_model_fit_spheres_workspace(M, B))
        bufs = _buffers(M, P, 1)
        lab, n = bufs[0], bufs[5]
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        args = (pm.handle, T, 0.0, math.inf, P, B, 200, ref.SCENE_SEED, None, 0, *(_p(x) for x in bufs[:9]), _p(ws))
        assert L.pcreg_dev_model_fit_spheres_f32(*args, C.c_size_t(need - 1), None) == _l.PCREG_E_ARG
        assert b"bad argument" in L.pcreg_last_error()
        torch.cuda.synchronize()
        assert (lab == -7).all().item() and (n == -7).all().item()
        _l.check(L.pcreg_dev_model_fit_spheres_f32(*args, C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        got = _host(dict(zip(NAMES, bufs[:9])))
        assert _same(got, want)
    finally:
        pm.close()
