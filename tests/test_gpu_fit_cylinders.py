"""MSAC cylinder fitting and extraction on a prepared model (knn_fitcylinder.hip) on the GPU against
tests/cylinders_ref.py.

Per round, from the alive set the returned labels imply: best_trial, best_cost and best_count EQUAL to the reference (exact fmaf
chain, IEEE root, integer sums); cylinders, extents and refit_used bit for bit equal to finish64 on the reference's integer sums;
labels, counts, rmse and extents EQUAL to the classification restated from the RETURNED cylinder.  No row is excluded anywhere.
Then the sample table, the radius bounds and the angle rule, the edge clouds, the knife edge, the refit that is not used,
determinism (calls, streams, a shuffle, negated normals), normals given or computed, the tiers and the workspace.
tests/test_cylinders_ref.py asserts the premises of these scenes on the CPU."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import cylinders_ref as ref

pytestmark = pytest.mark.gpu

T, RMAX = ref.SCENE_T, ref.SCENE_RMAX


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
    """a PreparedModel.fit_cylinders dict as numpy"""
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out["n_cylinders"] = int(out["n_cylinders"][0])
    return out


def _run(pm, nrm_t, t, samples=None, **kw):
    if samples is not None:
        samples = torch.from_numpy(np.ascontiguousarray(samples, np.int32)).to(_dev())
    return _host(pm.fit_cylinders(t, nrm_t, samples=samples, **kw))


def _fit(model, nrm, t, **kw):
    pm, _t = _prepared(model)
    try:
        return _run(pm, _soa(nrm), t, **kw)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


KEYS_F, KEYS_I = ("cylinders", "extents", "rmse"), ("labels", "counts", "refit_used", "best_trial", "best_cost", "best_count")
NAMES = ("labels", "cylinders", "extents", "counts", "rmse", "refit_used", "n_cylinders", "best_trial", "best_cost", "best_count")


def _same(a, b):
    return (a["n_cylinders"] == b["n_cylinders"] and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS_F)
            and all(np.array_equal(a[k], b[k]) for k in KEYS_I))


@functools.lru_cache(maxsize=None)
def _scene(M):
    m, n, kind = ref.scene(M)
    for a in (m, n, kind):
        a.setflags(write=False)
    return m, n, kind


def _check(model, nrm, got, t, max_cylinders, n_trials, min_inliers=4, seed=0, samples=None, min_radius=0.0, max_radius=math.inf,
           ref_vec=None, max_angle=math.pi / 2, what=""):
    """every round against the reference, from the alive set the returned labels imply -> the reference's rounds"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    P = max_cylinders
    fin = ref.finite_rows(m)
    e = ref.exponent(m)
    lab = got["labels"]
    assert lab.dtype == np.int32 and lab.shape == (len(m),) and not lab[~fin].any() and lab.min(initial=0) >= 0
    assert got["cylinders"].shape == (P, 7) and got["extents"].shape == (P, 2) and got["best_cost"].dtype == np.int64
    assert got["refit_used"].dtype == np.int32
    if len(m) == 0:                                                      # no round runs: zeros everywhere
        assert got["n_cylinders"] == 0 and not any(got[k].any() for k in KEYS_F + KEYS_I)
        return []
    rounds = []
    n_seen = P
    for p in range(P):
        alive = fin & ((lab == 0) | (lab > p))
        r = ref.round_(m, nrm, alive, p, t, n_trials, min_inliers, seed, None if samples is None else np.asarray(samples)[p], min_radius,
                       max_radius, ref_vec, max_angle, e)
        rounds.append(r)
        print(f"{what} round {p}: device best trial {got['best_trial'][p]} cost {int(got['best_cost'][p])} count {got['best_count'][p]}; "
              f"reference {r['best_trial']} {r['best_cost']} {r['best_count']}")
        assert (got["best_trial"][p], int(got["best_cost"][p]), got["best_count"][p]) == (r["best_trial"], r["best_cost"], r["best_count"]), (what, p)
        if r["stop"]:
            n_seen = p
            break
        want = np.array([*r["centre"], *r["w"], r["R"]], np.float64)
        print(f"{what} round {p}: axis n_n {r['asums'][0]}, max |gn| {r['max_gn']}, max |g| {r['max_g']}, used {r['used']}, cylinder "
              f"{got['cylinders'][p].tolist()}, reference {want.tolist()}")
        assert got["refit_used"][p] == int(r["used"]), (what, p)
        assert np.array_equal(_bits(got["cylinders"][p]), _bits(want)), (what, p)
        c = ref.classify(m, alive, got["cylinders"][p, :3], got["cylinders"][p, 3:6], got["cylinders"][p, 6], t)
        assert np.array_equal(lab == p + 1, c["mask"]), (what, p)
        assert got["counts"][p] == c["count"] and _bits(got["rmse"][p]) == _bits(c["rmse"]), (what, p)
        assert np.array_equal(_bits(got["extents"][p]), _bits(c["extents"])), (what, p)
        cr = ref.classify(m, alive, r["centre"], r["w"], r["R"], t)      # ... and from the reference's own cylinder
        assert np.array_equal(_bits(got["extents"][p]), _bits(cr["extents"])), (what, p)
    assert got["n_cylinders"] == n_seen, what
    z = slice(n_seen, P)
    assert not got["cylinders"][z].any() and not got["extents"][z].any() and not got["counts"][z].any() and not got["rmse"][z].any(), what
    assert not got["refit_used"][z].any() and lab.max(initial=0) <= n_seen
    zz = slice(min(n_seen + 1, P), P)                                    # the stopping round records its diagnostics
    assert not got["best_trial"][zz].any() and not got["best_cost"][zz].any() and not got["best_count"][zz].any(), what
    return rounds


# ---- 1. the scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, B, mi", (*ref.SCENES, (2051, 300, 100)))
def test_scene_against_the_reference(M, B, mi):
    """two noisy cylinders, then a stop: M = 1030 is two 512-row tiles and a 6-row tail (one scoring chunk), 4096 two chunks; 2051 a
    second chunk of 3 rows (the scoring reads a NaN-staged fourth), B = 300 a partial second trial block (the clamped lanes b >= B)"""
    m, nrm, _ = _scene(M)
    kw = dict(max_radius=RMAX, max_cylinders=ref.SCENE_P, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)
    got = _fit(m, nrm, T, **kw)
    _check(m, nrm, got, T, ref.SCENE_P, B, mi, ref.SCENE_SEED, max_radius=RMAX, what=f"scene M = {M}")
    assert got["n_cylinders"] == 2 and got["refit_used"][:2].tolist() == [1, 1]
    assert 4 <= got["best_count"][2] < mi
    assert sorted(np.round(got["cylinders"][:2, 6], 1).tolist()) == [1.5, 3.0] and (got["rmse"][:2] < 0.04).all()
    for cyl, (lo, hi) in zip(got["cylinders"][:2], got["extents"][:2]):  # the axis' extent covers the surface's length (clutter extends it)
        assert hi - lo > (12.0 if round(cyl[6]) == 3 else 8.0) - 0.5


# ---- 2. a caller's sample table ---------------------------------------------------------------------------------------------------------
def test_sample_table_with_void_trials():
    """an equal pair, an index out of range on either side, two rows with exactly parallel normals (L2 == 0), a row with a NaN
    normal, one with a component of 3, and a row an earlier round removed"""
    m, nrm, smp, _ = ref.bad_sample_scene()
    P, B = smp.shape[:2]
    got = _fit(m, nrm, T, max_radius=RMAX, max_cylinders=P, n_trials=B, min_inliers=60, samples=smp)
    rounds = _check(m, nrm, got, T, P, B, 60, samples=smp, max_radius=RMAX, what="sample table")
    assert got["n_cylinders"] == 2 and not np.isin(got["best_trial"][:2], range(7)).any()
    for p, r in enumerate(rounds):
        assert r["void"][:6].all() and r["void"][6] == (p > 0)
    assert (got["labels"][smp[1, 6]] == 1).all()
    # ... and with a base of 1, as the host tiers pass it
    pm, _t = _prepared(m)
    try:
        one = _run(pm, _soa(nrm), T, max_radius=RMAX, max_cylinders=P, n_trials=B, min_inliers=60, samples=smp + 1, idx_base=1)
    finally:
        pm.close()
    assert _same(one, got)
    void = np.full((1, 4, 2), 3, np.int32)                                # every trial void: no cylinder, trial -1
    none = _fit(m, nrm, T, n_trials=4, samples=void)
    assert none["n_cylinders"] == 0 and none["best_trial"][0] == -1 and not none["labels"].any()


# ---- 3. the radius bounds and the angle rule ------------------------------------------------------------------------------------------------
def test_radius_bounds():
    m, nrm, kind = _scene(1030)
    smp = ref.sample_table(len(m), kind, 3, 256, 5)
    kw = dict(min_radius=1.0, max_radius=2.0)
    got = _fit(m, nrm, T, max_cylinders=3, n_trials=256, min_inliers=60, samples=smp, **kw)
    _check(m, nrm, got, T, 3, 256, 60, samples=smp, what="radius 1 .. 2", **kw)
    assert got["n_cylinders"] >= 1 and abs(got["cylinders"][0, 6] - 1.5) < 0.05       # the radius-1.5 cylinder, found first
    assert (np.abs(got["cylinders"][:got["n_cylinders"], 6] - 3.0) > 0.5).all()
    kw = dict(min_radius=0.0, max_radius=0.01)
    none = _fit(m, nrm, T, max_cylinders=3, n_trials=256, min_inliers=60, samples=smp, **kw)
    _check(m, nrm, none, T, 3, 256, 60, samples=smp, what="radius <= 0.01", **kw)
    assert none["n_cylinders"] == 0 and none["best_trial"][0] == -1 and not none["labels"].any()


def test_refit_not_used_returns_the_trial():
    """radius bounds so tight that the trial's Rf passes and the refit's (float)R does not: the returned cylinder is the trial's bits"""
    m, nrm, _ = _scene(1030)
    M, B, mi = ref.SCENES[0]
    plain = _fit(m, nrm, T, max_radius=RMAX, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)
    r0 = ref.round_(m, nrm, ref.finite_rows(m), 0, T, B, mi, ref.SCENE_SEED, max_radius=RMAX)
    p0, af, wf, Rf = r0["trial"]
    assert plain["best_trial"][0] == r0["best_trial"] and plain["refit_used"][0] == 1
    kw = dict(min_radius=float(Rf), max_radius=float(Rf))
    got = _fit(m, nrm, T, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED, **kw)
    _check(m, nrm, got, T, 1, B, mi, ref.SCENE_SEED, what="refit not used", **kw)
    assert got["n_cylinders"] == 1 and got["refit_used"][0] == 0 and got["best_trial"][0] == plain["best_trial"][0]
    assert np.array_equal(_bits(got["cylinders"][0]), _bits([float(v) for v in (*af, *wf, Rf)]))


def test_reference_vector_bounds_the_axis():
    """ref_vec against cylinder 1's axis with 10 degrees: cylinder 1 is found, cylinder 2 (74 degrees away) never, and the returned
    axis points along ref_vec, not along the largest-component rule's choice"""
    m, nrm, _ = _scene(1030)
    M, B, mi = ref.SCENES[0]
    rv = tuple(-v for v in ref.SCENE_CYLINDERS[0][1])
    kw = dict(max_radius=RMAX, ref_vec=rv, max_angle=math.radians(10.0))
    got = _fit(m, nrm, T, max_cylinders=3, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED, **kw)
    _check(m, nrm, got, T, 3, B, mi, ref.SCENE_SEED, what="reference vector", **kw)
    assert got["n_cylinders"] == 1 and abs(got["cylinders"][0, 6] - 3.0) < 0.05
    w = got["cylinders"][0, 3:6]
    assert w @ np.array(rv) / np.linalg.norm(rv) > math.cos(math.radians(3.0)) and w[2] < 0


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows():
    m, nrm = (np.array(a) for a in _scene(1030)[:2])
    kind = _scene(1030)[2]
    bad = [0, 17, 511, 512, 1029]
    m[bad[0]] = [np.nan, 50, 90]
    m[bad[1]] = [100, np.inf, 90]
    m[bad[2]] = [100, 50, -np.inf]
    m[bad[3]] = [np.nan, np.nan, np.nan]
    m[bad[4]] = [np.inf, np.nan, 95]
    got = _fit(m, nrm, T, max_radius=RMAX, max_cylinders=4, n_trials=256, min_inliers=60, seed=ref.SCENE_SEED)
    _check(m, nrm, got, T, 4, 256, 60, ref.SCENE_SEED, max_radius=RMAX, what="non-finite rows")
    assert got["n_cylinders"] == 2 and not got["labels"][bad].any()
    good = [int(v) for v in np.flatnonzero(kind == 1) if v not in bad][:4]
    smp = np.array([[[bad[0], good[0]], [good[0], bad[4]], good[:2]]], np.int32)
    s = _fit(m, nrm, T, n_trials=3, samples=smp)
    rounds = _check(m, nrm, s, T, 1, 3, samples=smp, what="non-finite samples")
    assert s["best_trial"][0] == 2 and rounds[0]["void"].tolist() == [True, True, False]


@pytest.mark.parametrize("M", [0, 1, 2])
def test_few_rows(M):
    m = (np.array([[0, 0, 0], [1, 1, 0]], np.float32) + 5)[:M]
    nrm = np.array([[1, 0, 0], [0, 1, 0]], np.float32)[:M]
    got = _fit(m, nrm, 0.1, max_cylinders=2, n_trials=32, seed=2)
    _check(m, nrm, got, 0.1, 2, 32, 4, 2, what=f"M = {M}")
    assert got["n_cylinders"] == 0 and got["labels"].shape == (M,) and not got["labels"].any()
    if M:
        assert got["best_trial"][0] == -1 and got["best_count"][0] == 0          # two rows make a trial, never four inliers


def test_coincident_rows():
    """700 rows at one point with random normals: every non-void trial is the cylinder of radius 0 through it (d = 0, so s = 0), all
    rows are its inliers and the refit's circle has no extent (N = 0: not used); with min_radius above 0 every trial is void"""
    m = np.full((700, 3), 2.5, np.float32)
    nrm = np.random.default_rng(3).normal(size=(700, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    got = _fit(m, nrm, 0.1, max_cylinders=2, n_trials=64)
    _check(m, nrm, got, 0.1, 2, 64, what="coincident")
    assert got["n_cylinders"] == 1 and got["counts"][0] == 700 and got["refit_used"][0] == 0 and got["cylinders"][0, 6] == 0.0
    assert got["extents"][0].tolist() == [0.0, 0.0] and got["best_trial"][1] == -1
    none = _fit(m, nrm, 0.1, min_radius=0.5, max_cylinders=2, n_trials=64)
    rounds = _check(m, nrm, none, 0.1, 2, 64, min_radius=0.5, what="coincident, min_radius 0.5")
    assert none["n_cylinders"] == 0 and none["best_trial"][0] == -1 and rounds[0]["void"].all()


def test_all_normals_equal():
    m, _, _ = _scene(1030)
    nrm = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (len(m), 1))
    got = _fit(m, nrm, T, max_cylinders=2, n_trials=64, seed=1)
    rounds = _check(m, nrm, got, T, 2, 64, seed=1, what="all normals equal")
    assert got["n_cylinders"] == 0 and got["best_trial"][0] == -1 and not got["labels"].any() and rounds[0]["void"].all()


def test_knife_edge_rows():
    """rows at exactly radius 5 about the line (16, 32, z) and, in pairs on the x axis, rows at R + t (r2 == t2: inliers with
    q = 2^20), one float below (inliers) and one float above (outliers).  With min_radius = max_radius = 5 the RETURNED cylinder is
    the trial's own exact one, ((16, 32, z_0), (0, 0, 1), 5) with z_0 the height of the trial's first row: the refit's axis is free
    and comes out as (0, 0, 1) exactly (every normal has a zero z), but the four inlying pair rows pull the circle's radius above 5,
    (float)R leaves the bounds and the refit is not used.  So the final classification meets the same edge as the trial's scoring."""
    m, nrm, n = ref.knife_scene()
    t = ref.KNIFE_T
    smp = np.array([[list(ref.KNIFE_SAMPLE)]], np.int32)
    kw = dict(min_radius=5.0, max_radius=5.0)
    got = _fit(m, nrm, t, n_trials=1, samples=smp, **kw)
    _check(m, nrm, got, t, 1, 1, samples=smp, what="knife edge", **kw)
    z0 = float(m[ref.KNIFE_SAMPLE[0], 2])
    assert got["cylinders"][0].tolist() == [*ref.KNIFE_C, z0, 0.0, 0.0, 1.0, 5.0] and got["refit_used"][0] == 0
    assert list(got["labels"][n:]) == [1, 1, 1, 1, 0, 0] and got["counts"][0] == n + 4 and got["best_count"][0] == n + 4
    assert got["extents"][0].tolist() == [min(ref.KNIFE_HEIGHTS) - z0, max(ref.KNIFE_HEIGHTS) - z0]
    t2, s = ref.thresholds(t)
    r2 = ref.chain_r2(m[n:], np.array([*ref.KNIFE_C, z0], np.float32), np.array([0, 0, 1], np.float32), np.float32(5.0))
    assert r2[0] == r2[1] == t2 and r2[2] == r2[3] < t2 and (r2[4:] > t2).all()
    q = [int(v) for v in ref.q_of(r2[[0, 2]], s)]
    assert q[0] == ref.QMAX and q[1] < ref.QMAX and got["best_cost"][0] == 2 * (q[0] + q[1]) + 2 * ref.QMAX
    assert _bits(got["rmse"][0]) == _bits(math.sqrt((2 * (q[0] + q[1]) / (n + 4)) * (float(t2) * 2.0 ** -20)))
    free = _fit(m, nrm, t, n_trials=1, samples=smp)                        # without the bounds the refit is used
    _check(m, nrm, free, t, 1, 1, samples=smp, what="knife edge, refit used")
    assert free["refit_used"][0] == 1 and free["best_cost"][0] == got["best_cost"][0] and free["cylinders"][0, 6] > 5.0
    assert free["cylinders"][0, 3:6].tolist() == [0.0, 0.0, 1.0]


# ---- 5. identical bits ---------------------------------------------------------------------------------------------------------------
def _buffers(M, P, need, fill=-7):
    i32, f64 = torch.int32, torch.float64
    return (torch.full((M,), fill, dtype=i32, device=_dev()), torch.full((P, 7), float(fill), dtype=f64, device=_dev()),
            torch.full((P, 2), float(fill), dtype=f64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((P,), float(fill), dtype=f64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((1,), fill, dtype=i32, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((P,), fill, dtype=torch.int64, device=_dev()),
            torch.full((P,), fill, dtype=i32, device=_dev()), torch.full((need,), 0x5A, dtype=torch.uint8, device=_dev()))


def test_identical_bits_across_calls_streams_a_shuffle_and_negated_normals():
    from pcreg_amd._lib import lib
    m, nrm, kind = _scene(4096)
    M, P, B = len(m), 4, 256
    kw = dict(max_radius=RMAX, max_cylinders=P, n_trials=B, min_inliers=200, seed=ref.SCENE_SEED)
    pm, _t = _prepared(m)
    nt = _soa(nrm)
    try:
        a = _run(pm, nt, T, **kw)
        b = _run(pm, nt, T, **kw)
        assert _same(a, b) and a["n_cylinders"] == 2
        need = max(int(lib().pcreg_dev_model_fit_cylinders_workspace(M, B)), 256)
        outs = [_buffers(M, P, need) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.fit_cylinders(T, nt, out=o, **kw)
        torch.cuda.synchronize()
        for o in outs:
            assert _same(_host(dict(zip(NAMES, o[:10]))), a)
        # a random half of the normals negated: the contract says the sign of a normal changes no bit
        rng = np.random.default_rng(23)
        flip = np.where(rng.random(M) < 0.5, -1.0, 1.0).astype(np.float32)
        assert (flip < 0).sum() > M // 3
        assert _same(_run(pm, _soa(nrm * flip[:, None]), T, **kw), a)
    finally:
        pm.close()
    # a shuffled copy of rows and normals with the sample table mapped through the permutation: the integer sums know no order
    smp = ref.sample_table(M, kind, P, B, 17)
    c = _fit(m, nrm, T, samples=smp, **kw)
    rng = np.random.default_rng(17)
    perm = rng.permutation(M)                                          # row j of the copy is row perm[j] of the model
    back = np.empty(M, np.int64)
    back[perm] = np.arange(M)
    d = _fit(m[perm], nrm[perm], T, samples=back[smp].astype(np.int32), **kw)
    assert c["n_cylinders"] == 2 and np.array_equal(d["labels"][back], c["labels"])
    d2 = dict(d, labels=c["labels"])
    assert _same(d2, c)


# ---- 6. normals given or computed, tiers, workspace --------------------------------------------------------------------------------------
def test_normals_computed_in_the_call_equal_normals_given():
    import pcreg_amd as pc
    m, _, _ = _scene(1030)
    kw = dict(max_radius=RMAX, max_cylinders=3, n_trials=256, min_inliers=60, seed=ref.SCENE_SEED)
    with pc.Model(m) as h:
        n12 = h.normals(12)
        a = h.fit_cylinders(T, normals=None, k_normals=12, **kw)
        b = h.fit_cylinders(T, normals=n12, **kw)
    c = pc.point_fit_cylinders(m, T, normals=None, k_normals=12, **kw)
    assert n12.shape == (len(m), 3) and _same(a, b) and _same(c, b) and a["n_cylinders"] >= 1
    _check(m, n12, a, T, 3, 256, 60, ref.SCENE_SEED, max_radius=RMAX, what="normals of k = 12")


def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    m, nrm, kind = _scene(1030)
    smp = ref.sample_table(len(m), kind, 2, 64, 4)
    rv = ref.SCENE_CYLINDERS[1][1]
    for kw in (dict(max_radius=RMAX, max_cylinders=5, n_trials=256, min_inliers=60, seed=ref.SCENE_SEED),
               dict(max_cylinders=2, n_trials=256, min_inliers=60, min_radius=1.0, max_radius=2.0, seed=3),
               dict(max_radius=RMAX, max_cylinders=2, n_trials=256, min_inliers=60, ref_vec=rv, max_angle=0.3, seed=5),
               dict(max_radius=RMAX, max_cylinders=2, n_trials=64, min_inliers=60, samples=smp)):
        want = _fit(m, nrm, T, **kw)
        if "samples" in kw:
            kw = dict(kw, samples=smp + 1)                               # the host tiers take 1-based rows
        with pc.Model(m) as h:
            a = h.fit_cylinders(T, normals=nrm, **kw)
        b = pc.point_fit_cylinders(m, T, normals=nrm, **kw)
        for got in (a, b):
            assert got["labels"].dtype == np.int32 and got["cylinders"].shape == (kw["max_cylinders"], 7)
            assert _same(got, want)
        assert want["n_cylinders"] >= 1
    e = pc.point_fit_cylinders(np.zeros((0, 3)), 0.1, max_cylinders=3)
    assert e["n_cylinders"] == 0 and e["labels"].shape == (0,) and not e["cylinders"].any() and not e["best_count"].any()
    with pytest.raises(ValueError):
        pc.point_fit_cylinders(m, 0.0)


def test_workspace_size_is_exact():
    """one byte short is refused as a bad argument; a canary behind the reported size survives"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    m, nrm, _ = _scene(4096)
    M, P, B = len(m), 4, 256
    pm, _t = _prepared(m)
    nt = _soa(nrm)
    try:
        want = _run(pm, nt, T, max_radius=RMAX, max_cylinders=P, n_trials=B, min_inliers=200, seed=ref.SCENE_SEED)
        need = int(L.pcreg_dev_model_fit_cylinders_workspace(M, B))
        bufs = _buffers(M, P, 1)
        lab, n = bufs[0], bufs[6]
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        args = (pm.handle, T, 0.0, RMAX, None, 0.0, _p(nt), M, P, B, 200, ref.SCENE_SEED, None, 0, *(_p(x) for x in bufs[:10]), _p(ws))
        assert L.pcreg_dev_model_fit_cylinders_f32(*args, C.c_size_t(need - 1), None) == _l.PCREG_E_ARG
        assert b"bad argument" in L.pcreg_last_error()
        torch.cuda.synchronize()
        assert (lab == -7).all().item() and (n == -7).all().item()
        _l.check(L.pcreg_dev_model_fit_cylinders_f32(*args, C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        got = _host(dict(zip(NAMES, bufs[:10])))
        assert _same(got, want)
    finally:
        pm.close()
