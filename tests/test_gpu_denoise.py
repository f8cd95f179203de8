"""Statistical outlier removal of a prepared model (knn_denoise.hip) on the GPU against tests/denoise_ref.py.

mean_dist: |d - d_ref| <= (k + 3) 2^-52 d_ref -- one rounding per square root at 2^-52, up to k additions and one division at 2^-53
each, to first order; the NaNs in the same places.
thr: |thr - thr_ref| <= (nf + 2 k + 16) 2^-52 (mu_ref + t (dmax_ref + mu_ref + sd_ref)) -- worst-case summation of nf positive
terms for mu, and the perturbation of the two-pass deviation sum by the errors in d_i and in mu, via Cauchy-Schwarz.
The inlier list is the mask d_i <= thr restated on the RETURNED doubles, bit for bit, and equals the reference's set: no row of
any case lies within a relative 1e-7 of the threshold (tests/test_denoise_ref.py), the rounding is about 5e-13, so none is excused.
Then the exact cases bit for bit, the edges, culling soundness, the tiers and determinism."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import denoise_ref as ref
import normals_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -52


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _soa(x):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.array(x.T, order="C")))          # (a copy: the families are read-only arrays)
    return t


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    t = _soa(model)
    return PreparedModel(t), t


def _host(res):
    """a PreparedModel.denoise dict as numpy: mean_dist [M], inliers [n], stats [4]"""
    torch.cuda.synchronize()
    n = int(res["n_inliers"].cpu().item())
    return dict(mean_dist=res["mean_dist"].cpu().numpy(), inliers=res["inliers"].cpu().numpy()[:n], stats=res["stats"].cpu().numpy())


def _run(pm, k, t):
    return _host(pm.denoise(k, t))


def _denoise(model, k, t):
    pm, _t = _prepared(model)
    try:
        return _run(pm, k, t)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(a, b):
    return (np.array_equal(_bits(a["mean_dist"]), _bits(b["mean_dist"])) and np.array_equal(a["inliers"], b["inliers"])
            and np.array_equal(_bits(a["stats"]), _bits(b["stats"])))


@functools.lru_cache(maxsize=None)
def _family(name):
    a = ref.family(name)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(name, k, t):
    return ref.denoise(_family(name), k, t)


def _check_mask(got, M):
    """the list is the mask on the returned doubles: ascending, the matching count, int32 rows inside the model"""
    inl = got["inliers"]
    assert inl.dtype == np.int32
    assert np.array_equal(inl, ref.inliers_of(got["mean_dist"], got["stats"][0]))
    assert (np.diff(inl) > 0).all() and (len(inl) == 0 or (inl[0] >= 0 and inl[-1] < M))


def _check_against(got, r, k, t, what=""):
    """-> (the worst |d - d_ref| / bound, |thr - thr_ref| / bound)"""
    L = np.longdouble
    d, dr = got["mean_dist"], r["mean_dist"]
    assert np.array_equal(np.isnan(d), np.isnan(dr)), what
    fin = np.isfinite(dr)
    thr, mu, sd, nf = got["stats"]
    assert nf == r["nf"], what
    share_d = share_t = 0.0
    if fin.any():
        err = np.abs(d[fin].astype(L) - dr[fin])
        bound = (k + 3) * U * dr[fin]
        pos = bound > 0
        share_d = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
        tb = (r["nf"] + 2 * k + 16) * U * (r["mu"] + L(t) * (r["dmax"] + r["mu"] + r["sd"]))
        te = abs(L(thr) - r["thr"])
        share_t = float(te / tb) if tb > 0 else 0.0
        print(f"{what}: worst |d - d_ref| / bound {share_d:.3f}, |thr - thr_ref| / bound {share_t:.4f}, "
              f"{len(got['inliers'])} inliers of {len(d)}")
        assert (err <= bound).all(), (what, share_d)
        assert te <= tb, (what, share_t)
        assert abs(L(mu) - r["mu"]) <= (r["nf"] + 2 * k + 16) * U * r["mu"], what          # (the same bound at t = 0, where thr is mu)
    else:
        assert np.isnan(thr) and np.isnan(mu) and np.isnan(sd), what
    _check_mask(got, len(d))
    assert np.array_equal(got["inliers"], r["inliers"]), what
    return share_d, share_t


# ---- 1. families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ref.TS)
@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_families_against_the_reference(name, k, t):
    r = _ref(name, k, t)
    assert (r["n"] == k + 1).all() and r["rel_gap"] >= ref.GAP_MIN
    got = _denoise(_family(name), k, t)
    _check_against(got, r, k, t, f"{name} k = {k} t = {t}")
    assert 0 < len(got["inliers"]) < ref.M_FAMILY          # (real outliers exist, and are removed)


# ---- 2. exact cases, bit for bit ------------------------------------------------------------------------------------------
def _lattice():
    g = np.arange(32, dtype=np.float32)
    return np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])


@pytest.mark.parametrize("t", [0.0, 1.0, 2.5])
def test_lattice_with_two_neighbours_is_exact(t):
    """32 x 32 unit lattice in z = 7, k = 2: every row has two rows at distance 1; stats {1, 1, 0, 1024}; all inliers at any t"""
    got = _denoise(_lattice(), 2, t)
    assert (got["mean_dist"] == 1.0).all()
    assert np.array_equal(got["stats"], np.array([1.0, 1.0, 0.0, 1024.0]))
    assert np.array_equal(got["inliers"], np.arange(1024, dtype=np.int32))


def test_lattice_with_four_neighbours_is_exact_inside():
    pts = _lattice()
    got = _denoise(pts, 4, 1.0)
    inside = ((pts[:, 0] >= 1) & (pts[:, 0] <= 30) & (pts[:, 1] >= 1) & (pts[:, 1] <= 30))
    assert (got["mean_dist"][inside] == 1.0).all()
    corner = (1.0 + 1.0 + np.sqrt(2.0) + 2.0) / 4.0
    assert abs(got["mean_dist"][0] - corner) <= 7 * U * corner
    _check_against(got, ref.denoise(pts, 4, 1.0), 4, 1.0, "lattice k = 4")


@pytest.mark.parametrize("k", [1, 4, 15, 31])
def test_coincident_rows(k):
    """k + 2 coincident rows: every distance 0, thr 0, every row an inlier"""
    got = _denoise(np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (k + 2, 1)), k, 1.0)
    assert np.array_equal(_bits(got["mean_dist"]), _bits(np.zeros(k + 2)))
    assert np.array_equal(_bits(got["stats"]), _bits(np.array([0.0, 0.0, 0.0, k + 2.0])))
    assert np.array_equal(got["inliers"], np.arange(k + 2, dtype=np.int32))


# ---- 3. edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 9])
def test_few_rows(k):
    """M = 0, 1, 2, k, k + 1, k + 2: fewer than k + 1 rows shorten the neighbourhood; one row (or none) has no distance"""
    base = _family("volume")
    for M in sorted({0, 1, 2, k, k + 1, k + 2}):
        model = base[:M]
        got = _denoise(model, k, 1.0)
        assert got["mean_dist"].shape == (M,)
        r = ref.denoise(model, k, 1.0)
        assert (r["n"] == min(M, k + 1)).all()
        _check_against(got, r, k, 1.0, f"volume[:{M}] k = {k}")
        if M == 0:
            assert np.isnan(got["stats"][:3]).all() and got["stats"][3] == 0 and len(got["inliers"]) == 0
        if M == 1:
            assert np.isnan(got["mean_dist"]).all() and np.isnan(got["stats"][:3]).all() and got["stats"][3] == 0
            assert len(got["inliers"]) == 0
        if M == 2:
            assert got["stats"][3] == 2 and got["stats"][2] == 0 and len(got["inliers"]) == 2      # one distance, both ways


@pytest.mark.parametrize("M", [511, 512, 513, 1025, 2049])
def test_tile_and_chunk_boundaries(M):
    model = np.vstack([_family("volume"), _family("sheet")])[:M]
    got = _denoise(model, 8, 1.0)
    _check_against(got, ref.denoise(model, 8, 1.0), 8, 1.0, f"M = {M} k = 8")


def test_non_finite_rows():
    model = _family("sheet")[:700].copy()
    bad = model.copy()
    bad[100, 1] = np.nan
    bad[650, 0] = np.inf
    keep = np.setdiff1d(np.arange(700), [100, 650])
    for k in (6, 17):
        got = _denoise(bad, k, 1.0)
        clean = _denoise(model[keep], k, 1.0)
        assert np.isnan(got["mean_dist"][[100, 650]]).all()
        assert np.array_equal(_bits(got["mean_dist"][keep]), _bits(clean["mean_dist"]))
        assert not np.isnan(clean["mean_dist"]).any()
        assert got["stats"][3] == 698 and not np.isin([100, 650], got["inliers"]).any()
        _check_against(got, ref.denoise(bad, k, 1.0), k, 1.0, f"non-finite rows k = {k}")


def test_outputs_omitted():
    """mean_dist, inliers (with its count) or stats NULL: the others keep their bits; inliers without a count is refused"""
    from pcreg_amd._lib import lib, PCREG_E_ARG
    model = _family("volume")[:900]
    M, k, t = 900, 5, 1.0
    pm, _t = _prepared(model)
    try:
        want = _run(pm, k, t)
        need = max(int(lib().pcreg_dev_model_denoise_workspace(M, k)), 256)
        new = lambda: (torch.full((M,), -7.0, dtype=torch.float64, device=_dev()), torch.full((M,), -7, dtype=torch.int32, device=_dev()),
                       torch.full((1,), -7, dtype=torch.int32, device=_dev()), torch.full((4,), -7.0, dtype=torch.float64, device=_dev()),
                       torch.empty(need, dtype=torch.uint8, device=_dev()))
        md, inl, n, st, ws = new()
        pm.denoise(k, t, out=(None, inl, n, st, ws))
        got = _host(dict(mean_dist=md, inliers=inl, n_inliers=n, stats=st))
        assert np.array_equal(got["inliers"], want["inliers"]) and np.array_equal(_bits(got["stats"]), _bits(want["stats"]))
        md, inl, n, st, ws = new()
        pm.denoise(k, t, out=(md, None, None, st, ws))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(md.cpu().numpy()), _bits(want["mean_dist"])) and np.array_equal(_bits(st.cpu().numpy()), _bits(want["stats"]))
        md, inl, n, st, ws = new()
        pm.denoise(k, t, out=(md, None, n, None, ws))
        torch.cuda.synchronize()
        assert int(n.cpu().item()) == len(want["inliers"]) and np.array_equal(_bits(md.cpu().numpy()), _bits(want["mean_dist"]))
        md, inl, n, st, ws = new()
        pm.denoise(k, t, out=(md, inl, n, None, ws))
        got = _host(dict(mean_dist=md, inliers=inl, n_inliers=n, stats=st))
        assert np.array_equal(got["inliers"], want["inliers"]) and (inl.cpu().numpy()[len(want["inliers"]):] == -7).all()
        L = lib()
        assert L.pcreg_dev_model_denoise_f32(pm.handle, k, t, _p(md), _p(inl), None, _p(st), _p(ws), ws.numel(), None) == PCREG_E_ARG
    finally:
        pm.close()


def test_workspace_size_is_exact():
    """one byte short is refused as a bad argument; a canary behind the reported size survives"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    model = _family("sheet")
    M, k = len(model), 15
    pm, _t = _prepared(model)
    try:
        want = _run(pm, k, 1.0)
        need = int(L.pcreg_dev_model_denoise_workspace(M, k))
        r256 = lambda b: -(-b // 256) * 256
        assert need == r256(4 * M) + r256(8 * M) + 2 * r256(8 * 1) + 2 * r256(4 * 1) + 256
        md = torch.empty(M, dtype=torch.float64, device=_dev())
        inl = torch.empty(M, dtype=torch.int32, device=_dev())
        n = torch.empty(1, dtype=torch.int32, device=_dev())
        st = torch.empty(4, dtype=torch.float64, device=_dev())
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        assert L.pcreg_dev_model_denoise_f32(pm.handle, k, 1.0, _p(md), _p(inl), _p(n), _p(st), _p(ws), C.c_size_t(need - 1), None) == _l.PCREG_E_ARG
        assert b"bad argument" in L.pcreg_last_error()
        _l.check(L.pcreg_dev_model_denoise_f32(pm.handle, k, 1.0, _p(md), _p(inl), _p(n), _p(st), _p(ws), C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        assert _same(_host(dict(mean_dist=md, inliers=inl, n_inliers=n, stats=st)), want)
    finally:
        pm.close()


# ---- 4. culling soundness -------------------------------------------------------------------------------------------------
def test_small_cluster_takes_neighbours_from_the_far_one(debug_set):
    """5 rows spread over a plane patch and 600 rows in a small ball 1000 units away, k = 7: each of the five takes three far rows,
    its mean distance is hundreds of units, and it is an outlier"""
    import knn_k_ref
    rng = np.random.default_rng(11)
    small = np.column_stack([rng.uniform(0, 100, (5, 2)), rng.normal(0, 1, 5)])
    ball = rng.normal(0, 0.5, (600, 3)) + np.array([1000.0, 30.0, 10.0])
    order = rng.permutation(605)
    model = np.vstack([small, ball])[order].astype(np.float32)
    small_rows = np.flatnonzero(order < 5)
    idx, _d = knn_k_ref.knn(model[small_rows], model, 8)
    assert all(np.isin(row, small_rows).sum() == 5 for row in idx)          # five own rows, three far ones
    r = ref.denoise(model, 7, 1.0)
    pm, _t = _prepared(model)
    try:
        a = _run(pm, 7, 1.0)
        debug_set("knn_nocull", 1)
        b = _run(pm, 7, 1.0)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    _check_against(a, r, 7, 1.0, "two clusters k = 7")
    assert _same(a, b)
    assert (a["mean_dist"][small_rows] > 300).all() and not np.isin(small_rows, a["inliers"]).any()


# ---- 5. tiers -------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    model = _family("volume")
    for k, t in ((4, 1.0), (9, 0.0)):
        want = _denoise(model, k, t)
        with pc.Model(model) as h:
            a = h.denoise(k, t)
        b = pc.point_denoise(model, k, t)
        for got in (a, b):
            assert got["mean_dist"].dtype == np.float64 and got["inliers"].dtype == np.int32
            assert np.array_equal(_bits(got["mean_dist"]), _bits(want["mean_dist"]))
            assert np.array_equal(got["inliers"], want["inliers"])
            assert np.array_equal(_bits([got["thr"], got["mean"], got["std"], float(got["n_finite"])]), _bits(want["stats"]))
    with pc.Model(model) as h:
        assert np.array_equal(h.denoise()["inliers"], _denoise(model, 4, 1.0)["inliers"])          # the defaults: 4 and 1.0
    e = pc.point_denoise(np.zeros((0, 3)))
    assert e["mean_dist"].shape == (0,) and e["inliers"].shape == (0,) and np.isnan(e["thr"]) and e["n_finite"] == 0
    for bad in (0, 32):
        with pytest.raises(ValueError):
            pc.point_denoise(model, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.point_denoise(model, 4, bad)


# ---- 6. determinism -------------------------------------------------------------------------------------------------------
def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def test_determinism_on_the_large_sheet(debug_set):
    from pcreg_amd._lib import lib
    model = normals_ref.family("sheet", 65536)
    k, t = 15, 1.0
    pm, _t = _prepared(model)
    try:
        debug_set("knn_stats", 1)
        _stats()
        a = _run(pm, k, t)
        searches, visited, nominal, _tail = _stats()
        n_tiles = (len(model) + 511) // 512
        print(f"sheet M = 65536 k = 15: {visited} of {nominal} tile visits ({100.0 * visited / nominal:.2f} %)")
        assert searches == 1 and nominal == n_tiles * n_tiles and 0 < visited < nominal
        debug_set("knn_stats", 0)
        b = _run(pm, k, t)
        debug_set("knn_nocull", 1)
        c = _run(pm, k, t)
        debug_set("knn_nocull", 0)
        assert _same(a, b) and _same(a, c)
        assert not np.isnan(a["mean_dist"]).any() and a["stats"][3] == 65536
        _check_mask(a, 65536)
        # two streams sharing the handle, buffers of their own
        M = pm.M
        need = max(int(lib().pcreg_dev_model_denoise_workspace(M, k)), 256)
        outs = [(torch.full((M,), -7.0, dtype=torch.float64, device=_dev()), torch.full((M,), -7, dtype=torch.int32, device=_dev()),
                 torch.full((1,), -7, dtype=torch.int32, device=_dev()), torch.full((4,), -7.0, dtype=torch.float64, device=_dev()),
                 torch.full((need,), 0x5A, dtype=torch.uint8, device=_dev())) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.denoise(k, t, out=o)
        torch.cuda.synchronize()
        for o in outs:
            assert _same(_host(dict(mean_dist=o[0], inliers=o[1], n_inliers=o[2], stats=o[3])), a)
    finally:
        pm.close()
