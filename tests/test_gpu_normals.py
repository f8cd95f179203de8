"""Surface normals of a prepared model (knn_normals.hip) on the GPU against tests/normals_ref.py.

Direction: sin(angle to the reference) <= 2^-22 + 16 eps64 / g, g the reference's relative gap (lambda_1 - lambda_0) / ||C||_F.
The first term is the fp32 rounding of a unit vector's three components (at most sqrt(3) 2^-25) with a margin of four, the
second the eigenvector perturbation bound error / gap; a plain-double restatement of the contract's arithmetic measured at most
1.7 eps64 / g against this reference on these families, and 16 leaves about nine times that for the device's square root,
reciprocal square root and division.  Rows with g < 1e-3 are not compared in direction; they may be at most 4 % of a case
(tests/test_normals_ref.py checks the share of every case).  Variation: |v - v_ref| <= 2^-23 v_ref + 64 eps64.
Then the sign rules, the exact cases bit for bit, the edges, culling soundness, determinism and the tiers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import knn_k_ref
import normals_ref as ref

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _soa(x):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
    return t


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    t = _soa(model)
    return PreparedModel(t), t


def _run(pm, k, viewpoint=None, variation=True):
    """-> normals [M, 3] float32, variation [M] float32 (or None) as numpy"""
    res = pm.normals(k, viewpoint=viewpoint, variation=variation)
    torch.cuda.synchronize()
    nrm, var = res if variation else (res, None)
    return np.ascontiguousarray(nrm.cpu().numpy().T), None if var is None else var.cpu().numpy()


def _normals(model, k, viewpoint=None, variation=True):
    pm, _t = _prepared(model)
    try:
        return _run(pm, k, viewpoint, variation)
    finally:
        pm.close()


@functools.lru_cache(maxsize=None)
def _family(name, M=ref.M_FAMILY):
    a = ref.family(name, M)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    return ref.normals(_family(name), k)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sin_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.cross(a, b)
    with np.errstate(invalid="ignore"):
        return np.sqrt((c * c).sum(axis=-1)) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _check_against(nrm, var, r, what=""):
    """direction and variation against the reference dict r; -> (the worst sin / bound, the excluded share)"""
    has = np.isfinite(r["gap"])
    assert np.array_equal(np.isnan(nrm).any(axis=1), ~has), what
    assert np.array_equal(np.isnan(nrm).all(axis=1), ~has), what
    cmp = has & (r["gap"] >= ref.GAP_MIN)
    excluded = 1.0 - cmp[has].mean() if has.any() else 0.0
    assert excluded <= ref.EXCLUDED_CAP, (what, excluded)
    sin = _sin_angle(nrm[cmp], r["normal"][cmp])
    bound = 2.0 ** -22 + 16 * EPS / r["gap"][cmp]
    worst = float((sin / bound).max()) if cmp.any() else 0.0
    print(f"{what}: worst sin(angle) {sin.max() if cmp.any() else 0.0:.3e}, worst sin / bound {worst:.3f}, excluded {100 * excluded:.2f} %")
    assert (sin <= bound).all(), (what, worst)
    if var is not None:
        assert np.array_equal(np.isnan(var), ~has), what
        dv = np.abs(var[has].astype(np.float64) - r["variation"][has])
        vb = 2.0 ** -23 * r["variation"][has] + 64 * EPS
        print(f"{what}: worst |v - v_ref| / bound {float((dv / vb).max()) if has.any() else 0.0:.3f}")
        assert (dv <= vb).all(), what
    return worst, excluded


# ---- 1. families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_families_against_the_reference(name, k):
    nrm, var = _normals(_family(name), k)
    r = _ref(name, k)
    assert (r["n"] == k).all()
    _check_against(nrm, var, r, f"{name} k = {k}")
    # unit length up to the fp32 rounding of the components
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22


# ---- 2. sign --------------------------------------------------------------------------------------------------------------
def _negation_or_equal(a, b):
    same = (_bits(a) == _bits(b)).all(axis=1)
    neg = (_bits(a) == (_bits(b) ^ np.uint32(0x80000000))).all(axis=1)
    nan = np.isnan(a).all(axis=1) & np.isnan(b).all(axis=1)
    return same | neg | nan


@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_sign_rules(name, k):
    model = _family(name)
    mid = (model.astype(np.float64).min(axis=0) + model.astype(np.float64).max(axis=0)) / 2
    vp = mid + np.array([0.0, 0.0, 1000.0])
    r = ref.normals(model, k, viewpoint=vp)
    pm, _t = _prepared(model)
    try:
        plain, var_a = _run(pm, k)
        toward, var_b = _run(pm, k, viewpoint=vp)
    finally:
        pm.close()
    assert np.array_equal(_bits(var_a), _bits(var_b))
    assert _negation_or_equal(plain, toward).all()
    ok_dir = r["gap"] >= ref.GAP_MIN
    # without a viewpoint: the component of largest magnitude is non-negative
    use = ok_dir & (r["big"] > 1e-6)
    assert 1.0 - use.mean() <= 0.01
    want = ref.oriented(r, model)
    assert ((plain[use].astype(np.float64) * want[use]).sum(axis=1) > 0).all()
    j = np.argmax(np.abs(plain), axis=1)
    assert (plain[np.arange(len(plain)), j] >= 0).all()
    # with a viewpoint: towards it, and n . (v - p) >= 0 in the contract's own arithmetic for EVERY finite row
    use = ok_dir & (np.abs(r["toward"]) > 1e-6)
    assert 1.0 - use.mean() <= 0.01
    want = ref.oriented(r, model, vp)
    assert ((toward[use].astype(np.float64) * want[use]).sum(axis=1) > 0).all()
    d = vp[None, :] - model.astype(np.float64)
    n64 = toward.astype(np.float64)
    s = (n64[:, 0] * d[:, 0] + n64[:, 1] * d[:, 1]) + n64[:, 2] * d[:, 2]
    assert (s >= 0).all()


# ---- 3. exact cases, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 5, 9])
def test_lattice_in_a_plane_is_exact(k):
    """32 x 32 integer lattice in z = 7: ties at the k-th neighbour everywhere; every normal exactly (0, 0, +-1), variation 0"""
    g = np.arange(32, dtype=np.float32)
    pts = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    pm, _t = _prepared(pts)
    try:
        up, var = _run(pm, k)
        down, var2 = _run(pm, k, viewpoint=(16.0, 16.0, -50.0))
    finally:
        pm.close()
    assert (up == np.array([0, 0, 1], np.float32)).all()
    assert (down == np.array([0, 0, -1], np.float32)).all()
    assert (var == 0).all() and (var2 == 0).all()


@pytest.mark.parametrize("k", [3, 8])
def test_three_rows_carry_the_triangle_normal(k):
    flat = np.array([[0, 0, 5], [4, 0, 5], [0, 4, 5]], np.float32)            # in z = 5: exact
    nrm, var = _normals(flat, k)
    assert (nrm == np.array([0, 0, 1], np.float32)).all() and (var == 0).all()
    tri = np.array([[1, 2, 3], [4, 2, 5], [2, 6, 4]], np.float32)
    nrm, var = _normals(tri, k)
    r = ref.normals(tri, k)
    assert (r["n"] == 3).all()
    _check_against(nrm, var, r, f"triangle k = {k}")
    want = np.cross(tri[1].astype(float) - tri[0], tri[2].astype(float) - tri[0])
    assert (_sin_angle(nrm, want[None]) <= 2.0 ** -22).all()


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
def test_fewer_than_three_rows():
    for M in (0, 1, 2):
        nrm, var = _normals(np.arange(3 * M, dtype=np.float32).reshape(M, 3) * 1.5, 3)
        assert nrm.shape == (M, 3) and var.shape == (M,)
        assert np.isnan(nrm).all() and np.isnan(var).all()


@pytest.mark.parametrize("M", [511, 512, 513, 1025])
def test_tile_boundaries(M):
    model = _family("volume")[:M]
    nrm, var = _normals(model, 8)
    _check_against(nrm, var, ref.normals(model, 8), f"volume[:{M}] k = 8")


def test_non_finite_rows():
    model = _family("sheet")[:700].copy()
    bad = model.copy()
    bad[100, 1] = np.nan
    bad[650, 0] = np.inf
    keep = np.setdiff1d(np.arange(700), [100, 650])
    for k in (6, 17):
        nrm, var = _normals(bad, k)
        assert np.isnan(nrm[[100, 650]]).all() and np.isnan(var[[100, 650]]).all()
        nrm0, var0 = _normals(model[keep], k)
        assert np.array_equal(_bits(nrm[keep]), _bits(nrm0))
        assert np.array_equal(_bits(var[keep]), _bits(var0))
        assert not np.isnan(nrm0).any()


def test_coincident_rows():
    nrm, var = _normals(np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (5, 1)), 4)
    assert np.isnan(nrm).all() and np.isnan(var).all()


def test_padding_and_no_variation():
    """ldn > M leaves the padding untouched; variation NULL gives the same normals"""
    from pcreg_amd._lib import check, lib
    model = _family("volume")[:300]
    M, pad = 300, 7
    pm, _t = _prepared(model)
    try:
        want, _var = _run(pm, 9)
        only = _run(pm, 9, variation=False)[0]
        assert np.array_equal(_bits(only), _bits(want))
        big = torch.full((3, M + pad), -7.0, dtype=torch.float32, device=_dev())
        need = int(lib().pcreg_dev_model_normals_workspace(M, 9))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
        pm.normals(9, out=(big[:, :M], None, ws))
        torch.cuda.synchronize()
        got = big.cpu().numpy()
        assert np.array_equal(_bits(got[:, :M].T), _bits(want)) and (got[:, M:] == -7.0).all()
        # ldn < M is refused
        L = lib()
        assert L.pcreg_dev_model_normals_f32(pm.handle, 9, None, _p(big), M - 1, None, _p(ws), ws.numel(), None) == 1
        check(L.pcreg_dev_model_normals_f32(pm.handle, 9, None, _p(big), M, None, _p(ws), ws.numel(), None))
        torch.cuda.synchronize()
    finally:
        pm.close()


# ---- 5. culling soundness -------------------------------------------------------------------------------------------------
def test_small_cluster_takes_neighbours_from_the_far_one(debug_set):
    """5 rows spread over a plane patch and 600 rows in a small ball 1000 units away, k = 8: each of the five takes three far rows"""
    rng = np.random.default_rng(11)
    small = np.column_stack([rng.uniform(0, 100, (5, 2)), rng.normal(0, 1, 5)])
    ball = rng.normal(0, 0.5, (600, 3)) + np.array([1000.0, 30.0, 10.0])
    order = rng.permutation(605)
    model = np.vstack([small, ball])[order].astype(np.float32)
    small_rows = np.flatnonzero(order < 5)
    idx, _d = knn_k_ref.knn(model[small_rows], model, 8)
    assert all(np.isin(row, small_rows).sum() == 5 for row in idx)          # five own rows, three far ones
    r = ref.normals(model, 8)
    assert (r["gap"][small_rows] >= ref.GAP_MIN).all()
    pm, _t = _prepared(model)
    try:
        nrm, var = _run(pm, 8)
        debug_set("knn_nocull", 1)
        nrm2, var2 = _run(pm, 8)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    _check_against(nrm, var, r, "two clusters k = 8")
    assert np.array_equal(_bits(nrm), _bits(nrm2)) and np.array_equal(_bits(var), _bits(var2))


# ---- 6. determinism -------------------------------------------------------------------------------------------------------
def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def test_determinism_on_the_large_sheet(debug_set):
    from pcreg_amd._lib import lib
    model = _family("sheet", 65536)
    k = 16
    vp = (120.0, 70.0, 500.0)
    pm, _t = _prepared(model)
    try:
        debug_set("knn_stats", 1)
        _stats()
        a = _run(pm, k, vp)
        searches, visited, nominal, _tail = _stats()
        n_tiles = (len(model) + 511) // 512
        print(f"sheet M = 65536 k = 16: {visited} of {nominal} tile visits ({100.0 * visited / nominal:.2f} %)")
        assert searches == 1 and nominal == n_tiles * n_tiles and 0 < visited < nominal
        debug_set("knn_stats", 0)
        b = _run(pm, k, vp)
        debug_set("knn_nocull", 1)
        c = _run(pm, k, vp)
        debug_set("knn_nocull", 0)
        for other in (b, c):
            assert np.array_equal(_bits(a[0]), _bits(other[0])) and np.array_equal(_bits(a[1]), _bits(other[1]))
        assert not np.isnan(a[0]).any()
        # two streams sharing the handle, buffers of their own
        M = pm.M
        need = max(int(lib().pcreg_dev_model_normals_workspace(M, k)), 256)
        outs = [(torch.full((3, M), -7.0, dtype=torch.float32, device=_dev()), torch.full((M,), -7.0, dtype=torch.float32, device=_dev()),
                 torch.empty(need, dtype=torch.uint8, device=_dev())) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.normals(k, viewpoint=vp, variation=True, out=o)
        torch.cuda.synchronize()
        for o in outs:
            assert np.array_equal(_bits(o[0].cpu().numpy().T), _bits(a[0])) and np.array_equal(_bits(o[1].cpu().numpy()), _bits(a[1]))
    finally:
        pm.close()


# ---- 7. tiers -------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    model = _family("volume")
    vp = (3.0, -4.0, 500.0)
    for viewpoint in (None, vp):
        want_n, want_v = _normals(model, 9, viewpoint)
        with pc.Model(model) as h:
            a = h.normals(9, viewpoint=viewpoint, variation=True)
            only = h.normals(9, viewpoint=viewpoint)
        b = pc.point_normals(model, 9, viewpoint=viewpoint, variation=True)
        for nrm, var in (a, b):
            assert nrm.dtype == var.dtype == np.float32 and nrm.shape == (len(model), 3)
            assert np.array_equal(_bits(nrm), _bits(want_n)) and np.array_equal(_bits(var), _bits(want_v))
        assert np.array_equal(_bits(only), _bits(want_n))
    assert pc.point_normals(np.zeros((0, 3)), 3).shape == (0, 3)
    with pytest.raises(ValueError):
        pc.point_normals(model, 2)
    with pytest.raises(ValueError):
        pc.point_normals(model, 33)


def test_workspace_size_is_exact():
    """one byte short is refused with the k-nearest launcher's code; a canary behind the reported size survives"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    model = _family("sheet")
    M = len(model)
    pm, _t = _prepared(model)
    try:
        need = int(L.pcreg_dev_model_normals_workspace(M, 16))
        assert need == -(-4 * M // 256) * 256
        nrm = torch.empty((3, M), dtype=torch.float32, device=_dev())
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        assert L.pcreg_dev_model_normals_f32(pm.handle, 16, None, _p(nrm), M, None, _p(ws), C.c_size_t(need - 1), None) == _l.PCREG_E_WORKSPACE
        # (the k-nearest launcher's code for the same mistake)
        q = _soa(model[:4])
        idx = torch.empty((4, 16), dtype=torch.int32, device=_dev())
        dist = torch.empty((4, 16), dtype=torch.float32, device=_dev())
        kneed = int(L.pcreg_dev_model_knn_workspace(4, M, 16))
        kws = torch.empty(kneed, dtype=torch.uint8, device=_dev())
        assert L.pcreg_dev_model_knn_f32(pm.handle, _p(q), 4, 4, 16, 0, _p(idx), _p(dist), _p(kws), C.c_size_t(kneed - 1), None) == _l.PCREG_E_WORKSPACE
        _l.check(L.pcreg_dev_model_normals_f32(pm.handle, 16, None, _p(nrm), M, None, _p(ws), C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        assert np.array_equal(_bits(nrm.cpu().numpy().T), _bits(_run(pm, 16)[0]))
    finally:
        pm.close()
