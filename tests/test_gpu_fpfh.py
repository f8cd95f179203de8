"""FPFH descriptors of a prepared model (knn_fpfh.hip) on the GPU against tests/fpfh_ref.py.

On the compared rows (tests/test_fpfh_ref.py holds the excluded share of every case under 1 %; none is excluded on these inputs)
the SPFH counts must be EQUAL and the output must satisfy |x - x_ref| <= 64 eps64 * 100 = 1.4e-12: a plain-double restatement of
the contract sits at most 4.3e-14 from the long-double reference on these inputs, and the bound leaves about 30 times that for the
device's division, square root and atan2.  Then the exact cases bit for bit, the edges, culling soundness, determinism, the tiers
and a registration chain."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fpfh_ref as ref
import knn_k_ref

pytestmark = pytest.mark.gpu
UP = np.array([0.0, 0.0, 1.0], np.float32)


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


def _run(pm, k, nrm_soa, spfh=True):
    """-> out [M, 33] float64, counts [M, 33] uint8 (or None) as numpy"""
    res = pm.fpfh(k, nrm_soa, spfh=spfh)
    torch.cuda.synchronize()
    out, cnt = res if spfh else (res, None)
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _fpfh(model, normals, k, spfh=True):
    pm, _t = _prepared(model)
    try:
        return _run(pm, k, _soa(normals), spfh)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_against(out, cnt, r, what=""):
    """counts and output against the reference dict r on the compared rows; -> the worst |x - x_ref| / bound"""
    cmp = ~r["excluded"]
    assert 1.0 - cmp.mean() <= ref.EXCLUDED_CAP if len(cmp) else True, what
    want = np.asarray(r["out"], np.float64)
    assert np.array_equal(np.isnan(out), np.isnan(want)), what
    if cnt is not None:
        assert np.array_equal(cnt[cmp].astype(np.int64), r["counts"][cmp]), what
    fin = cmp & ~np.isnan(want).any(axis=1)
    err = np.abs(out[fin] - want[fin])
    worst = float(err.max() / ref.OUT_TOL) if err.size else 0.0
    print(f"{what}: worst |x - x_ref| {float(err.max()) if err.size else 0.0:.3e}, worst / bound {worst:.4f}, excluded {100 * (1.0 - cmp.mean()) if len(cmp) else 0.0:.2f} %")
    assert (err <= ref.OUT_TOL).all(), (what, worst)
    return worst


# ---- 1. families, with and without culling -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_families_against_the_reference(name, k, debug_set):
    model, nrm = ref.family_inputs(name)
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        out, cnt = _run(pm, k, n)
        debug_set("knn_nocull", 1)
        out2, cnt2 = _run(pm, k, n)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    _check_against(out, cnt, ref.case(name, k), f"{name} k = {k}")
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(cnt, cnt2)
    # each histogram adds up to 100
    assert np.abs(out.reshape(len(model), 3, 11).sum(axis=2) - 100.0).max() <= 1e-10


# ---- 2. exact cases, bit for bit --------------------------------------------------------------------------------------------------
def _one_bin(out):
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    return (out == want[None, :]).all()


@pytest.mark.parametrize("k", [3, 8])
def test_rows_on_a_line_are_exact(k):
    pts = np.column_stack([np.arange(40, dtype=np.float32) * 1.5 + 3, np.full(40, 2, np.float32), np.full(40, -1, np.float32)])
    out, cnt = _fpfh(pts, np.tile(UP, (40, 1)), k)
    assert _one_bin(out)
    assert (cnt[:, [5, 16, 27]] == k - 1).all() and cnt.sum() == 40 * 3 * (k - 1)


@pytest.mark.parametrize("k", [4, 5, 9])
def test_lattice_in_a_plane_is_exact(k):
    """32 x 32 integer lattice in z = 7 with normals (0, 0, 1): ties at the k-th neighbour everywhere; every row 100 at 5, 16, 27"""
    g = np.arange(32, dtype=np.float32)
    pts = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    out, cnt = _fpfh(pts, np.tile(UP, (1024, 1)), k)
    assert _one_bin(out)
    assert np.array_equal(cnt.astype(np.int64), ref.fpfh(pts, np.tile(UP, (1024, 1)), k)["counts"])


def test_hand_worked_four_points_are_exact():
    """tests/test_fpfh_ref.py works this case by hand; the weighting is additions and divisions of doubles in a fixed order, so the
    plain-double restatement gives the device's bits"""
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1]], np.float32)
    nrm = np.tile(UP, (4, 1))
    out, cnt = _fpfh(pts, nrm, 4)
    counts, pout = ref.plain_double(pts, nrm, 4)
    assert np.array_equal(cnt.astype(np.int64), counts) and list(counts[:, :11].sum(axis=1)) == [2, 3, 3, 2]
    assert np.array_equal(_bits(out), _bits(pout))
    assert out[0, 25] == pytest.approx(200 / 3, abs=ref.OUT_TOL) and out[3, 27] == pytest.approx(1900 / 21, abs=ref.OUT_TOL)


# ---- 3. edges -------------------------------------------------------------------------------------------------------------------
def test_fewer_than_three_rows():
    for M in (0, 1, 2):
        pts = np.arange(3 * M, dtype=np.float32).reshape(M, 3) * 1.5
        out, cnt = _fpfh(pts, np.tile(UP, (M, 1)), 3)
        assert out.shape == (M, 33) and cnt.shape == (M, 33)
        r = ref.fpfh(pts, np.tile(UP, (M, 1)), 3)
        assert np.array_equal(out, np.asarray(r["out"], np.float64)) and np.array_equal(cnt.astype(np.int64), r["counts"])
    assert (_fpfh(np.array([[1, 2, 3]], np.float32), UP[None], 3)[0] == 0).all()


@pytest.mark.parametrize("M", [511, 512, 513, 1025])
def test_tile_boundaries(M):
    model, nrm = ref.family_inputs("volume")
    out, cnt = _fpfh(model[:M], nrm[:M], 8)
    _check_against(out, cnt, ref.fpfh(model[:M], nrm[:M], 8), f"volume[:{M}] k = 8")


def test_coincident_rows_give_zeros():
    out, cnt = _fpfh(np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (5, 1)), np.tile(UP, (5, 1)), 4)
    assert (out == 0).all() and (cnt == 0).all()


def test_non_finite_rows():
    model, nrm = ref.family_inputs("sheet")
    model, nrm = model[:700].copy(), nrm[:700].copy()
    bad = model.copy()
    bad[100, 1] = np.nan
    bad[650, 0] = np.inf
    keep = np.setdiff1d(np.arange(700), [100, 650])
    for k in (6, 17):
        out, cnt = _fpfh(bad, nrm, k)
        assert np.isnan(out[[100, 650]]).all() and (cnt[[100, 650]] == 0).all()
        out0, cnt0 = _fpfh(model[keep], nrm[keep], k)
        assert np.array_equal(_bits(out[keep]), _bits(out0)) and np.array_equal(cnt[keep], cnt0)
        assert not np.isnan(out0).any()


def test_a_nan_normal_counts_nowhere_but_its_row_is_described():
    model, nrm = ref.family_inputs("sheet")
    model, nrm = model[:300].copy(), nrm[:300].copy()
    nrm[11, 2] = np.nan
    nrm[40, 0] = np.inf
    out, cnt = _fpfh(model, nrm, 8)
    r = ref.fpfh(model, nrm, 8)
    _check_against(out, cnt, r, "sheet[:300] with a NaN and an inf normal, k = 8")
    assert (cnt[[11, 40]] == 0).all() and not np.isnan(out).any()
    assert np.abs(out[[11, 40]].reshape(2, 3, 11).sum(axis=2) - 100.0).max() <= 1e-10
    idx, _d2, nb = ref.neighbours(model, 8)
    near = (nb & ((idx == 11) | (idx == 40))).any(axis=1)
    near[[11, 40]] = False
    assert near.any() and (cnt[near, :11].sum(axis=1) < 7).all()


def test_padding_and_no_counts():
    """ldn > M reads the rows only; without the SPFH output the descriptors are the same; ldf > M on the host tier leaves the padding"""
    import pcreg_amd as pc
    from pcreg_amd._lib import check, lib
    model, nrm = ref.family_inputs("volume")
    model, nrm = model[:300], nrm[:300]
    M, pad = 300, 7
    pm, _t = _prepared(model)
    try:
        want, cnt = _run(pm, 9, _soa(nrm))
        only = _run(pm, 9, _soa(nrm), spfh=False)[0]
        assert np.array_equal(_bits(only), _bits(want))
        big = torch.full((3, M + pad), float("nan"), dtype=torch.float32, device=_dev())
        big[:, :M] = _soa(nrm)
        got = _run(pm, 9, big[:, :M])[0]
        assert np.array_equal(_bits(got), _bits(want))
        # ldn < M is refused
        L = lib()
        need = int(L.pcreg_dev_model_fpfh_workspace(M, 9))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
        o = torch.empty((M, 33), dtype=torch.float64, device=_dev())
        assert L.pcreg_dev_model_fpfh_f32(pm.handle, 9, _p(big), M - 1, _p(o), None, _p(ws), ws.numel(), None) == 1
        check(L.pcreg_dev_model_fpfh_f32(pm.handle, 9, _p(big), M + pad, _p(o), None, _p(ws), ws.numel(), None))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want))
    finally:
        pm.close()
    # the host tier: ldn > M and ldf > M
    hn = np.full((M + pad, 3), np.nan, np.float32, order="F")
    hn[:M] = nrm
    ho = np.full((M + pad + 2, 33), -7.0, np.float64, order="F")
    hc = np.zeros((M, 33), np.uint8)
    with pc.Model(model) as h:
        check(lib().pcreg_model_fpfh_f32(h._h, 9, hn.ctypes.data, M + pad, 0, None, ho.ctypes.data, M + pad + 2, hc.ctypes.data))
    assert np.array_equal(_bits(ho[:M]), _bits(want)) and (ho[M:] == -7.0).all() and np.array_equal(hc, cnt)


def test_workspace_size_is_exact():
    """one byte short is refused; a canary behind the reported size survives"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    model, nrm = ref.family_inputs("sheet")
    M = len(model)
    pm, _t = _prepared(model)
    try:
        need = int(L.pcreg_dev_model_fpfh_workspace(M, 16))
        n = _soa(nrm)
        o = torch.empty((M, 33), dtype=torch.float64, device=_dev())
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        assert L.pcreg_dev_model_fpfh_f32(pm.handle, 16, _p(n), M, _p(o), None, _p(ws), C.c_size_t(need - 1), None) == _l.PCREG_E_ARG
        _l.check(L.pcreg_dev_model_fpfh_f32(pm.handle, 16, _p(n), M, _p(o), None, _p(ws), C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(_run(pm, 16, n)[0]))
    finally:
        pm.close()


# ---- 4. culling soundness ---------------------------------------------------------------------------------------------------------
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
    nrm = rng.normal(0, 1, (605, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    r = ref.fpfh(model, nrm, 8)
    assert not r["excluded"][small_rows].any() and 1.0 - (~r["excluded"]).mean() <= ref.EXCLUDED_CAP
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        out, cnt = _run(pm, 8, n)
        debug_set("knn_nocull", 1)
        out2, cnt2 = _run(pm, 8, n)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    _check_against(out, cnt, r, "two clusters k = 8")
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(cnt, cnt2)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def test_determinism_on_the_large_sheet(debug_set):
    import normals_ref
    from pcreg_amd._lib import lib
    model = normals_ref.family("sheet", 65536)
    k = 16
    pm, _t = _prepared(model)
    try:
        nrm = pm.normals(ref.K_NORMALS, viewpoint=ref.VIEWPOINT)
        debug_set("knn_stats", 1)
        _stats()
        a = _run(pm, k, nrm)
        searches, visited, nominal, _tail = _stats()
        n_tiles = (len(model) + 511) // 512
        print(f"sheet M = 65536 k = 16: {visited} of {nominal} tile visits ({100.0 * visited / nominal:.2f} %)")
        assert searches == 1 and nominal == n_tiles * n_tiles and 0 < visited < nominal
        debug_set("knn_stats", 0)
        b = _run(pm, k, nrm)
        debug_set("knn_nocull", 1)
        c = _run(pm, k, nrm)
        debug_set("knn_nocull", 0)
        for other in (b, c):
            assert np.array_equal(_bits(a[0]), _bits(other[0])) and np.array_equal(a[1], other[1])
        assert not np.isnan(a[0]).any() and (a[1][:, :11].sum(axis=1) == k - 1).all()
        # two streams sharing the handle, buffers of their own
        M = pm.M
        need = max(int(lib().pcreg_dev_model_fpfh_workspace(M, k)), 256)
        outs = [(torch.full((M, 33), -7.0, dtype=torch.float64, device=_dev()), torch.full((M, 33), 77, dtype=torch.uint8, device=_dev()),
                 torch.empty(need, dtype=torch.uint8, device=_dev())) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.fpfh(k, nrm, spfh=True, out=o)
        torch.cuda.synchronize()
        for o in outs:
            assert np.array_equal(_bits(o[0].cpu().numpy()), _bits(a[0])) and np.array_equal(o[1].cpu().numpy(), a[1])
    finally:
        pm.close()


# ---- 6. tiers --------------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    model, nrm = ref.family_inputs("volume")
    want, wcnt = _fpfh(model, nrm, 9)
    with pc.Model(model) as h:
        a = h.fpfh(9, normals=nrm, spfh=True)
        only = h.fpfh(9, normals=nrm)
    b = pc.point_fpfh(model, 9, normals=nrm, spfh=True)
    for out, cnt in (a, b):
        assert out.dtype == np.float64 and cnt.dtype == np.uint8 and out.shape == cnt.shape == (len(model), 33)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, wcnt)
    assert np.array_equal(_bits(only), _bits(want))
    assert pc.point_fpfh(np.zeros((0, 3)), 3).shape == (0, 33)
    with pytest.raises(ValueError):
        pc.point_fpfh(model, 2)
    with pytest.raises(ValueError):
        pc.point_fpfh(model, 33)


def test_normals_in_the_call_equal_normals_then_fpfh():
    import pcreg_amd as pc
    model, _nrm = ref.family_inputs("sheet")
    vp = ref.VIEWPOINT
    with pc.Model(model) as h:
        for kn, viewpoint in ((9, vp), (6, None)):
            nrm = h.normals(kn, viewpoint=viewpoint)
            want = h.fpfh(16, normals=nrm, spfh=True)
            got = h.fpfh(16, k_normals=kn, viewpoint=viewpoint, spfh=True)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
            pt = pc.point_fpfh(model, 16, k_normals=kn, viewpoint=viewpoint, spfh=True)
            assert np.array_equal(_bits(pt[0]), _bits(want[0])) and np.array_equal(pt[1], want[1])
        nrm = h.normals(16, viewpoint=vp)                      # k_normals defaults to k
        assert np.array_equal(_bits(h.fpfh(16, viewpoint=vp)), _bits(h.fpfh(16, normals=nrm)))
    # the device tier on the library's normals
    pm, _t = _prepared(model)
    try:
        out = _run(pm, 16, pm.normals(9, viewpoint=vp))[0]
    finally:
        pm.close()
    with pc.Model(model) as h:
        assert np.array_equal(_bits(out), _bits(h.fpfh(16, k_normals=9, viewpoint=vp)))


# ---- 7. the chain: normals -> fpfh -> getMatches -> ransac ------------------------------------------------------------------------------
def _chain_scene():
    rng = np.random.default_rng(5)
    u = rng.uniform(0, 40, (2048, 2))
    z = (3 * np.sin(u[:, 0] / 5) * np.cos(u[:, 1] / 7) + 0.004 * u[:, 0] * u[:, 1]
         + 2.0 * np.exp(-((u[:, 0] - 12) ** 2 + (u[:, 1] - 27) ** 2) / 30))          # no symmetry: a saddle term and one bump
    a = (np.column_stack([u, z]) + np.array([100.0, 50.0, 90.0])).astype(np.float32)
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K                       # 0.7 rad about a skew axis
    t = np.array([7.0, -3.0, 11.0])
    b = (a.astype(np.float64) @ R.T + t).astype(np.float32)
    return a, b, R, t


def test_registration_chain_recovers_the_motion():
    """A cloud of 2048 rows on a height field without symmetry and its copy under a rotation of 0.7 rad about (0.3, -0.5, 0.8) and
    a translation, rounded to fp32.  Normals from the library at k = 9 with the viewpoint moved along, fpfh at k = 16, getMatches
    at D = 33 (SSD, MatchThreshold 100, MaxRatio 0.9, Unique), ransac on the matched coordinates: every point of the copy must
    come back to within half the cloud's median nearest-neighbour distance (0.216) of its original.
    The reference chain (fpfh_ref on normals_ref's normals, the oracle's getMatches and ransac) keeps 1370 pairs, all of them
    correct, and brings every point to within 9.0e-6: a margin of 2.4e4 under the condition."""
    import pcreg_amd as pc
    a, b, R, t = _chain_scene()
    vp_a = np.array(ref.VIEWPOINT)
    vp_b = R @ vp_a + t
    desc = []
    for cloud, vp in ((a, vp_a), (b, vp_b)):
        with pc.Model(cloud) as h:
            desc.append(h.fpfh(16, k_normals=9, viewpoint=vp))
    par = dict(UNNORMALIZE=False, CHANGE_METRIC=False, Method="Exhaustive", MatchThreshold=100.0, MaxRatio=0.9, Metric="SSD", Unique=True)
    pairs = pc.getMatches(desc[1], desc[0], par)               # surface: the copy; model: the original
    assert len(pairs) >= 500
    p1 = b[pairs[:, 0] - 1].astype(np.float64)
    p2 = a[pairs[:, 1] - 1].astype(np.float64)
    coef = dict(minPtNum=3, iterNum=2000, thDist=0.05, thInlrRatio=0.1, REFINE=True, VERBOSE=0)
    T, inl, _ns, mi, _ratio = pc.ransac(p1, p2, coef, pc.estimateTransform, pc.calcDists, seed=7)
    assert T.shape == (4, 4) and mi >= 500
    back = (np.hstack([b.astype(np.float64), np.ones((len(b), 1))]) @ np.linalg.inv(T))[:, :3]      # [original, 1] T = [copy, 1]
    err = np.linalg.norm(back - a.astype(np.float64), axis=1)
    _idx, d2 = knn_k_ref.knn(a, a, 2)
    half = float(np.median(np.sqrt(d2[:, 1].astype(np.float64)))) / 2
    print(f"chain: {len(pairs)} pairs ({(pairs[:, 0] == pairs[:, 1]).mean():.3f} correct), {mi} inliers, worst distance {err.max():.3e}, "
          f"half the median nearest-neighbour distance {half:.4f}")
    assert (err <= half).all()
