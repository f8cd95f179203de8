"""FPFH descriptors from radius neighbourhoods (knn_fpfh_radius.hip) on the GPU against tests/fpfh_radius_ref.py.

On the compared rows (tests/test_fpfh_radius_ref.py holds the excluded share of every family case under 1 %) the SPFH counts, m and
n_neighbors must be EQUAL and the output must satisfy |x - x_ref| <= OUT_TOL(n) = 2 (n_max + 8) eps64 * 100, n_max the case's longest
counted neighbourhood (the derivation is at fpfh_radius_ref.out_tol).  Then the equivalence to the k-nearest kernel bit for bit,
max_neighbors, the tile boundaries, the edge rows, the degenerate sizes, a truncated capacity between sentinels, determinism, the
workspace size, the tiers and a registration chain."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpfh_radius_ref as ref
import fpfh_ref
import knn_k_ref

pytestmark = pytest.mark.gpu
UP = np.array([0.0, 0.0, 1.0], np.float32)
INF = np.float32(np.inf)


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


def _run(pm, r2, nrm_soa, max_neighbors=0):
    """count, ONE read of the total, the second call -> out [M, 33] float64, counts [M, 33] int64, n_neighbors [M] int32, total"""
    _counts, seg = pm.fpfh_radius_count(r2)
    total = int(seg[-1].item())
    out, cnt, nn = pm.fpfh_radius(r2, nrm_soa, seg, total, max_neighbors=max_neighbors, spfh=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), nn.cpu().numpy(), total


def _fpfh(model, normals, r2, max_neighbors=0):
    pm, _t = _prepared(model)
    try:
        return _run(pm, r2, _soa(normals), max_neighbors)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_against(got, r, what=""):
    """counts, m, n_neighbors and output against the reference dict r on the compared rows; -> the worst |x - x_ref| / bound"""
    out, cnt, nn, _total = got
    cmp = ~r["excluded"]
    share = 1.0 - cmp.mean() if len(cmp) else 0.0
    n_max = int(r["n"].max(initial=0))
    tol = ref.out_tol(n_max)
    want = np.asarray(r["out"], np.float64)
    fin = cmp & ~np.isnan(want).any(axis=1)
    err = np.abs(out[fin] - want[fin])
    worst = float(err.max() / tol) if err.size else 0.0
    print(f"{what}: n_max {n_max}, largest count {int(cnt.max(initial=0))}, worst |x - x_ref| {float(err.max()) if err.size else 0.0:.3e}, "
          f"worst / bound {worst:.4f}, excluded {100 * share:.2f} %")
    assert share <= ref.EXCLUDED_CAP, what
    assert np.array_equal(np.isnan(out), np.isnan(want)), what
    assert np.array_equal(cnt[cmp], r["counts"][cmp]), what
    assert np.array_equal(cnt[cmp, :11].sum(axis=1), r["m"][cmp]), what
    assert np.array_equal(nn[cmp].astype(np.int64), r["n"][cmp]), what
    assert (err <= tol).all(), (what, worst)
    return worst


# ---- 1. families ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_neighbors", ref.MAX_NEIGHBORS)
@pytest.mark.parametrize("name,radius", ref.CASES)
def test_families_against_the_reference(name, radius, max_neighbors, debug_set):
    model, nrm = fpfh_ref.family_inputs(name)
    r2 = ref.r2_of(radius)
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        got = _run(pm, r2, n, max_neighbors)
        debug_set("knn_nocull", 1)
        got2 = _run(pm, r2, n, max_neighbors)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    r = ref.case(name, radius, max_neighbors)
    _check_against(got, r, f"{name} radius {radius:g} max_neighbors {max_neighbors}")
    assert np.array_equal(_bits(got[0]), _bits(got2[0])) and np.array_equal(got[1], got2[1]) and np.array_equal(got[2], got2[2])
    assert np.array_equal(got[2].astype(np.int64), r["n"])                 # the window's length depends on the lists alone: every row
    assert np.abs(got[0].reshape(len(model), 3, 11).sum(axis=2) - 100.0).max() <= 1e-10


# ---- 2. the k-nearest kernel, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 9, 32])
def test_equals_the_k_nearest_kernel_where_the_rules_coincide(k):
    """M = 300 without coincident rows, a radius that covers the cloud (+inf and a finite one), max_neighbors = k - 1"""
    model, nrm = fpfh_ref.family_inputs("volume")
    model, nrm = model[:300], nrm[:300]
    assert len(np.unique(model, axis=0)) == 300
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        want, wcnt = pm.fpfh(k, n, spfh=True)
        torch.cuda.synchronize()
        want, wcnt = want.cpu().numpy(), wcnt.cpu().numpy().astype(np.int64)
        for r2 in (INF, ref.r2_of(40.0)):
            out, cnt, nn, total = _run(pm, r2, n, k - 1)
            assert total == 300 * 300 and (nn == k - 1).all()
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, wcnt)
    finally:
        pm.close()


# ---- 3. max_neighbors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 31])
def test_max_neighbors_counts_the_first_n_positive_entries(n):
    """sheet at radius 4 (14 .. 79 rows inside): the window is the first n entries at a distance > 0; a row with fewer uses them all"""
    model, nrm = fpfh_ref.family_inputs("sheet")
    r2 = ref.r2_of(4.0)
    got = _fpfh(model, nrm, r2, n)
    r = ref.fpfh(model, nrm, r2, n)
    full = ref.case("sheet", 4.0, 0)["n"]
    assert np.array_equal(r["n"], np.minimum(full, n)) and (n < 31 or (full < n).any())
    _check_against(got, r, f"sheet radius 4 max_neighbors {n}")
    assert np.array_equal(got[2].astype(np.int64), np.minimum(full, n))


# ---- 4. tile boundaries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [511, 512, 513, 1025])
def test_tile_boundaries(M):
    model, nrm = fpfh_ref.family_inputs("volume")
    r2 = ref.r2_of(7.0)
    got = _fpfh(model[:M], nrm[:M], r2)
    _check_against(got, ref.fpfh(model[:M], nrm[:M], r2), f"volume[:{M}] radius 7")


# ---- 5. edge rows -----------------------------------------------------------------------------------------------------------------
def test_coincident_rows_are_skipped_and_not_counted_against_n():
    """rows 0 .. 39 of the sheet appear twice more each: the zeros lead every such segment, and max_neighbors = 5 still counts five
    rows at a distance > 0; a cloud of coincident rows alone gives zeros"""
    model, nrm = fpfh_ref.family_inputs("sheet")
    model = np.vstack([model[:400], model[:40], model[:40]])
    nrm = np.vstack([nrm[:400], nrm[:40], nrm[:40]])
    r2 = ref.r2_of(6.0)
    for n in (0, 5):
        r = ref.fpfh(model, nrm, r2, n)
        got = _fpfh(model, nrm, r2, n)
        _check_against(got, r, f"sheet[:400] with 80 coincident rows, max_neighbors {n}")
        assert np.array_equal(got[2].astype(np.int64), r["n"]) and (n == 0 or (got[2][:40] == 5).all())
        assert np.array_equal(_bits(got[0][:40]), _bits(got[0][400:440])) and np.array_equal(got[1][:40], got[1][440:])
    out, cnt, nn, total = _fpfh(np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (5, 1)), np.tile(UP, (5, 1)), 9.0)
    assert total == 25 and (out == 0).all() and (cnt == 0).all() and (nn == 0).all()


@pytest.mark.parametrize("r2", [ref.r2_of(5.0), INF])
def test_non_finite_rows(r2):
    model, nrm = fpfh_ref.family_inputs("sheet")
    model, nrm = model[:700].copy(), nrm[:700].copy()
    bad = model.copy()
    bad[100, 1] = np.nan
    bad[650, 0] = np.inf
    bad[651, 2] = -np.inf
    rows = [100, 650, 651]
    keep = np.setdiff1d(np.arange(700), rows)
    out, cnt, nn, _total = _fpfh(bad, nrm, r2, 40)
    assert np.isnan(out[rows]).all() and (cnt[rows] == 0).all() and (nn[rows] == 0).all()
    out0, cnt0, nn0, _t0 = _fpfh(model[keep], nrm[keep], r2, 40)
    assert np.array_equal(_bits(out[keep]), _bits(out0)) and np.array_equal(cnt[keep], cnt0) and np.array_equal(nn[keep], nn0)
    assert not np.isnan(out0).any()


def test_a_nan_normal_counts_nowhere_but_its_row_is_described():
    model, nrm = fpfh_ref.family_inputs("sheet")
    model, nrm = model[:300].copy(), nrm[:300].copy()
    nrm[11, 2] = np.nan
    nrm[40, 0] = np.inf
    r2 = ref.r2_of(6.0)
    got = _fpfh(model, nrm, r2)
    r = ref.fpfh(model, nrm, r2)
    _check_against(got, r, "sheet[:300] with a NaN and an inf normal, radius 6")
    out, cnt, nn, _total = got
    assert (cnt[[11, 40]] == 0).all() and (nn[[11, 40]] > 0).all() and not np.isnan(out).any()
    assert np.abs(out[[11, 40]].reshape(2, 3, 11).sum(axis=2) - 100.0).max() <= 1e-10
    near = (r["nb"] & ((r["idx"] == 11) | (r["idx"] == 40))).any(axis=1)
    near[[11, 40]] = False
    assert near.any() and (cnt[near, :11].sum(axis=1) < nn[near]).all()


# ---- 6. degenerate sizes ----------------------------------------------------------------------------------------------------------
def test_fewer_than_three_rows_and_a_radius_of_zero():
    for M in (0, 1, 2):
        pts = np.arange(3 * M, dtype=np.float32).reshape(M, 3) * 1.5
        out, cnt, nn, total = _fpfh(pts, np.tile(UP, (M, 1)), 100.0)
        assert out.shape == (M, 33) and cnt.shape == (M, 33) and nn.shape == (M,) and total == M * M
        r = ref.fpfh(pts, np.tile(UP, (M, 1)), 100.0)
        assert np.array_equal(out, np.asarray(r["out"], np.float64)) and np.array_equal(cnt, r["counts"]) and np.array_equal(nn, r["n"])
    model, nrm = fpfh_ref.family_inputs("volume")
    out, cnt, nn, total = _fpfh(model[:600], nrm[:600], 0.0)
    assert total == 600 and (out == 0).all() and (cnt == 0).all() and (nn == 0).all()


# ---- 7. a truncated capacity ------------------------------------------------------------------------------------------------------
def test_truncated_capacity_writes_nothing_outside_its_buffers():
    """capacity = half the total: whole segments and one partial one are cut off.  The outputs and the workspace sit between
    sentinels that must survive; the rows whose segments and whose neighbours' segments are whole keep their values; no claim is made
    on the others."""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    model, nrm = fpfh_ref.family_inputs("sheet")
    order = np.argsort(model[:, 0], kind="stable")                       # rows in x order: a row's neighbours have nearby row numbers
    model, nrm = model[order], nrm[order]
    M, pad, r2 = len(model), 256, float(ref.r2_of(4.0))
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        want = _run(pm, r2, n)
        _counts, seg = pm.fpfh_radius_count(r2)
        total = int(seg[-1].item())
        cap = total // 2
        assert 0 < cap < total
        need = int(L.pcreg_dev_model_fpfh_radius_workspace(M, cap))
        assert need < int(L.pcreg_dev_model_fpfh_radius_workspace(M, total))
        big_o = torch.full((M * 33 + 2 * pad,), -7.0, dtype=torch.float64, device=_dev())
        big_c = torch.full((M * 33 + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        big_n = torch.full((M + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        big_w = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=_dev())
        o, c = big_o[pad:pad + M * 33].view(M, 33), big_c[pad:pad + M * 33].view(M, 33)
        nn, ws = big_n[pad:pad + M], big_w[pad:pad + need]
        pm.fpfh_radius(r2, n, seg, cap, spfh=True, out=(o, c, nn, ws))
        torch.cuda.synchronize()
        for big, fill in ((big_o, -7.0), (big_c, 0x5A5A5A5A), (big_n, 0x5A5A5A5A), (big_w, 0xA5)):
            assert (big[:pad] == fill).all().item() and (big[-pad:] == fill).all().item()
        so = seg.cpu().numpy()
        whole = so[1:] <= cap                                             # the row's own segment fits
        idx, _d2, nb, _n = ref.lists(model, r2)
        ok = whole & ~(nb & ~whole[idx]).any(axis=1)                      # ... and so does every neighbour's
        assert 0 < ok.sum() < whole.sum() < M
        assert np.array_equal(c.cpu().numpy()[whole].astype(np.int64), want[1][whole]) and np.array_equal(nn.cpu().numpy()[whole], want[2][whole])
        assert np.array_equal(_bits(o.cpu().numpy()[ok]), _bits(want[0][ok]))
    finally:
        pm.close()


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------
def test_determinism_on_the_large_sheet(debug_set):
    """20 000 rows at about 50 neighbours: a second call, a call without culling and the two other lane counts (4, 16) of the counting
    kernel give every bit of the first; two streams sharing the handle, buffers of their own"""
    import normals_ref
    from pcreg_amd._lib import lib
    model = normals_ref.family("sheet", 20000)
    r2 = float(ref.r2_of(1.13))
    pm, _t = _prepared(model)
    try:
        nrm = pm.normals(fpfh_ref.K_NORMALS, viewpoint=fpfh_ref.VIEWPOINT)
        a = _run(pm, r2, nrm)
        print(f"sheet M = 20000 radius 1.13: {a[3]} list entries, neighbourhoods {a[2].min()}-{a[2].max()}, mean {a[2].mean():.1f}")
        assert 30 <= a[2].mean() <= 70 and not np.isnan(a[0]).any()
        others = [_run(pm, r2, nrm)]
        for key, val in (("knn_nocull", 1), ("fpfh_radius_lanes", 4), ("fpfh_radius_lanes", 16)):
            debug_set(key, val)
            others.append(_run(pm, r2, nrm))
            debug_set(key, 0)
        for b in others:
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
        M = pm.M
        _counts, seg = pm.fpfh_radius_count(r2)
        need = max(int(lib().pcreg_dev_model_fpfh_radius_workspace(M, a[3])), 256)
        outs = [(torch.full((M, 33), -7.0, dtype=torch.float64, device=_dev()), torch.full((M, 33), 77, dtype=torch.int32, device=_dev()),
                 torch.full((M,), -3, dtype=torch.int32, device=_dev()), torch.empty(need, dtype=torch.uint8, device=_dev())) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.fpfh_radius(r2, nrm, seg, a[3], spfh=True, out=o)
        torch.cuda.synchronize()
        for o in outs:
            assert np.array_equal(_bits(o[0].cpu().numpy()), _bits(a[0])) and np.array_equal(o[1].cpu().numpy().astype(np.int64), a[1])
            assert np.array_equal(o[2].cpu().numpy(), a[2])
    finally:
        pm.close()


# ---- 9. the workspace and the device tier's refusals --------------------------------------------------------------------------------
def test_workspace_size_is_exact_and_the_device_tier_refuses_bad_arguments():
    """one byte short is refused; a canary behind the reported size survives; r2, max_neighbors, capacity and ldn are checked"""
    from pcreg_amd import _lib as _l
    L = _l.lib()
    model, nrm = fpfh_ref.family_inputs("volume")
    M, r2 = len(model), float(ref.r2_of(4.0))
    pm, _t = _prepared(model)
    try:
        n = _soa(nrm)
        want = _run(pm, r2, n)
        total = want[3]
        need0 = int(L.pcreg_dev_model_fpfh_radius_workspace(M, 0))
        need = int(L.pcreg_dev_model_fpfh_radius_workspace(M, total))
        counts = torch.empty(M, dtype=torch.int32, device=_dev())
        seg = torch.empty(M + 1, dtype=torch.int64, device=_dev())
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        o = torch.empty((M, 33), dtype=torch.float64, device=_dev())
        E = _l.PCREG_E_ARG
        count = lambda r2_, nbytes: L.pcreg_dev_model_fpfh_radius_count_f32(pm.handle, r2_, _p(counts), _p(seg), _p(ws), C.c_size_t(nbytes), None)
        call = lambda r2_, nmax, ldn, cap, nbytes: L.pcreg_dev_model_fpfh_radius_f32(pm.handle, r2_, nmax, _p(n), ldn, _p(seg), cap, _p(o), None, None,
                                                                                      _p(ws), C.c_size_t(nbytes), None)
        assert count(r2, need0 - 1) == E and count(float("nan"), need0) == E and count(-1.0, need0) == E
        _l.check(count(r2, need0))
        torch.cuda.synchronize()
        assert int(seg[-1].item()) == total and (ws[need0:] == 0xA5).all().item()
        assert call(r2, 0, M, total, need - 1) == E
        assert call(float("nan"), 0, M, total, need) == E and call(r2, -1, M, total, need) == E
        assert call(r2, 0, M - 1, total, need) == E and call(r2, 0, M, -1, need) == E
        _l.check(call(r2, 0, M, total, need))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want[0]))
    finally:
        pm.close()


# ---- 10. tiers --------------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    model, nrm = fpfh_ref.family_inputs("volume")
    for radius, n in ((4.0, 0), (6.0, 50)):
        want, wcnt, wnn, _total = _fpfh(model, nrm, ref.r2_of(radius), n)
        with pc.Model(model) as h:
            a = h.fpfh_radius(radius, normals=nrm, max_neighbors=n, counts=True, n_neighbors=True)
            only = h.fpfh_radius(radius, normals=nrm, max_neighbors=n)
            just_nn = h.fpfh_radius(radius, normals=nrm, max_neighbors=n, n_neighbors=True)
        b = pc.point_fpfh_radius(model, radius, normals=nrm, max_neighbors=n, counts=True, n_neighbors=True)
        for out, cnt, nn in (a, b):
            assert out.dtype == np.float64 and cnt.dtype == np.uint32 and nn.dtype == np.int32
            assert out.shape == cnt.shape == (len(model), 33) and nn.shape == (len(model),)
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt.astype(np.int64), wcnt) and np.array_equal(nn, wnn)
        assert np.array_equal(_bits(only), _bits(want)) and np.array_equal(_bits(just_nn[0]), _bits(want)) and np.array_equal(just_nn[1], wnn)
    assert pc.point_fpfh_radius(np.zeros((0, 3)), 1.0).shape == (0, 33)
    # ldn > M and ldf > M on the host tier leave the padding
    from pcreg_amd._lib import check, lib
    M, pad = 300, 7
    want, wcnt, wnn, _total = _fpfh(model[:M], nrm[:M], ref.r2_of(7.0), 50)
    hn = np.full((M + pad, 3), np.nan, np.float32, order="F")
    hn[:M] = nrm[:M]
    ho = np.full((M + pad + 2, 33), -7.0, np.float64, order="F")
    hc = np.zeros((M, 33), np.uint32)
    with pc.Model(model[:M]) as h:
        check(lib().pcreg_model_fpfh_radius_f32(h._h, float(ref.r2_of(7.0)), 50, hn.ctypes.data, M + pad, 0, None, ho.ctypes.data, M + pad + 2,
                                                hc.ctypes.data, None))
    assert np.array_equal(_bits(ho[:M]), _bits(want)) and (ho[M:] == -7.0).all() and np.array_equal(hc.astype(np.int64), wcnt)


def test_normals_in_the_call_equal_normals_then_the_call():
    import pcreg_amd as pc
    model, _nrm = fpfh_ref.family_inputs("sheet")
    vp = fpfh_ref.VIEWPOINT
    with pc.Model(model) as h:
        for kn, viewpoint in ((9, vp), (6, None)):
            nrm = h.normals(kn, viewpoint=viewpoint)
            want = h.fpfh_radius(4.0, normals=nrm, max_neighbors=50, counts=True)
            got = h.fpfh_radius(4.0, max_neighbors=50, k_normals=kn, viewpoint=viewpoint, counts=True)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
            pt = pc.point_fpfh_radius(model, 4.0, max_neighbors=50, k_normals=kn, viewpoint=viewpoint, counts=True)
            assert np.array_equal(_bits(pt[0]), _bits(want[0])) and np.array_equal(pt[1], want[1])
    pm, _t = _prepared(model)
    try:
        out = _run(pm, float(ref.r2_of(4.0)), pm.normals(9, viewpoint=vp), 50)[0]
    finally:
        pm.close()
    with pc.Model(model) as h:
        assert np.array_equal(_bits(out), _bits(h.fpfh_radius(4.0, max_neighbors=50, k_normals=9, viewpoint=vp)))


# ---- 11. the chain: normals -> radius fpfh -> getMatches -> ransac -------------------------------------------------------------------
def _chain_scene():
    """tests/test_gpu_fpfh.py's scene (2048 rows on a height field without symmetry, a rotation of 0.7 rad about a skew axis and a
    translation), the copy with Gaussian noise of sigma 0.002 on every coordinate before it is rounded to fp32"""
    rng = np.random.default_rng(5)
    u = rng.uniform(0, 40, (2048, 2))
    z = (3 * np.sin(u[:, 0] / 5) * np.cos(u[:, 1] / 7) + 0.004 * u[:, 0] * u[:, 1]
         + 2.0 * np.exp(-((u[:, 0] - 12) ** 2 + (u[:, 1] - 27) ** 2) / 30))
    a = (np.column_stack([u, z]) + np.array([100.0, 50.0, 90.0])).astype(np.float32)
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    t = np.array([7.0, -3.0, 11.0])
    b = (a.astype(np.float64) @ R.T + t + rng.normal(0, 0.002, a.shape)).astype(np.float32)
    return a, b, R, t


def test_registration_chain_recovers_the_motion():
    """Normals from the library at k = 9 with the viewpoint moved along, the radius FPFH at radius 4 (about 60 rows inside) on both
    clouds, getMatches at D = 33 (SSD, MatchThreshold 100, MaxRatio 0.9, Unique), ransac on the matched coordinates: every point of
    the copy must come back to within half the cloud's median nearest-neighbour distance of its original, the tolerance of
    tests/test_gpu_fpfh.py's chain."""
    import pcreg_amd as pc
    a, b, R, t = _chain_scene()
    vp_a = np.array(fpfh_ref.VIEWPOINT)
    vp_b = R @ vp_a + t
    desc = []
    for cloud, vp in ((a, vp_a), (b, vp_b)):
        with pc.Model(cloud) as h:
            d, nn = h.fpfh_radius(4.0, k_normals=9, viewpoint=vp, n_neighbors=True)
            assert nn.max() > 50 and not np.isnan(d).any()
            desc.append(d)
    par = dict(UNNORMALIZE=False, CHANGE_METRIC=False, Method="Exhaustive", MatchThreshold=100.0, MaxRatio=0.9, Metric="SSD", Unique=True)
    pairs = pc.getMatches(desc[1], desc[0], par)               # surface: the copy; model: the original
    assert len(pairs) >= 200
    p1 = b[pairs[:, 0] - 1].astype(np.float64)
    p2 = a[pairs[:, 1] - 1].astype(np.float64)
    coef = dict(minPtNum=3, iterNum=2000, thDist=0.05, thInlrRatio=0.1, REFINE=True, VERBOSE=0)
    T, inl, _ns, mi, _ratio = pc.ransac(p1, p2, coef, pc.estimateTransform, pc.calcDists, seed=7)
    assert T.shape == (4, 4) and mi >= 100
    back = (np.hstack([b.astype(np.float64), np.ones((len(b), 1))]) @ np.linalg.inv(T))[:, :3]      # [original, 1] T = [copy, 1]
    err = np.linalg.norm(back - a.astype(np.float64), axis=1)
    _idx, d2 = knn_k_ref.knn(a, a, 2)
    half = float(np.median(np.sqrt(d2[:, 1].astype(np.float64)))) / 2
    print(f"chain: {len(pairs)} pairs ({(pairs[:, 0] == pairs[:, 1]).mean():.3f} correct), {mi} inliers, worst distance {err.max():.3e}, "
          f"half the median nearest-neighbour distance {half:.4f}")
    assert (err <= half).all()
