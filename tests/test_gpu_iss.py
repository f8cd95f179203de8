"""ISS keypoints of a prepared model (knn_iss.hip) on the GPU against tests/iss_ref.py.

n_neighbors: EQUAL on every row.  The candidate flag (saliency > 0) and the keypoint list: EQUAL on every row the reference does
not exclude (tests/test_iss_ref.py holds the excluded share under 1 %; no row of the six family cases is excluded).  The list
restated on the RETURNED saliencies equals the contract's rule bit for bit on every row.
Eigenvalues: |mu - mu_ref| <= 64 eps ||N||_F per eigenvalue, mu = lambda n^2 4^(18 - e) formed in longdouble from the returned lambda
(its two roundings are 2^-52 mu <= ||N||_F / 64 of the bound): Jacobi's backward error is a small multiple of eps ||A||_F, the
constant is the one the normals' variation bound uses.
Then the exact cases bit for bit, the edges, culling soundness, determinism, the tiers and the chain."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iss_ref as ref
import knn_k_ref

pytestmark = pytest.mark.gpu
Lf = np.longdouble
DEF = (0.975, 0.975, 5)


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
    """a PreparedModel.iss_keypoints dict as numpy"""
    torch.cuda.synchronize()
    n = int(res["n_keypoints"].cpu().item())
    return dict(n=res["n_neighbors"].cpu().numpy(), eig=None if res["eig"] is None else res["eig"].cpu().numpy(),
                s=res["saliency"].cpu().numpy(), keypoints=res["keypoints"].cpu().numpy()[:n])


def _run(pm, rs, rn, g21=DEF[0], g32=DEF[1], mn=DEF[2], **kw):
    return _host(pm.iss_keypoints(rs, rn, g21, g32, mn, **kw))


def _iss(model, rs, rn, g21=DEF[0], g32=DEF[1], mn=DEF[2], **kw):
    pm, _t = _prepared(model)
    try:
        return _run(pm, rs, rn, g21, g32, mn, **kw)
    finally:
        pm.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(a, b):
    return (np.array_equal(a["n"], b["n"]) and np.array_equal(_bits(a["eig"]), _bits(b["eig"])) and np.array_equal(_bits(a["s"]), _bits(b["s"]))
            and np.array_equal(a["keypoints"], b["keypoints"]))


@functools.lru_cache(maxsize=None)
def _family(name):
    a = ref.family(name)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(name, rs, rn):
    return ref.case(name, rs, rn)


def _check_list(got, model, rn):
    """the list is the contract's rule on the returned doubles: ascending int32 rows inside the model"""
    kp = got["keypoints"]
    assert kp.dtype == np.int32
    assert np.array_equal(kp, ref.keypoints_of(model, got["s"], ref.r2_of(rn)))
    assert (np.diff(kp) > 0).all() and (len(kp) == 0 or (kp[0] >= 0 and kp[-1] < len(model)))


def _check_against(got, r, model, rn, what=""):
    """-> the worst |mu - mu_ref| / (64 eps ||N||_F)"""
    M = len(model)
    assert got["n"].dtype == np.int32 and np.array_equal(got["n"], r["n"]), what
    dead = r["n"] == 0
    assert np.isnan(got["eig"][dead]).all() and (got["s"][dead] == 0).all() and not np.isnan(got["eig"][~dead]).any(), what
    assert (got["s"] >= 0).all() and not np.signbit(got["s"]).any(), what
    assert (np.diff(got["eig"][~dead], axis=1) <= 0).all(), what                         # descending
    share = 0.0
    if (~dead).any():
        n2 = (r["n"][~dead].astype(Lf) ** 2)[:, None]
        mu = got["eig"][~dead].astype(Lf) * n2 * Lf(4.0) ** Lf(18 - r["e"])
        err = np.abs(mu - r["mu"][~dead])
        bound = (64 * ref.EPS * r["normN"][~dead])[:, None].astype(Lf)
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, Lf(1e-300))).max()))
        pos = bound[:, 0] > 0
        share = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    keep = ~r["excluded"]
    assert np.array_equal((got["s"] > 0)[keep], r["cand"][keep]), what
    cand = got["s"] > 0
    assert (got["s"][cand] == got["eig"][cand, 2]).all(), what                            # the saliency is lambda_3's bits
    key = np.zeros(M, bool)
    key[got["keypoints"]] = True
    assert np.array_equal(key[keep], r["key"][keep]), what
    _check_list(got, model, rn)
    print(f"{what}: worst |mu - mu_ref| / (64 eps ||N||_F) = {share:.4f}, {int(cand.sum())} candidates, {len(got['keypoints'])} keypoints, "
          f"{int(r['excluded'].sum())} rows excluded")
    return share


# ---- 1. families, with and without culling -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rs,rn", ref.cases())
def test_families_against_the_reference(name, rs, rn, debug_set):
    r = _ref(name, rs, rn)
    model = _family(name)
    pm, _t = _prepared(model)
    try:
        a = _run(pm, rs, rn)
        debug_set("knn_nocull", 1)
        b = _run(pm, rs, rn)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    share = _check_against(a, r, model, rn, f"{name} r = ({rs}, {rn})")
    assert share < 1.0 and _same(a, b)
    assert len(a["keypoints"]) >= 10


# ---- 2. exact cases, bit for bit ------------------------------------------------------------------------------------------
def test_hand_worked_eight_points_are_exact():
    """tests/test_iss_ref.py's case: N is diagonal, so the Jacobi does not turn and the eigenvalues are exact quotients"""
    pts = ref.hand_case()
    got = _iss(pts, 2.0, 3.0)
    assert list(got["n"]) == [7, 6, 6, 7, 7, 7, 7, 1]
    want = np.array([[31.5, 14, 3.5]] * 8) / 49
    want[[1, 2]] = np.array([12, 11.25, 3]) / 36
    want[7] = 0.0
    assert np.array_equal(_bits(got["eig"]), _bits(want))
    s = want[:, 2].copy()
    assert np.array_equal(_bits(got["s"]), _bits(s)) and list(got["keypoints"]) == [1]
    assert list(_iss(pts, 2.0, 0.1)["keypoints"]) == [0, 1, 2, 3, 4, 5, 6]
    g7 = _iss(pts, 2.0, 3.0, mn=7)
    assert list(g7["keypoints"]) == [0] and list(g7["s"] > 0) == [True, False, False, True, True, True, True, False]
    assert np.array_equal(_bits(g7["eig"]), _bits(want))
    assert len(_iss(pts, 2.0, 3.0, mn=8)["keypoints"]) == 0
    _check_against(got, ref.iss(pts, 4.0, 9.0), pts, 3.0, "hand-worked")


def test_plane_and_line_have_exact_zeros_and_no_keypoint():
    for pts in (ref.lattice_plane(),
                np.column_stack([np.arange(40, dtype=np.float32) * 0.5 + 3, np.full(40, 5, np.float32), np.full(40, -2, np.float32)])):
        got = _iss(pts, 3.0, 2.0)
        assert (got["eig"][:, 2] == 0).all() and (got["eig"][:, 0] > 0).all()
        assert not got["s"].any() and len(got["keypoints"]) == 0
        _check_against(got, ref.iss(pts, ref.r2_of(3.0), ref.r2_of(2.0)), pts, 2.0, f"flat cloud of {len(pts)} rows")


def test_cube_lattice_ties_go_to_the_lowest_row():
    pts, interior = ref.lattice_cube()
    got = _iss(pts, 1.0, 1.0, 2.0, 2.0, 7)
    r = ref.iss(pts, 1.0, 1.0, 2.0, 2.0, 7)
    assert np.array_equal(got["s"] > 0, interior)
    assert np.array_equal(_bits(got["eig"][interior]), _bits(np.full((343, 3), 2.0 / 7.0)))
    assert np.array_equal(got["keypoints"], r["keypoints"]) and 20 < len(got["keypoints"]) < 343
    _check_against(got, r, pts, 1.0, "cube lattice")


# ---- 3. edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 2, 511, 512, 513, 1025])
def test_few_rows_and_tile_boundaries(M):
    model = np.vstack([_family("volume"), _family("sheet")])[:M]
    got = _iss(model, 3.0, 2.0)
    assert got["n"].shape == (M,) and got["eig"].shape == (M, 3) and got["s"].shape == (M,)
    _check_against(got, ref.iss(model, ref.r2_of(3.0), ref.r2_of(2.0)), model, 2.0, f"M = {M}")
    if M <= 2:
        assert len(got["keypoints"]) == 0


def test_coincident_rows_across_a_tile_boundary():
    got = _iss(np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (600, 1)), 1.0, 1.0, mn=1)
    assert (got["n"] == 600).all() and np.array_equal(_bits(got["eig"]), _bits(np.zeros((600, 3))))
    assert np.array_equal(_bits(got["s"]), _bits(np.zeros(600))) and len(got["keypoints"]) == 0


def test_non_finite_rows():
    model = _family("sheet")[:700].copy()
    bad = model.copy()
    bad[100, 1] = np.nan
    bad[650, 0] = np.inf
    keep = np.setdiff1d(np.arange(700), [100, 650])
    got = _iss(bad, 3.0, 2.0)
    clean = _iss(model[keep], 3.0, 2.0)
    assert (got["n"][[100, 650]] == 0).all() and np.isnan(got["eig"][[100, 650]]).all() and (got["s"][[100, 650]] == 0).all()
    assert np.array_equal(got["n"][keep], clean["n"]) and np.array_equal(_bits(got["eig"][keep]), _bits(clean["eig"]))
    assert np.array_equal(_bits(got["s"][keep]), _bits(clean["s"]))
    assert np.array_equal(got["keypoints"], keep[clean["keypoints"]]) and len(clean["keypoints"]) > 0
    _check_against(got, ref.iss(bad, ref.r2_of(3.0), ref.r2_of(2.0)), bad, 2.0, "non-finite rows")


def test_parameter_edges():
    """min_neighbors above every n: no keypoint; a tiny nonmax radius: every candidate is one; eig omitted: the rest keeps its bits"""
    model = _family("volume")
    pm, _t = _prepared(model)
    try:
        want = _run(pm, 3.0, 2.0)
        none = _run(pm, 3.0, 2.0, mn=int(want["n"].max()) + 1)
        assert not none["s"].any() and len(none["keypoints"]) == 0 and np.array_equal(_bits(none["eig"]), _bits(want["eig"]))
        every = _run(pm, 3.0, 1e-3)
        assert np.array_equal(_bits(every["s"]), _bits(want["s"]))
        assert np.array_equal(every["keypoints"], np.flatnonzero(want["s"] > 0).astype(np.int32)) and len(every["keypoints"]) > 1000
        bare = _run(pm, 3.0, 2.0, eig=False)
        assert bare["eig"] is None and np.array_equal(bare["n"], want["n"]) and np.array_equal(_bits(bare["s"]), _bits(want["s"]))
        assert np.array_equal(bare["keypoints"], want["keypoints"])
    finally:
        pm.close()


def test_workspace_size_is_exact():
    """one byte short is refused as a bad argument; a canary behind the reported size survives; keypoints without a count is refused"""
    from pcreg_amd import _lib as _l
    from pcreg_amd.api import iss_args
    L = _l.lib()
    model = _family("sheet")
    M = len(model)
    pm, _t = _prepared(model)
    try:
        want = _run(pm, 3.0, 2.0)
        need = int(L.pcreg_dev_model_iss_workspace(M))
        r256 = lambda b: -(-b // 256) * 256
        assert need == r256(M) + r256(4 * 1)
        new = lambda: (torch.full((M,), -7, dtype=torch.int32, device=_dev()), torch.full((M, 3), -7.0, dtype=torch.float64, device=_dev()),
                       torch.full((M,), -7.0, dtype=torch.float64, device=_dev()), torch.full((M,), -7, dtype=torch.int32, device=_dev()),
                       torch.full((1,), -7, dtype=torch.int32, device=_dev()))
        nn, ev, sal, kp, n = new()
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        a = iss_args(3.0, 2.0, *DEF)
        assert L.pcreg_dev_model_iss_f32(pm.handle, *a, _p(nn), _p(ev), _p(sal), _p(kp), _p(n), _p(ws), C.c_size_t(need - 1), None) == _l.PCREG_E_ARG
        assert b"bad argument" in L.pcreg_last_error()
        assert L.pcreg_dev_model_iss_f32(pm.handle, *a, _p(nn), _p(ev), _p(sal), _p(kp), None, _p(ws), C.c_size_t(need), None) == _l.PCREG_E_ARG
        torch.cuda.synchronize()
        assert (nn == -7).all().item() and (n == -7).all().item()
        _l.check(L.pcreg_dev_model_iss_f32(pm.handle, *a, _p(nn), _p(ev), _p(sal), _p(kp), _p(n), _p(ws), C.c_size_t(need), None))
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item()
        got = _host(dict(n_neighbors=nn, eig=ev, saliency=sal, keypoints=kp, n_keypoints=n))
        assert _same(got, want) and (kp.cpu().numpy()[len(want["keypoints"]):] == -7).all()
    finally:
        pm.close()


# ---- 4. culling soundness -------------------------------------------------------------------------------------------------
def test_small_cluster_far_from_the_rest(debug_set):
    """five rows 1000 units from a cloud of 700: they see each other and nothing else, with and without culling"""
    rng = np.random.default_rng(11)
    small = rng.normal(0, 0.6, (5, 3)) + np.array([1100.0, 30.0, 10.0])
    rest = _family("volume")[:700].astype(np.float64)
    order = rng.permutation(705)
    model = np.vstack([small, rest])[order].astype(np.float32)
    small_rows = np.flatnonzero(order < 5)
    r = ref.iss(model, ref.r2_of(3.0), ref.r2_of(2.0))
    assert (r["n"][small_rows] == 5).all()
    pm, _t = _prepared(model)
    try:
        a = _run(pm, 3.0, 2.0)
        debug_set("knn_nocull", 1)
        b = _run(pm, 3.0, 2.0)
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    _check_against(a, r, model, 2.0, "two clusters")
    assert _same(a, b) and (a["n"][small_rows] == 5).all()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------
def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def test_determinism_on_the_large_sheet(debug_set):
    """the same bits across two calls, without culling, on two streams, and -- what the exact sums buy -- on a SHUFFLED copy of the
    rows: n, the eigenvalues and the saliency of every row map back through the permutation bit for bit, and so does the keypoint
    status of every row whose saliency no other row shares (an exact tie goes to the lower row NUMBER, which a shuffle changes)"""
    from pcreg_amd._lib import lib
    import normals_ref
    model = normals_ref.family("sheet", 65536)
    M, rs, rn = len(model), 1.0, 0.75
    pm, _t = _prepared(model)
    try:
        debug_set("knn_stats", 1)
        _stats()
        a = _run(pm, rs, rn)
        searches, visited, nominal, _tail = _stats()
        n_tiles = (M + 511) // 512
        print(f"sheet M = 65536 r = ({rs}, {rn}): {visited} of {nominal} tile visits ({100.0 * visited / nominal:.2f} %), "
              f"n in {a['n'].min()}..{a['n'].max()}, {len(a['keypoints'])} keypoints")
        assert searches == 2 and nominal == 2 * n_tiles * n_tiles and 0 < visited < nominal
        debug_set("knn_stats", 0)
        b = _run(pm, rs, rn)
        debug_set("knn_nocull", 1)
        c = _run(pm, rs, rn)
        debug_set("knn_nocull", 0)
        assert _same(a, b) and _same(a, c)
        assert len(a["keypoints"]) > 100 and a["n"].min() >= 1 and not np.isnan(a["eig"]).any()
        # two streams sharing the handle, buffers of their own
        need = max(int(lib().pcreg_dev_model_iss_workspace(M)), 256)
        outs = [(torch.full((M,), -7, dtype=torch.int32, device=_dev()), torch.full((M, 3), -7.0, dtype=torch.float64, device=_dev()),
                 torch.full((M,), -7.0, dtype=torch.float64, device=_dev()), torch.full((M,), -7, dtype=torch.int32, device=_dev()),
                 torch.full((1,), -7, dtype=torch.int32, device=_dev()), torch.full((need,), 0x5A, dtype=torch.uint8, device=_dev()))
                for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                pm.iss_keypoints(rs, rn, *DEF, out=o)
        torch.cuda.synchronize()
        for o in outs:
            assert _same(_host(dict(n_neighbors=o[0], eig=o[1], saliency=o[2], keypoints=o[3], n_keypoints=o[4])), a)
    finally:
        pm.close()
    perm = np.random.default_rng(17).permutation(M)
    d = _iss(model[perm], rs, rn)
    back = np.empty(M, np.int64)
    back[perm] = np.arange(M)                                      # row i of the model is row back[i] of the shuffled copy
    assert np.array_equal(d["n"][back], a["n"]) and np.array_equal(_bits(d["eig"][back]), _bits(a["eig"]))
    assert np.array_equal(_bits(d["s"][back]), _bits(a["s"]))
    vals, counts = np.unique(a["s"], return_counts=True)
    alone = np.isin(a["s"], vals[counts == 1]) & (a["s"] > 0)
    ka, kd = np.zeros(M, bool), np.zeros(M, bool)
    ka[a["keypoints"]] = True
    kd[perm[d["keypoints"]]] = True
    assert np.array_equal(ka[alone], kd[alone]) and alone.sum() > 0.9 * (a["s"] > 0).sum()


# ---- 6. tiers -------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    model = _family("volume")
    for rs, rn, mn in ((3.0, 2.0, 5), (2.0, 2.0, 8)):
        want = _iss(model, rs, rn, mn=mn)
        with pc.Model(model) as h:
            a = h.iss_keypoints(rs, rn, min_neighbors=mn)
        b = pc.point_iss(model, rs, rn, min_neighbors=mn)
        for got in (a, b):
            assert got["n_neighbors"].dtype == np.int32 and got["keypoints"].dtype == np.int32 and got["eig"].shape == (len(model), 3)
            assert np.array_equal(got["n_neighbors"], want["n"]) and np.array_equal(_bits(got["eig"]), _bits(want["eig"]))
            assert np.array_equal(_bits(got["saliency"]), _bits(want["s"])) and np.array_equal(got["keypoints"], want["keypoints"])
    e = pc.point_iss(np.zeros((0, 3)), 1.0, 1.0)
    assert e["keypoints"].shape == (0,) and e["n_neighbors"].shape == (0,) and e["eig"].shape == (0, 3) and e["saliency"].shape == (0,)
    with pytest.raises(ValueError):
        pc.point_iss(model, 0.0, 1.0)


# ---- 7. the chain: normals -> fpfh -> iss -> getMatches on the keypoints -> ransac --------------------------------------------------
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


def test_registration_chain_on_keypoints_recovers_the_motion():
    """The height field of 2048 rows and its copy under a rotation of 0.7 rad about (0.3, -0.5, 0.8) and a translation, rounded to
    fp32.  On both clouds: normals from the library at k = 9 with the viewpoint moved along, fpfh at k = 16, ISS keypoints at
    SalientRadius 3, NonMaxRadius 1.5 (thresholds 0.975, five neighbours); getMatches at D = 33 (SSD, MatchThreshold 100, MaxRatio
    0.9, Unique) on the KEYPOINT rows only; ransac on the matched coordinates.  Every point of the copy must come back to within
    half the cloud's median nearest-neighbour distance (0.2165) of its original.
    The reference chain (iss_ref, fpfh_ref on normals_ref's normals, the oracle's getMatches and ransac) finds 134 keypoints in
    either cloud (133 of them the same rows), keeps 128 pairs, all of them correct, and brings every point to within 9.2e-6: a
    margin of 2.3e4 under the condition.  (At radii (3, 1): 434 / 435 keypoints, 380 pairs, 8.6e-6; at (2, 1): 486 / 490, 418 pairs
    of which 99.5 % correct, 2.8e-4.)"""
    import pcreg_amd as pc
    import fpfh_ref
    a, b, R, t = _chain_scene()
    vp_a = np.array(fpfh_ref.VIEWPOINT)
    vp_b = R @ vp_a + t
    desc, kps = [], []
    for cloud, vp in ((a, vp_a), (b, vp_b)):
        with pc.Model(cloud) as h:
            desc.append(h.fpfh(16, k_normals=9, viewpoint=vp))
            kps.append(h.iss_keypoints(3.0, 1.5)["keypoints"])
    ka, kb = kps
    assert len(ka) >= 50 and len(kb) >= 50
    par = dict(UNNORMALIZE=False, CHANGE_METRIC=False, Method="Exhaustive", MatchThreshold=100.0, MaxRatio=0.9, Metric="SSD", Unique=True)
    pairs = pc.getMatches(np.ascontiguousarray(desc[1][kb]), np.ascontiguousarray(desc[0][ka]), par)      # surface: the copy; model: the original
    assert len(pairs) >= 50
    rb, ra = kb[pairs[:, 0] - 1], ka[pairs[:, 1] - 1]
    p1 = b[rb].astype(np.float64)
    p2 = a[ra].astype(np.float64)
    coef = dict(minPtNum=3, iterNum=2000, thDist=0.05, thInlrRatio=0.1, REFINE=True, VERBOSE=0)
    T, inl, _ns, mi, _ratio = pc.ransac(p1, p2, coef, pc.estimateTransform, pc.calcDists, seed=7)
    assert T.shape == (4, 4) and mi >= 50
    back = (np.hstack([b.astype(np.float64), np.ones((len(b), 1))]) @ np.linalg.inv(T))[:, :3]      # [original, 1] T = [copy, 1]
    err = np.linalg.norm(back - a.astype(np.float64), axis=1)
    _idx, d2 = knn_k_ref.knn(a, a, 2)
    half = float(np.median(np.sqrt(d2[:, 1].astype(np.float64)))) / 2
    print(f"chain: {len(ka)} / {len(kb)} keypoints, {len(pairs)} pairs ({(ra == rb).mean():.3f} correct), {mi} inliers, "
          f"worst distance {err.max():.3e}, half the median nearest-neighbour distance {half:.4f}")
    assert (err <= half).all()
