"""DBSCAN of a prepared model (knn_dbscan.hip, knn_cluster.hip) on the GPU against tests/dbscan_ref.py, every output
bit for bit: label, n_clusters, core, count, first and sizes of the device tier, and the host tiers' CSR lists.  The sizes are the
smallest at which the kernels can go wrong: a tile is 512 rows, a workgroup owns 64, a scan chunk is 2048.  Every device case runs
again with culling off ("knn_nocull") and with the "same root" early-out off ("cluster_noskip")."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dbscan_ref as ref
import knn_cull_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.array([101.0, 56.0, 99.0])
U = 2.0 ** -24
EPS = (1.0, 1.5, 2.0, 3.0)
MINPTS = (1, 2, 4, 8, 12)


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    x = np.asarray(model, np.float32).reshape(-1, 3)
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
    return PreparedModel(t), t


KEYS = ("label", "n_clusters", "core", "count", "first", "sizes")


def _dbscan(pm, r2, minpts):
    out = pm.dbscan(r2, minpts)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in zip(KEYS, out)}
    got["n_clusters"] = int(got["n_clusters"][0])
    return got


def _equal_ref(got, want, what=""):
    nc = got["n_clusters"]
    assert got["label"].dtype == np.int32 and got["count"].dtype == np.int32 and got["core"].dtype == np.uint8
    assert nc == want["n_clusters"], (what, nc, want["n_clusters"])
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=what)
    np.testing.assert_array_equal(got["core"] != 0, want["core"], err_msg=what)
    assert set(np.unique(got["core"]).tolist()) <= {0, 1}
    np.testing.assert_array_equal(got["label"], want["label"], err_msg=what)
    np.testing.assert_array_equal(got["first"][:nc], want["first"], err_msg=what)
    np.testing.assert_array_equal(got["sizes"][:nc], want["sizes"], err_msg=what)
    assert not got["first"][nc:].any() and not got["sizes"][nc:].any(), what        # zeros at and past n_clusters


def _check(pm, r2, minpts, debug_set, want):
    what = f"M = {pm.M}, r2 = {float(r2)!r}, minpts = {minpts}"
    _equal_ref(_dbscan(pm, r2, minpts), want, what)
    for key in ("knn_nocull", "cluster_noskip"):
        debug_set(key, 1)
        try:
            _equal_ref(_dbscan(pm, r2, minpts), want, what + ", " + key)
        finally:
            debug_set(key, 0)
    return want


def _check_cloud(model, r2, minpts, debug_set):
    pm, _t = _prepared(model)
    try:
        return _check(pm, r2, minpts, debug_set, ref.dbscan(model, r2, minpts))
    finally:
        pm.close()


# ---- the lattice family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 511, 512, 513, 1500, 2049, 4100])
def test_lattice_family(M, debug_set):
    model = ref.lattice_cloud(500 + M, M)
    d2 = ref.d2_matrix(model)
    pm, _t = _prepared(model)
    kinds = np.zeros(3, np.int64)
    try:
        for eps in EPS:
            r2 = np.float32(eps) ** 2
            adj = ref.neighbours(model, r2, d2=d2)
            for minpts in MINPTS:
                want = _check(pm, r2, minpts, debug_set, ref.dbscan_from(adj, minpts))
                kinds += [want["core"].sum(), want["border"].sum(), want["noise"].sum()]
    finally:
        pm.close()
    print(f"M = {M}: core / border / noise rows over the 20 settings: {kinds.tolist()}")
    if M >= 63:
        assert kinds.all(), kinds                                  # premise: the family shows all three kinds of rows


# ---- contested border rows --------------------------------------------------------------------------------------------------
def _two_blobs(pad=0):
    """eps = 2, minpts = 6: blob A = (0,0,0), 3 x (-1,0,0), 3 x (-2,0,0); blob B its mirror image about x = 2; two rows at (2,0,0),
    at distance exactly eps from the core rows (0,0,0) and (4,0,0) and with 4 neighbours each.  pad: more rows for A, x <= -3"""
    A = [[0, 0, 0]] + [[-1, 0, 0]] * 3 + [[-2, 0, 0]] * 3 + [[-3 - (k % 6), k % 2, 0] for k in range(pad)]
    Bb = [[4, 0, 0]] + [[5, 0, 0]] * 3 + [[6, 0, 0]] * 3
    mid = [[2, 0, 0]] * 2
    return np.array(A, np.float32), np.array(Bb, np.float32), np.array(mid, np.float32)


def _contested(model, r2, want):
    """the border rows with core neighbours in two or more clusters, by the reference's lists alone"""
    indptr, indices = ref.neighbours(model, r2)
    out = []
    for i in np.flatnonzero(want["border"]):
        nb = indices[indptr[i]:indptr[i + 1]]
        if len(set(want["label"][nb[want["core"][nb]]].tolist())) >= 2:
            out.append(int(i))
    return out


@pytest.mark.parametrize("case", ["a_first", "b_first", "border_first", "two_tiles"])
def test_contested_border_rows(case, debug_set):
    A, Bb, mid = _two_blobs(pad=505 if case == "two_tiles" else 0)
    parts = {"a_first": [A, mid, Bb], "b_first": [Bb, mid, A], "border_first": [mid, Bb, A], "two_tiles": [mid[:1], Bb, A, mid[1:]]}[case]
    model = np.vstack(parts)
    r2, minpts = np.float32(4.0), 6
    want = ref.dbscan(model, r2, minpts)
    rows_mid = np.flatnonzero((model == [2, 0, 0]).all(axis=1))
    a0 = int(np.flatnonzero((model == [0, 0, 0]).all(axis=1))[0]); b0 = int(np.flatnonzero((model == [4, 0, 0]).all(axis=1))[0])
    # premises, by the reference alone: two clusters, both (2,0,0) rows contested, and they go with the blob whose core rows come first
    assert want["n_clusters"] == 2 and want["core"][a0] and want["core"][b0] and want["label"][a0] != want["label"][b0]
    assert _contested(model, r2, want) == rows_mid.tolist() and list(want["count"][rows_mid]) == [4, 4]
    assert (want["label"][rows_mid] == 0).all() and want["label"][a0 if case == "a_first" else b0] == 0
    if case == "border_first":
        assert rows_mid[0] == 0 and want["first"][0] > 1             # the border row has the smallest index of all and starts nothing
    pm, _t = _prepared(model)
    try:
        if case == "two_tiles":
            from pcreg_amd._lib import check, lib
            perm = torch.empty(pm.M, dtype=torch.int32, device=_dev())
            tb = torch.empty(6 * ((pm.M + 511) // 512), dtype=torch.float32, device=_dev())
            prep = (C.c_float * 24)()
            check(lib().pcreg_debug_dev_model_export(pm.handle, _p(perm), None, _p(tb), prep, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            tile_of = knn_cull_ref.row_tiles(perm.cpu().numpy())
            assert pm.M > 512 and tile_of[a0] != tile_of[b0], "premise: the blobs' core rows lie in different tiles"
        _check(pm, r2, minpts, debug_set, want)
    finally:
        pm.close()


# ---- thresholds -------------------------------------------------------------------------------------------------------------
def test_minpts_and_the_radius_are_inclusive(debug_set):
    # three rows at the origin and one at (3, 4, 0): distance exactly 5, r2 = 25 exact
    model = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    w = _check_cloud(model, np.float32(25.0), 4, debug_set)
    assert w["count"].tolist() == [4, 4, 4, 4] and w["core"].all() and w["n_clusters"] == 1          # exactly minpts neighbours: core
    w = _check_cloud(model, np.float32(25.0), 5, debug_set)
    assert not w["core"].any() and (w["label"] == -1).all() and w["n_clusters"] == 0                 # minpts - 1: not core
    below = np.nextafter(np.float32(25.0), np.float32(0.0))
    w = _check_cloud(model, below, 3, debug_set)
    assert w["count"].tolist() == [3, 1, 3, 3] and w["label"].tolist() == [0, -1, 0, 0]              # a hair inside eps: not a neighbour
    w = _check_cloud(model, np.float32(25.0), 2, debug_set)
    assert w["label"].tolist() == [0, 0, 0, 0]
    # a row with minpts - 1 neighbours beside a core row is a border row: (0,0,0) x 3 and (1,0,0) with eps = 1, minpts = 4
    model = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0]], np.float32)
    w = _check_cloud(model, np.float32(1.0), 4, debug_set)
    assert w["count"].tolist() == [5, 4, 4, 4, 2] and w["core"].tolist() == [True] * 4 + [False] and w["label"].tolist() == [0] * 5
    w = _check_cloud(model, np.float32(1.0), 5, debug_set)
    assert w["core"].tolist() == [True, False, False, False, False] and w["label"].tolist() == [0] * 5 and w["first"].tolist() == [0]


def test_the_32u_window_with_minpts_2(debug_set):
    """4.11's window: tile 0 is 512 rows with x <= 0.75, tile 1 begins at x = b; g = b - 0.75 is exact and fl(g * g) < g^2, so with
    r2 = fl(g * g) the rows (0.75, .5, .5) and (b, .5, .5) are neighbours although the boxes' gap G2 > r2; only the 32u margin keeps
    the pair of tiles, in the count walk, the core walk and the border walk alike"""
    rng = np.random.default_rng(3)
    for k in range(1, 1000):
        b = np.float32(1.0) + np.float32(k * 2.0 ** -23)
        g = np.float32(b - np.float32(0.75))
        if float(g) == float(b) - 0.75 and float(g * g) < float(g) * float(g):
            break
    r2 = np.float32(g * g)
    A = np.column_stack([rng.uniform(0.0, 0.7, 512), rng.uniform(0.0, 0.95, 512), rng.uniform(0.0, 0.95, 512)])
    A[0] = [0, 0, 0]
    A[1] = [0.75, 0.5, 0.5]
    B = np.column_stack([rng.uniform(1.3, 1.9, 511), rng.uniform(0.0, 0.95, 511), rng.uniform(0.0, 0.95, 511)])
    B[0] = [float(b), 0.5, 0.5]
    model = np.vstack([B[:200], A, B[200:], [[64.0, 64.0, 64.0]]]).astype(np.float32)
    ia, ib = 201, 0
    indptr, indices = adj = ref.neighbours(model, r2)
    want = ref.dbscan_from(adj, 2)
    assert ia in indices[indptr[ib]:indptr[ib + 1]], "premise: the two rows are neighbours"
    assert want["label"][ia] == want["label"][ib] >= 0 and want["label"][-1] == -1
    pm, _t = _prepared(model)
    try:
        _check(pm, r2, 2, debug_set, want)
        # the same pair decides a border row: with minpts = count[ib] + 1 row ib is not core
        for minpts in (int(want["count"][ib]) + 1, int(want["count"][ia]) + 1):
            _check(pm, r2, minpts, debug_set, ref.dbscan_from(adj, minpts))
    finally:
        pm.close()


# ---- minpts = 1 is clusterPoints ---------------------------------------------------------------------------------------------
def _float_cloud(M, seed, scale=0.3):
    return (np.random.default_rng(seed).random((M, 3)) * BOX * scale).astype(np.float32)


def test_minpts_1_equals_cluster():
    for model, radii in ((ref.lattice_cloud(7, 1500), (1.0, 2.0)), (_float_cloud(6000, 21, 0.2), (0.0, 0.7, 1.1, np.inf)),
                         (ref.lattice_cloud(8, 513), (0.0, 1.5))):
        pm, _t = _prepared(model)
        try:
            for r in radii:
                r2 = np.float32(r) ** 2
                label, nc, first, sizes = pm.cluster(r2)
                got = _dbscan(pm, r2, 1)
                torch.cuda.synchronize()
                assert got["n_clusters"] == int(nc.item())
                for key, t in (("label", label), ("first", first), ("sizes", sizes)):
                    np.testing.assert_array_equal(got[key], t.cpu().numpy(), err_msg=f"{key}, r = {r}")
                assert got["core"].all() and (got["count"] >= 1).all()
        finally:
            pm.close()


# ---- non-finite rows ---------------------------------------------------------------------------------------------------------
def test_non_finite_rows_are_noise(debug_set):
    rng = np.random.default_rng(31)
    model = (rng.random((3000, 3)) * 12).astype(np.float32)
    bad = np.sort(np.concatenate([[0, 2999], rng.choice(np.arange(1, 2999), 28, replace=False)]))
    for k, i in enumerate(bad):
        model[i] = [[np.nan, 1, 1], [np.inf, 1, 1], [3, -np.inf, 1], [np.nan, np.inf, -np.inf], [np.inf, np.inf, np.inf]][k % 5]
    model[bad[5]] = model[bad[10]] = [np.inf, 2.0, 3.0]           # coincident twins: not each other's neighbours either
    pm, _t = _prepared(model)
    try:
        for r2, minpts in ((np.float32(0.8) ** 2, 1), (np.float32(0.8) ** 2, 4), (np.float32(1.2) ** 2, 8), (np.float32(np.inf), 5)):
            want = _check(pm, r2, minpts, debug_set, ref.dbscan(model, r2, minpts))
            got = _dbscan(pm, r2, minpts)
            assert (got["label"][bad] == -1).all() and not got["count"][bad].any() and not got["core"][bad].any()
            if r2 == np.inf:                                       # every finite row counts every finite row and nobody else
                assert (np.delete(got["count"], bad) == 3000 - 30).all() and got["n_clusters"] == 1
            else:
                assert want["noise"].sum() > 30 or minpts == 1
    finally:
        pm.close()


# ---- empty and degenerate ----------------------------------------------------------------------------------------------------
def test_empty_and_degenerate(debug_set):
    for M in (1, 5, 700):
        model = ref.lattice_cloud(90 + M, M)
        w = _check_cloud(model, np.float32(1e4), M + 1, debug_set)  # minpts > M: all noise
        assert w["n_clusters"] == 0 and (w["label"] == -1).all() and (w["count"] == M).all()
        w = _check_cloud(model, np.float32(1e4), M, debug_set)
        assert w["n_clusters"] == 1 and w["sizes"].tolist() == [M]
    pm, _t = _prepared(np.zeros((0, 3), np.float32))
    try:
        got = _dbscan(pm, 1.0, 3)
        assert got["n_clusters"] == 0 and all(len(got[k]) == 0 for k in ("label", "core", "count", "first", "sizes"))
    finally:
        pm.close()
    with pytest.raises(ValueError):
        pm.dbscan(-1.0, 3)
    with pytest.raises(ValueError):
        pm.dbscan(1.0, 0)


# ---- one float cloud against the grid reference ----------------------------------------------------------------------------------
def test_float_cloud_equals_the_grid_reference(debug_set):
    model = _float_cloud(20_000, 77)
    pm, _t = _prepared(model)
    try:
        for r, minpts in ((0.9, 5), (1.2, 10)):
            r2 = np.float32(r) ** 2
            want = ref.dbscan(model, r2, minpts, grid=True)
            n = [int(want[k].sum()) for k in ("core", "border", "noise")]
            print(f"20 000 rows, r = {r}, minpts = {minpts}: {n[0]} core, {n[1]} border, {n[2]} noise rows, {want['n_clusters']} clusters")
            assert min(n) >= 100 and want["n_clusters"] > 1, "premise: all three kinds of rows"
            _check(pm, r2, minpts, debug_set, want)
    finally:
        pm.close()


# ---- row permutations and determinism ----------------------------------------------------------------------------------------
def _renumber(label, core):
    """the numbering rule applied to the core rows of any labelling: clusters in ascending order of their first core row"""
    out = np.full(len(label), -1, np.int64)
    _, first_at, inv = np.unique(label[core], return_index=True, return_inverse=True)
    rank = np.empty(len(first_at), np.int64)
    rank[np.argsort(first_at)] = np.arange(len(first_at))
    out[core] = rank[inv]
    return out


def test_determinism_and_row_permutations():
    model = _float_cloud(5000, 5, 0.2)
    r2, minpts = np.float32(1.0) ** 2, 6
    outs = []
    for _ in range(2):
        pm, _t = _prepared(model)
        try:
            outs += [_dbscan(pm, r2, minpts), _dbscan(pm, r2, minpts)]
        finally:
            pm.close()
    for o in outs[1:]:
        for k in KEYS:
            np.testing.assert_array_equal(o[k], outs[0][k], err_msg=k)
    a = outs[0]
    assert a["n_clusters"] > 5 and 0 < (a["core"] != 0).sum() < len(model) and (a["label"] < 0).any()
    order = np.random.default_rng(9).permutation(len(model))
    pm, _t = _prepared(model[order])
    try:
        b = _dbscan(pm, r2, minpts)
    finally:
        pm.close()
    core = a["core"][order] != 0
    np.testing.assert_array_equal(b["core"], a["core"][order])                       # the core set, the counts and the noise set
    np.testing.assert_array_equal(b["count"], a["count"][order])
    np.testing.assert_array_equal(b["label"] < 0, a["label"][order] < 0)
    np.testing.assert_array_equal(b["label"][core], _renumber(a["label"][order], core)[core])   # the core rows' partition, renumbered
    _equal_ref(b, ref.dbscan(model[order], r2, minpts))                                 # border rows: the rule on the new order


# ---- tiers and callers -------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    from pcreg_amd._lib import check, lib
    for model, r, minpts in ((_float_cloud(4000, 3, 0.2), 1.0, 5), (ref.lattice_cloud(4, 700), 1.5, 8), (ref.lattice_cloud(5, 40), 1.0, 50)):
        r2 = np.float32(r) ** 2
        want = ref.dbscan(model, r2, minpts)
        pm, _t = _prepared(model)
        try:
            _equal_ref(_dbscan(pm, r2, minpts), want)
        finally:
            pm.close()
        with pc.Model(model) as h:
            a = h.dbscan(r2, minpts)
        b = pc.dbscan_points(model, r2, minpts)
        for label, core, off, members in (a, b):
            assert label.dtype == off.dtype == members.dtype == np.int32 and core.dtype == bool
            np.testing.assert_array_equal(label, want["label"])
            np.testing.assert_array_equal(core, want["core"])
            np.testing.assert_array_equal(off, want["cl_off"])
            np.testing.assert_array_equal(members, want["members"])
        # the C entry itself: count as well; label alone
        mf = np.asfortranarray(model)
        M = len(model)
        label = np.full(M, -7, np.int32); count = np.full(M, -7, np.int32); core = np.full(M, 7, np.uint8); nc = C.c_int32(-1)
        check(lib().pcreg_dbscan_points_f32(mf.ctypes.data, M, M, float(r2), minpts, label.ctypes.data, C.byref(nc), core.ctypes.data,
                                            count.ctypes.data, None, None))
        np.testing.assert_array_equal(count, want["count"]); np.testing.assert_array_equal(core != 0, want["core"])
        label[:] = -7
        check(lib().pcreg_dbscan_points_f32(mf.ctypes.data, M, M, float(r2), minpts, label.ctypes.data, C.byref(nc), None, None, None, None))
        np.testing.assert_array_equal(label, want["label"])
        assert nc.value == want["n_clusters"]
    label, core, off, members = pc.dbscan_points(np.zeros((0, 3)), 1.0, 3)
    assert len(label) == 0 and off.tolist() == [0] and len(members) == 0


def test_two_streams_on_one_handle():
    from pcreg_amd._lib import lib
    model = _float_cloud(20_000, 77)
    pm, _t = _prepared(model)
    try:
        args = ((np.float32(0.9) ** 2, 5), (np.float32(1.3) ** 2, 10))
        serial = [_dbscan(pm, *a) for a in args]
        M = pm.M
        need = int(lib().pcreg_dev_model_dbscan_workspace(M))
        outs = [(torch.full((M,), -1, dtype=torch.int32, device=_dev()), torch.full((1,), -1, dtype=torch.int32, device=_dev()),
                 torch.full((M,), 9, dtype=torch.uint8, device=_dev())) + tuple(torch.full((M,), -1, dtype=torch.int32, device=_dev()) for _ in range(3)) +
                (torch.empty(need, dtype=torch.uint8, device=_dev()),) for _ in args]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, a, o in ((s1, args[0], outs[0]), (s2, args[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.dbscan(*a, out=o)
        torch.cuda.synchronize()
        for o, want in zip(outs, serial):
            for k, t in zip(KEYS, o):
                got = t.cpu().numpy()
                np.testing.assert_array_equal(int(got[0]) if k == "n_clusters" else got, want[k], err_msg=k)
        assert serial[0]["n_clusters"] != serial[1]["n_clusters"]
    finally:
        pm.close()


@pytest.fixture(scope="module")
def mexdrv(tmp_path_factory):
    import subprocess
    out = str(tmp_path_factory.mktemp("mexdbscan") / "libmexdbscan.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexdbscan", "dbscan_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    drv = C.CDLL(out)
    drv.dd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                  C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return drv


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, r, minpts", [(3000, 0.9, 4), (5, 40.0, 5), (5, 40.0, 6), (0, 1.0, 3)])
def test_mex_round_trip_equals_the_host_tier(mexdrv, via_handle, M, r, minpts):
    """[label, core, clOff, members] = pcreg_mex('modelDbscan', h, epsilon, minpts) / pcreg_mex('dbscanPoints', single(pts), epsilon,
    minpts) through tests/mexdbscan/dbscan_driver.cpp: 1-based rows and labels, noise -1, epsilon squared once in single"""
    import pcreg_amd as pc
    m = (np.random.default_rng(M + 3).random((M, 3)) * 12).astype(np.float32)
    want = pc.dbscan_points(m, np.float32(r) * np.float32(r), minpts)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    label = np.full(max(M, 1), -7, np.int32); core = np.full(max(M, 1), 7, np.uint8); off = np.full(M + 1, -7, np.int32)
    members = np.full(max(M, 1), -7, np.int32)
    e = C.create_string_buffer(1024); nc = C.c_int(-1); nm = C.c_int(-1)
    assert mexdrv.dd_round_trip(via_handle, mf.ctypes.data, M, float(r), float(minpts), label.ctypes.data, core.ctypes.data, off.ctypes.data,
                                C.byref(nc), members.ctypes.data, C.byref(nm), e, 1024) == 0, e.value
    assert mexdrv.dd_live_arrays() == 0
    assert nc.value == len(want[2]) - 1 and nm.value == len(want[3])
    np.testing.assert_array_equal(label[:M], np.where(want[0] >= 0, want[0] + 1, -1))
    np.testing.assert_array_equal(core[:M] != 0, want[1])
    np.testing.assert_array_equal(off[:nc.value + 1], want[2])
    np.testing.assert_array_equal(members[:nm.value], want[3] + 1)


def test_promising_clusters_with_min_spheres():
    """min_spheres=None is the call without the keyword; with min_spheres=2 a lone promising sphere is in no cluster"""
    from pcreg_amd.sweep import largest_cluster, promising_clusters
    g = np.array([[0, 0, 0], [5, 0, 0], [5, 5, 0], [100, 0, 0], [40, 40, 0], [45, 40, 0]], np.float64)
    n = len(g)
    T = []
    for t in range(n):
        Tt = np.eye(4); Tt[0, 1] = float(t); T.append(Tt)
    res = dict(centres=g, trial=np.arange(n), statsPutative=np.full(n, 300), statsSuccess=np.ones(n, np.int64), statsInliers=np.full(n, 50),
               statsRatio=np.full(n, 50.0), transforms=T)
    plain, none = promising_clusters(res), promising_clusters(res, min_spheres=None)
    assert len(plain) == len(none) == 3
    for (la, Ta), (lb, Tb) in zip(plain, none):
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(Ta, Tb)
    two = promising_clusters(res, min_spheres=2)
    assert len(two) == 2                                           # the sphere at (100, 0, 0) is noise
    for (la, Ta), (lb, Tb) in zip(two, [plain[0], plain[2]]):
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(Ta, Tb)
    a, b = largest_cluster(res), largest_cluster(res, min_spheres=None)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    c = largest_cluster(res, min_spheres=2)
    np.testing.assert_array_equal(c[0], a[0])
    assert largest_cluster(res, min_spheres=4)[0].tolist() == [] and promising_clusters(res, min_spheres=4) == []
