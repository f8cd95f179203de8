"""Every device-tier entry that takes a workspace stays inside the size its size function reports.

Each case allocates need + 1 MiB, fills the last MiB with a byte pattern, passes workspace_bytes = need exactly and asserts:
the call succeeds, the guard still holds the pattern (a stray write past the reported size would land there, in memory this
test owns), and the outputs equal those of the same call on a separately allocated, generously sized workspace.  Once per entry
workspace_bytes = need - 1 must be refused with PCREG_E_WORKSPACE.  The cases take every branch of the launchers that lays its
buffers out differently (one layout function per workspace).

The tight workspace holds 0xFF below `need` and the roomy one 0x00, so the comparison of the two also shows a launcher that reads
a word before it writes it; every output is a tensor of sentinels between guards (tests/ws_state.py), so a slot that is never
written does not read as a plausible 0 and a write in front of or behind an output shows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ws_state
from conftest import rigid_case

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 1 << 20, 0xA5


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a, b, where=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    else:
        np.testing.assert_array_equal(a, b, err_msg=where)


def _guarded(fn):
    """fn(ws, new) -> outputs, new(shape, dtype) allocating every output as sentinels between guards that must come back untouched"""
    def call(ws):
        outs = ws_state.Outputs()
        got = fn(ws, outs.new)
        outs.check_guards()
        return got
    return call


def _check_bounds(need, call, refuse=True):
    """call(ws) -> outputs (nested dicts / lists of arrays); ws = (workspace tensor, the workspace_bytes to pass)"""
    from pcreg_amd._lib import PCREG_E_WORKSPACE, PcregError
    need = int(need)
    assert need > 0
    tight = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    tight[need:] = PATTERN
    out = call((tight, need))
    torch.cuda.synchronize()
    assert bool((tight[need:] == PATTERN).all()), "a write past the reported workspace size"
    roomy = torch.zeros(2 * need + GUARD, dtype=torch.uint8, device=_dev())
    _same(out, call((roomy, roomy.numel())))
    if refuse:
        with pytest.raises(PcregError) as e:
            call((tight, need - 1))
        assert e.value.code == PCREG_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((tight[need:] == PATTERN).all())


# ---- pcreg_dev_ransac ------------------------------------------------------------------------------------------------
_STAGED = dict(n=5000, iters=2000)
RANSAC_CASES = [
    pytest.param(dict(n=1000, iters=2000), {}, True, id="resident-fp32-screen"),
    pytest.param(dict(n=2049, iters=10000), {}, False, id="staged-2049"),
    pytest.param(_STAGED, {}, False, id="staged-5000"),
    pytest.param(dict(_STAGED, REFINE=False), {}, False, id="staged-5000-norefine"),
    pytest.param(_STAGED, dict(ransac_pass2=1), False, id="staged-full-pass2"),
    pytest.param(_STAGED, dict(ransac_pass2=2), False, id="staged-bounded-pass2"),
    pytest.param(_STAGED, dict(ransac_nolane=1), False, id="staged-nolane"),
    pytest.param(_STAGED, dict(ransac_f64score=1), False, id="staged-f64score"),
    pytest.param(_STAGED, dict(ransac_fused=1), False, id="fused-tiled"),
    pytest.param(dict(n=1000, iters=2000), dict(ransac_resident_f64=1), False, id="resident-f64"),
]


@pytest.mark.parametrize("shape,flags,refuse", RANSAC_CASES)
def test_dev_ransac(shape, flags, refuse, debug_set):
    from pcreg_amd._lib import lib
    from test_gpu_ransac_bound import _dev_ransac
    n, iters = shape["n"], shape["iters"]
    p1, p2, _ = rigid_case(n, 300 + n, noise=0.05, outlier_frac=0.3)
    coef = dict(minPtNum=3, iterNum=iters, thDist=0.1, thInlrRatio=0.1, REFINE=shape.get("REFINE", True), VERBOSE=0)
    for key, value in flags.items():
        debug_set(key, value)
    out = []
    _check_bounds(lib().pcreg_dev_ransac_workspace(n, iters), _guarded(lambda ws, new: out.append(_dev_ransac(p1, p2, coef, 9, ws=ws, alloc=new)) or out[-1]), refuse)
    assert not out[0]["failed"] and out[0]["max_inliers"] > n // 2


@pytest.mark.parametrize("cap,sizes", [(3000, [500, 1500, 2500, 3000]), (4000, [1000, 4000, 2500])],
                         ids=["fp32-launch-plus-fp64-launch", "tiled"])
def test_dev_ransac_batched(cap, sizes):
    from pcreg_amd._lib import lib
    B, iters = len(sizes), 500
    call = _guarded(lambda ws, new: ws_state.ransac_batched_call(sizes, cap, iters, 11, ws[0], ws[1], new))
    first = []
    _check_bounds(lib().pcreg_dev_ransac_batched_workspace(cap, iters, B), lambda ws: first.append(call(ws)) or first[-1])
    assert all(r["counts"][3] == 0 and r["counts"][2] > n // 2 for r, n in zip(first[0], sizes))


# ---- pcreg_dev_get_matches, pcreg_dev_get_matches_segmented ----------------------------------------------------------------
PAR = dict(UNNORMALIZE=True, norm_factor=2, CHANGE_METRIC=True, metric_factor=0.6, Method="Approximate",
           MatchThreshold=20, MaxRatio=0.9, Metric="SAD", Unique=True, VERBOSE=0)


def _count_descriptors(Q, M, D, seed):
    rng = np.random.default_rng(seed)
    dM = rng.poisson(3.0, (M, D)).astype(np.float64)
    return dM[rng.choice(M, Q, replace=False)] + rng.poisson(0.3, (Q, D)), dM


@pytest.mark.parametrize("par_over", [dict(), dict(Unique=False), dict(Metric="SSD", MatchThreshold=1.0)], ids=["sad-unique", "sad", "ssd-unique"])
def test_dev_get_matches(par_over):
    from pcreg_amd import _lib
    from pcreg_amd.api import _match_opts
    L = _lib.lib()
    Q, M, D = 300, 900, 64
    dS, dM = _count_descriptors(Q, M, D, 2)
    o = _match_opts(dict(PAR, **par_over))
    call = _guarded(lambda ws, new: ws_state.get_matches_call(dS, dM, dict(PAR, **par_over), ws[0], ws[1], new))
    first = []
    _check_bounds(L.pcreg_dev_get_matches_workspace(Q, M, D), lambda ws: first.append(call(ws)) or first[-1], refuse=not par_over)
    if o.metric == _lib.METRIC_SAD:
        assert first[0]["k"] > Q // 4


def test_dev_get_matches_segmented():
    from pcreg_amd._lib import lib
    from test_gpu_sweep import _segments_direct
    Q, VM, D = 260, 3000, 96
    dS, dM = _count_descriptors(Q, VM, D, 6)
    rng = np.random.default_rng(7)
    rows_list = [np.sort(rng.choice(VM, n, replace=False)) for n in (1800, 700, 1, 2500)] + [np.zeros(0, np.int64), np.arange(VM)]
    S, tot, n_max = len(rows_list), sum(len(r) for r in rows_list), VM
    need = lib().pcreg_dev_get_matches_segmented_workspace(Q, VM, D, S, tot, n_max)
    _check_bounds(need, _guarded(lambda ws, new: _segments_direct(dS, dM, rows_list, PAR, metric=True, ws=ws, alloc=new)))


# ---- pcreg_dev_spatial_histogram_descriptors ----------------------------------------------------------------------------------
def test_dev_descriptors():
    from pcreg_amd._lib import lib
    from test_gpu_descriptors import OPT, keypoints, strips
    L = lib()
    pts_h, kp_h = strips(40000, 0), keypoints(300, 1)
    P, S = len(pts_h), len(kp_h)
    call = _guarded(lambda ws, new: ws_state.descriptors_call(pts_h, kp_h, OPT, ws[0], ws[1], new))
    first = []
    _check_bounds(L.pcreg_dev_spatial_histogram_descriptors_workspace(P, S), lambda ws: first.append(call(ws)) or first[-1])
    assert first[0]["counters"][0] > 50 and first[0]["counters"][1] == 0


# ---- the point searches ------------------------------------------------------------------------------------------------------
def _points(M, Q, seed):
    rng = np.random.default_rng(seed)
    model = (rng.random((M, 3)) * [100, 56, 99]).astype(np.float32)
    surf = (model[rng.choice(M, Q, replace=False)] + rng.normal(0, 0.05, (Q, 3))).astype(np.float32)
    return model, surf


def test_dev_model_search_and_knn():
    from pcreg_amd._lib import check, lib
    from test_gpu_knn_k import _prepared, _soa, _top2
    L = lib()
    M, Q, k = 50000, 3000, 8                                                # M above the seeding grid's minimum
    model, surf = _points(M, Q, 3)
    pm, _keep = _prepared(model)
    _check_bounds(L.pcreg_dev_model_search_workspace(Q, M), _guarded(lambda ws, new: list(_top2(pm, surf, ws=ws, alloc=new))))
    q = _soa(surf)

    def knn(ws, new):
        idx = new((Q, k), torch.int32); dist = new((Q, k), torch.float32)
        check(L.pcreg_dev_model_knn_f32(pm.handle, _p(q), Q, Q, k, C.c_int32(0), _p(idx), _p(dist), _p(ws[0]), C.c_size_t(ws[1]), _stream()))
        return [idx.cpu().numpy(), dist.cpu().numpy()]

    _check_bounds(L.pcreg_dev_model_knn_workspace(Q, M, k), _guarded(knn))


@pytest.mark.parametrize("exact", [0, 1], ids=["certified-f16", "knn_exact"])
def test_dev_knn2_points(exact, debug_set):
    from pcreg_amd._lib import check, lib
    from test_gpu_knn_k import _soa
    L = lib()
    M, Q = 50000, 3000
    model, surf = _points(M, Q, 4)
    m, q = _soa(model), _soa(surf)
    if exact:
        debug_set("knn_exact", 1)

    def call(ws, new):
        idx = new((Q, 2), torch.int32); dist = new((Q, 2), torch.float32)
        check(L.pcreg_dev_knn2_points_f32(_p(q), Q, Q, _p(m), M, M, C.c_int32(0), _p(idx), _p(dist), _p(ws[0]), C.c_size_t(ws[1]), _stream()))
        return [idx.cpu().numpy(), dist.cpu().numpy()]

    first = []
    _check_bounds(L.pcreg_dev_knn2_points_f32_workspace(Q, M), lambda ws: first.append(_guarded(call)(ws)) or first[-1], refuse=not exact)
    assert (first[0][0][:, 0] >= 0).all() and (np.diff(first[0][1], axis=1) >= 0).all()


# ---- pcreg_dev_sphere_select --------------------------------------------------------------------------------------------------
def test_dev_sphere_select():
    from pcreg_amd._lib import lib
    L = lib()
    V = 6000
    feat = np.random.default_rng(5).uniform([0, 0, 0], [40, 30, 20], (V, 3))
    call = _guarded(lambda ws, new: ws_state.sphere_select_call(feat, (22.0, 14.0, 9.0), 8.0, ws[0], ws[1], new))
    first = []
    _check_bounds(L.pcreg_dev_sphere_select_workspace(V), lambda ws: first.append(call(ws)) or first[-1])
    assert 100 < first[0]["k"] < V
