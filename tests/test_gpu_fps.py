"""Farthest point sampling of a prepared model (knn_fps.hip) on the GPU against tests/fps_ref.py, BIT FOR BIT: idx,
dist, n_out, cover_d2, min_dist and label; nothing is excused and there is no tolerance (a NaN is compared as a NaN).  Every output
is pre-filled with a mark, so what the contract says is not written must still hold the mark.  The shapes are the smallest at
which the kernel can go wrong: around a 64-row unit, a 512-row tile, several tiles, more tiles than the workgroup judges in one
trip; every family of the reference; the starts, the stops, the NULL outputs, the dead start row, culling, determinism, the tiers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fps_ref as ref

pytestmark = pytest.mark.gpu
MARK = -7
INF = float("inf")


def _dev():
    return torch.device("cuda", 0)


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


@functools.lru_cache(maxsize=None)
def _family(name, M):
    a = ref.family(name, M)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(name, M, K, start=-1, stop_d2=0.0):
    return ref.fps(_family(name, M), K, start, stop_d2)


def _outs(M, K, fill=0x5A, skip=()):
    """marked output tensors and a workspace of `fill` bytes, in PreparedModel.farthest_points's out= order; skip: names passed as None"""
    from pcreg_amd._lib import lib
    need = int(lib().pcreg_dev_model_fps_workspace(M, K))
    mk = lambda n, dt: torch.full((n,), MARK, dtype=dt, device=_dev())
    o = dict(idx=mk(K, torch.int32), dist=mk(K, torch.float32), n_out=mk(1, torch.int32), cover_d2=mk(1, torch.float32),
             min_dist=mk(M, torch.float32), label=mk(M, torch.int32), info=mk(1, torch.int32))
    for name in skip:
        o[name] = None
    return tuple(o.values()) + (torch.full((need,), fill, dtype=torch.uint8, device=_dev()),)


def _host(res):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


def _run(pm, K, start=-1, stop_d2=0.0, **kw):
    return _host(pm.farthest_points(K, start, stop_d2, out=_outs(pm.M, K, **kw)))


def _eq(a, b):
    """the same floats bit for bit, a NaN being a NaN"""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _check(got, want, what=""):
    """a marked device result against a reference dict; what the contract leaves unwritten still holds the mark"""
    n = want["n_out"]
    assert got["n_out"][0] == n, (what, got["n_out"][0], n)
    if got["info"] is not None:
        assert got["info"][0] == want["info"], what
    if got["idx"] is not None:
        assert np.array_equal(got["idx"][:n], want["idx"]) and (got["idx"][n:] == MARK).all(), what
    if got["dist"] is not None:
        assert _eq(got["dist"][:n], want["dist"]) and (got["dist"][n:] == MARK).all(), what
    if want["info"] == 1:                                         # a dead start row: nothing else is written
        for k in ("cover_d2", "min_dist", "label"):
            assert got[k] is None or (got[k] == MARK).all(), (what, k)
        return
    if got["cover_d2"] is not None:
        assert _eq(got["cover_d2"], want["cover_d2"]), (what, got["cover_d2"], want["cover_d2"])
    if got["min_dist"] is not None:
        assert _eq(got["min_dist"], want["min_dist"]), what
    if got["label"] is not None:
        assert np.array_equal(got["label"], want["label"]), what


# ---- 1. sizes around a unit, a tile and several tiles; K around its edges ---------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 2, 63, 64, 65, 511, 512, 513, 1025, 5000])
def test_sizes_and_k_on_the_surface(M):
    pm, _t = _prepared(_family("surface", M))
    try:
        for K in sorted({0, 1, 2, M, M + 5}):
            _check(_run(pm, K), _ref("surface", M, K), f"M = {M} K = {K}")
    finally:
        pm.close()


# ---- 2. every family ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ref.FAMILIES)
def test_every_family(fam):
    M, K = 4000, 300
    pm, _t = _prepared(_family(fam, M))
    try:
        want = _ref(fam, M, K)
        _check(_run(pm, K), want, fam)
        if fam == "lattice":
            full = _ref(fam, M, M + 5)
            assert full["n_out"] == M // 4                        # stops by itself at the number of distinct positions
            _check(_run(pm, M + 5), full, fam)
        if fam == "overflow":
            assert np.isinf(want["dist"][1:]).any() and np.isfinite(want["dist"]).any()      # +inf distances took part
    finally:
        pm.close()


# ---- 3. the start row, the stop, a dead start --------------------------------------------------------------------------------
def _perm(pm):
    from pcreg_amd._lib import check, lib
    perm = torch.empty(pm.M, dtype=torch.int32, device=_dev())
    check(lib().pcreg_debug_dev_model_export(pm.handle, C.c_void_p(perm.data_ptr()), None, None, (C.c_float * 24)(), None))
    torch.cuda.synchronize()
    return perm.cpu().numpy()


def test_start_rows():
    M, K = 1025, 40
    pm, _t = _prepared(_family("surface", M))
    try:
        last_unit = int(_perm(pm)[M - 1])                         # the one row of the last, partial unit (and tile)
        for start in (-1, 0, M - 1, last_unit):
            _check(_run(pm, K, start), _ref("surface", M, K, start), f"start = {start}")
    finally:
        pm.close()


def test_stops():
    M, K = 4000, 300
    pm, _t = _prepared(_family("cube", M))
    try:
        full = _ref("cube", M, K)
        mid = float(full["dist"][K // 3])
        for stop in (0.0, mid, INF):
            want = _ref("cube", M, K, -1, stop)
            _check(_run(pm, K, -1, stop), want, f"stop_d2 = {stop}")
        assert _ref("cube", M, K, -1, mid)["n_out"] == K // 3 and _ref("cube", M, K, -1, INF)["n_out"] == 1
    finally:
        pm.close()


def test_dead_start_row_and_dead_clouds():
    from pcreg_amd import _lib
    import pcreg_amd as pc
    M = 700
    m = _family("nonfinite", M)
    dead = np.flatnonzero(~np.isfinite(m).all(axis=1))
    assert dead[0] == 0 and len(dead) > 3
    pm, _t = _prepared(m)
    try:
        for start in (0, int(dead[-1])):
            want = _ref("nonfinite", M, 8, start)
            assert want["info"] == 1 and want["n_out"] == 0
            _check(_run(pm, 8, start), want, f"dead start {start}")
        _check(_run(pm, 0, 0), _ref("nonfinite", M, 0, 0), "K = 0 does not look at the start row")
    finally:
        pm.close()
    with pc.Model(m) as model:
        with pytest.raises(RuntimeError) as e:
            model.farthest_points(8, start=0)
        assert "start" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        pc.point_farthest_points(m, 8, start=int(dead[1]))
    assert "start" in str(e.value)
    assert _lib.lib().pcreg_last_error().startswith(b"bad argument")
    none = np.full((130, 3), np.nan, np.float32)
    none[::2, 1] = 1.0
    pm, _t = _prepared(none)
    try:
        _check(_run(pm, 5), ref.fps(none, 5), "no live row")
        want = ref.fps(none, 5, 3)
        assert want["info"] == 1
        _check(_run(pm, 5, 3), want, "no live row, a start given")
    finally:
        pm.close()


# ---- 4. NULL for each optional output in turn ---------------------------------------------------------------------------------
def test_null_outputs():
    M, K = 513, 20
    pm, _t = _prepared(_family("clusters", M))
    try:
        want = _ref("clusters", M, K)
        for name in ("idx", "dist", "cover_d2", "min_dist", "label", "info"):
            _check(_run(pm, K, skip=(name,)), want, f"{name} = NULL")
        _check(_run(pm, K, skip=("idx", "dist", "cover_d2", "min_dist", "label", "info")), want, "n_out alone")
    finally:
        pm.close()


# ---- 5. more tiles than the workgroup judges in one trip ---------------------------------------------------------------------
def test_more_tiles_than_one_trip():
    M, K = 600_000, 64
    assert (M + 511) // 512 > 1024
    pm, _t = _prepared(_family("surface", M))
    try:
        _check(_run(pm, K), _ref("surface", M, K), "M = 600 000")
    finally:
        pm.close()


# ---- 6. culling: the same bits without it, and it culls ------------------------------------------------------------------------
def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 2)()
    check(lib().pcreg_debug_fps_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def test_culling_changes_no_bit_and_culls(debug_set):
    M, K = 20_000, 512
    m = _family("surface", M)
    want = _ref("surface", M, K)
    nf, n = int(np.isfinite(m).all(axis=1).sum()), want["n_out"]
    pm, _t = _prepared(m)
    try:
        debug_set("knn_stats", 1)
        _stats()
        a = _run(pm, K)
        steps, touched = _stats()
        debug_set("knn_nocull", 1)
        b = _run(pm, K)
        steps_all, touched_all = _stats()
        debug_set("knn_nocull", 0)
        debug_set("knn_stats", 0)
        _check(a, want, "culled")
        _check(b, want, "knn_nocull")
        print(f"surface M = {M} K = {K}: {touched} of {touched_all} rows measured ({100.0 * touched / touched_all:.2f} %)")
        assert steps == steps_all == n
        assert touched_all == nf * n
        assert touched < touched_all // 2
    finally:
        pm.close()


# ---- 7. determinism -------------------------------------------------------------------------------------------------------------
def test_determinism_streams_and_workspace_contents():
    M, K = 5000, 200
    pm, _t = _prepared(_family("surface", M))
    try:
        want = _ref("surface", M, K)
        _check(_run(pm, K), want, "first")
        _check(_run(pm, K), want, "again")
        _check(_run(pm, K, fill=0xFF), want, "workspace of 0xFF bytes")
        _check(_run(pm, K, fill=0x00), want, "workspace of zero bytes")
        outs = [_outs(M, K, fill=f) for f in (0xFF, 0x33)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        res = []
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            with torch.cuda.stream(s):
                res.append(pm.farthest_points(K, out=o))
        torch.cuda.synchronize()
        for r in res:
            _check(_host(r), want, "two streams")
        d = _host(pm.farthest_points(K))                          # the cached workspace and tensors of its own
        assert d["n_out"][0] == want["n_out"] and np.array_equal(d["idx"][:want["n_out"]], want["idx"]) and _eq(d["min_dist"], want["min_dist"])
    finally:
        pm.close()


# ---- 8. the tiers ---------------------------------------------------------------------------------------------------------------
def test_tiers_agree():
    import pcreg_amd as pc
    M, K, start = 3000, 150, 17
    m = _family("nonfinite", M)
    stop = float(_ref("nonfinite", M, K, start)["dist"][60])      # the run stops with 60 samples, short of K
    want = _ref("nonfinite", M, K, start, stop)
    assert want["n_out"] == 60 and want["info"] == 0

    def same(r):
        assert r["n_out"] == want["n_out"] and np.array_equal(r["idx"], want["idx"]) and _eq(r["dist"], want["dist"])
        assert _eq(r["cover_d2"], want["cover_d2"]) and _eq(r["min_dist"], want["min_dist"]) and np.array_equal(r["label"], want["label"])
        assert r["idx"].dtype == np.int32 and r["dist"].dtype == np.float32 and r["min_dist"].dtype == np.float32
    same(pc.point_farthest_points(m, K, start, stop))
    with pc.Model(m) as model:
        same(model.farthest_points(K, start=start, stop_d2=stop))
        same(model.farthest_points(K, start, stop))
    pm, _t = _prepared(m)
    try:
        _check(_run(pm, K, start, stop), want, "device tier")
    finally:
        pm.close()
    # the C host tier with a leading dimension of its own and NULL outputs
    from pcreg_amd._lib import check, lib
    ld = M + 3
    buf = np.zeros((3, ld), np.float32)
    buf[:, :M] = m.T
    idx, n = np.full(K, MARK, np.int32), np.zeros(1, np.int32)
    check(lib().pcreg_point_fps_f32(buf.ctypes.data, M, ld, K, start, stop, idx.ctypes.data, None, n.ctypes.data, None, None, None))
    assert n[0] == want["n_out"] and np.array_equal(idx[:n[0]], want["idx"]) and (idx[n[0]:] == MARK).all()
