"""The k-nearest search against a prepared model (knn_k.hip) on the GPU, bit for bit.

k = 1, 2 against the top-2 search (pcreg_dev_model_search_f32); k = 3 .. 32 against the brute-force fp32 reference
(tests/knn_k_ref.c); every query against the same search with culling off ("knn_nocull").  Then the edges (M, Q, scale,
queries outside the box), a case that only a k-th-neighbour bound culls correctly, the visited share at the bench shape, the
shard merge, the host tiers and two streams on one handle."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import knn_k_ref as ref

pytestmark = pytest.mark.gpu
BOX = np.array([101.0, 56.0, 99.0])
CORES = min(len(os.sched_getaffinity(0)), 16)


def _dev():
    return torch.device("cuda", 0)


def _soa(x):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    t = torch.empty((3, max(len(x), 0)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
    return t


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    t = _soa(model)
    return PreparedModel(t), t


def _knn(pm, surf, k, idx_base=0):
    i, d = pm.knn(_soa(surf), k, idx_base)
    torch.cuda.synchronize()
    return i.cpu().numpy(), d.cpu().numpy()


def _top2(pm, surf, ws=None, alloc=None):
    """ws: the caller's (workspace tensor, the workspace_bytes to pass) in place of one of the reported size; alloc(shape, dtype):
    the caller's allocator of the two outputs"""
    from pcreg_amd._lib import check, lib
    Q = len(surf)
    q = _soa(surf)
    alloc = alloc or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=_dev()))
    idx = alloc((Q, 2), torch.int32)
    dist = alloc((Q, 2), torch.float32)
    ws, ws_bytes = ws if ws is not None else (torch.empty(max(lib().pcreg_dev_model_search_workspace(Q, pm.M), 256), dtype=torch.uint8, device=_dev()), None)
    check(lib().pcreg_dev_model_search_f32(pm.handle, _p(q), Q, Q, C.c_int32(0), _p(idx), _p(dist), _p(ws),
                                           C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes), _stream()))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _crop(model, Q, centre, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    d2 = ((model - centre) ** 2).sum(axis=1)
    sel = np.sort(np.argpartition(d2, Q - 1)[:Q])
    return (model[sel] + rng.normal(0, noise, (Q, 3))).astype(np.float32)


_FAM = {}


def _family(name):
    if name in _FAM:
        return _FAM[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + 70)
    if name == "bench":
        from bench import synth
        model, surf, _ = synth(1_000_000, 50_000)
    elif name == "scattered":
        model = (rng.random((1_000_000, 3)) * BOX).astype(np.float32)
        surf = (rng.random((12_000, 3)) * BOX).astype(np.float32)
    elif name in ("rod", "sheet", "duplicates"):
        if name == "rod":
            model = (rng.random((120_000, 3)) * [1000.0, 2.0, 1.0]).astype(np.float32)
        elif name == "sheet":
            model = (rng.random((120_000, 3)) * [80.0, 60.0, 0.0] + [0.0, 0.0, 3.0]).astype(np.float32)
        else:                                              # every row three times, far apart in row order and in tiles
            base = (rng.random((40_000, 3)) * BOX).astype(np.float32)
            model = np.vstack([base, base[::-1], base])
        q = model[rng.choice(len(model), 6000, replace=False)]
        surf = np.vstack([q + rng.normal(0, 0.05, q.shape), q[:1500]]).astype(np.float32)
    elif name == "equal":
        model = np.tile(np.array([[1.5, -2.25, 7.0]], np.float32), (20_000, 1))
        surf = np.vstack([model[:3], (rng.random((3000, 3)) * 10).astype(np.float32)])
    elif name == "outside":
        model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
        crop = _crop(model, 6000, BOX * 0.3, 13)
        near = (rng.random((2000, 3)) * 20 + [105.0, 20.0, 30.0]).astype(np.float32)
        far = crop[:800] + np.float32(5e3)
        huge = crop[800:1000].copy()
        huge[:, 1] = np.float32(-7e8)
        surf = np.vstack([crop, near, far, huge]).astype(np.float32)
        surf = surf[rng.permutation(len(surf))]
    else:
        raise ValueError(name)
    _FAM[name] = (model, surf)
    return model, surf


def _check_ref(model, surf, idx, dist, k, sample=None):
    sel = np.arange(len(surf)) if sample is None or len(surf) <= sample else np.sort(np.random.default_rng(3).choice(len(surf), sample, replace=False))
    ri, rd = ref.knn(surf[sel], model, k, threads=CORES)
    np.testing.assert_array_equal(idx[sel], ri)
    np.testing.assert_array_equal(_bits(dist[sel]), _bits(rd))


FAMILIES = ["bench", "scattered", "rod", "sheet", "equal", "duplicates"]


@pytest.mark.parametrize("name", FAMILIES)
def test_k1_and_k2_equal_the_top2_search(name):
    model, surf = _family(name)
    pm, _t = _prepared(model)
    try:
        i2, d2 = _top2(pm, surf)
        for k in (1, 2):
            ik, dk = _knn(pm, surf, k)
            assert ik.shape == (len(surf), k)
            np.testing.assert_array_equal(ik, i2[:, :k])
            np.testing.assert_array_equal(_bits(dk), _bits(d2[:, :k]))
    finally:
        pm.close()


@pytest.mark.parametrize("name", FAMILIES + ["outside"])
def test_larger_k_equal_the_reference_and_culling_off(name, debug_set):
    model, surf = _family(name)
    pm, _t = _prepared(model)
    try:
        for k in (3, 8, 17, 32):
            idx, dist = _knn(pm, surf, k)
            _check_ref(model, surf, idx, dist, k, sample=2000 if len(model) >= 1_000_000 else None)
            debug_set("knn_nocull", 1)
            i0, d0 = _knn(pm, surf, k)
            debug_set("knn_nocull", 0)
            np.testing.assert_array_equal(i0, idx)
            np.testing.assert_array_equal(_bits(d0), _bits(dist))
    finally:
        pm.close()


@pytest.mark.parametrize("k", [3, 8, 17, 32])
def test_small_models_and_query_counts(k):
    rng = np.random.default_rng(k)
    for M in (0, 1, k - 1, k, 511, 513, 100_003):
        model = (rng.random((M, 3)) * BOX).astype(np.float32)
        pm, _t = _prepared(model)
        try:
            for Q in (0, 1, 513):
                surf = (rng.random((Q, 3)) * BOX * 1.2 - 5.0).astype(np.float32)
                idx, dist = _knn(pm, surf, k)
                assert idx.shape == (Q, k) and dist.shape == (Q, k)
                _check_ref(model, surf, idx, dist, k)
                if M < k and Q:
                    assert np.all(idx[:, M:] == -1) and np.all(np.isposinf(dist[:, M:]))
        finally:
            pm.close()


@pytest.mark.parametrize("scale", [1e-20, 1e19])
def test_extreme_scales(scale):
    """A model with coordinates up to `scale`: at 1e-20 the squared distances are subnormal; at 1e19 every distance of the queries
    more than 2e19 outside the box overflows to +inf (then ordered by row, as the brute force does)."""
    rng = np.random.default_rng(int(np.log10(scale)) + 40)
    ext = (BOX / BOX.max() * scale).astype(np.float64)
    model = (rng.random((60_000, 3)) * ext).astype(np.float32)
    surf = np.vstack([_crop(model, 3000, model[0], 5, noise=0.003 * scale), (rng.random((500, 3)) * 2.5 - 1.0) * ext, (rng.random((500, 3)) * 0.5 - 2.5) * ext]).astype(np.float32)
    pm, _t = _prepared(model)
    try:
        for k in (2, 8, 32):
            idx, dist = _knn(pm, surf, k)
            _check_ref(model, surf, idx, dist, k)
            if scale > 1:
                assert np.isposinf(dist).any() and np.isfinite(dist).any(), "premise: some squared distances overflow"
            else:
                assert (dist[np.isfinite(dist)] < np.finfo(np.float32).tiny).mean() > 0.5, "premise: mostly subnormal distances"
    finally:
        pm.close()


def test_rank_sensitive_culling(debug_set):
    """Two model points sit next to the query, neighbours 3 to 8 in another tile 6.5 away.  The tile's box comes within 0.5 of
    the query, far more than the rank-2 bound (~1e-6): a search seeded with it would skip the tile and miss them.  The ordering
    grid has cells of 400 / 64 = 6.25, so the pair shares cell 0 with nothing, 600 rows at x, y in [9, 12.5] fill cell 3 (tile 0
    and part of tile 1) and the six neighbours sit in cell 4 (iz = 1), behind them in Morton order."""
    rng = np.random.default_rng(8)
    pair = np.array([[1e-3, 0, 0], [0, 1e-3, 0]], np.float32)
    filler = np.column_stack([rng.uniform(9, 12.4, 600), rng.uniform(9, 12.4, 600), rng.uniform(0, 1, 600)]).astype(np.float32)
    six = (np.array([0.5, 0.5, 6.5]) + rng.uniform(-0.1, 0.1, (6, 3))).astype(np.float32)
    corner = np.array([[400, 400, 400]], np.float32)
    model = np.vstack([corner, six, filler, pair]).astype(np.float32)
    surf = np.array([[1e-3, 1e-3, 1e-3]], np.float32)
    pm, _t = _prepared(model)
    try:
        debug_set("knn_stats", 1)
        _stats(reset=True)
        idx, dist = _knn(pm, surf, 8)
        st = _stats(reset=True)
        assert sorted(idx[0, :2].tolist()) == [len(model) - 2, len(model) - 1]
        assert sorted(idx[0, 2:].tolist()) == list(range(1, 7))
        _check_ref(model, surf, idx, dist, 8)
        assert st[0] == 1 and st[2] == 2 and st[1] == 2, st        # premise: both tiles visited (rows 0..511, 512..608)
        i2, _ = _knn(pm, surf, 2)
        assert sorted(i2[0].tolist()) == [len(model) - 2, len(model) - 1]
    finally:
        pm.close()


def test_culling_is_real_at_the_bench_shape(debug_set):
    model, surf = _family("bench")
    pm, _t = _prepared(model)
    try:
        debug_set("knn_stats", 1)
        _stats(reset=True)
        idx, dist = _knn(pm, surf, 8)
        st = _stats(reset=True)
        nb, nt = (len(surf) + 511) // 512, (len(model) + 511) // 512
        assert st[0] == 1 and st[2] == nb * nt and st[3] == 0
        share = st[1] / st[2]
        print(f"bench crop, k = 8: visited {st[1]} of {st[2]} (block, tile) pairs = {share:.4f}")
        assert share < 0.25
        debug_set("knn_nocull", 1)
        i0, d0 = _knn(pm, surf, 8)
        st0 = _stats(reset=True)
        assert st0[1] == st0[2] == st[2]
        np.testing.assert_array_equal(i0, idx)
        np.testing.assert_array_equal(_bits(d0), _bits(dist))
    finally:
        pm.close()


def test_three_shards_merge_to_the_whole():
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import PreparedModel
    model, surf = _family("scattered")
    surf = np.vstack([surf[:4000], _family("bench")[1][:4000]])
    M, Q, k = len(model), len(surf), 8
    t = _soa(model)
    whole = PreparedModel(t)
    cuts = [0, 333_331, 700_000, M]
    shards = [PreparedModel(t[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    try:
        ri, rd = _knn(whole, surf, k)
        q = _soa(surf)
        buf_i = torch.empty((3, Q, k), dtype=torch.int32, device=_dev())
        buf_d = torch.empty((3, Q, k), dtype=torch.float32, device=_dev())
        for r, (pm, a) in enumerate(zip(shards, cuts)):
            i, d = pm.knn(q, k, idx_base=a)
            buf_i[r].copy_(i); buf_d[r].copy_(d)
        oi = torch.empty((Q, k), dtype=torch.int32, device=_dev())
        od = torch.empty((Q, k), dtype=torch.float32, device=_dev())
        check(lib().pcreg_dev_merge_topk_f32(_p(buf_i), _p(buf_d), 3, Q, k, C.c_size_t(0), _p(oi), _p(od), _stream()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(oi.cpu().numpy(), ri)
        np.testing.assert_array_equal(_bits(od.cpu().numpy()), _bits(rd))
        # strided form: one buffer with a rank stride larger than Q * k
        big_i = torch.full((3, Q * k + 40), -7, dtype=torch.int32, device=_dev())
        big_d = torch.zeros((3, Q * k + 40), dtype=torch.float32, device=_dev())
        big_i[:, :Q * k].copy_(buf_i.view(3, -1)); big_d[:, :Q * k].copy_(buf_d.view(3, -1))
        check(lib().pcreg_dev_merge_topk_f32(_p(big_i), _p(big_d), 3, Q, k, C.c_size_t(Q * k + 40), _p(oi), _p(od), _stream()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(oi.cpu().numpy(), ri)
    finally:
        whole.close()
        for pm in shards:
            pm.close()


def test_host_tiers_and_two_streams_equal_the_device_tier():
    import pcreg_amd as pc
    from pcreg_amd._lib import lib
    model, surf = _family("rod")
    pm, _t = _prepared(model)
    try:
        for k in (1, 5, 32):
            di, dd = _knn(pm, surf, k)
            with pc.Model(model) as h:
                hi, hd = h.knn(surf, k)
            oi, od = pc.knn_points(surf, model, k)
            for i, d in ((hi, hd), (oi, od)):
                np.testing.assert_array_equal(i, di)
                np.testing.assert_array_equal(_bits(d), _bits(dd))
        # two streams on one handle, each call with its own workspace
        k = 8
        a, b = surf[:4000], surf[3000:]
        ra, rb = _knn(pm, a, k), _knn(pm, b, k)
        qa, qb = _soa(a), _soa(b)
        outs = []
        for q in (qa, qb):
            Q = q.shape[1]
            ws = torch.empty(int(lib().pcreg_dev_model_knn_workspace(Q, pm.M, k)), dtype=torch.uint8, device=_dev())
            outs.append((torch.empty((Q, k), dtype=torch.int32, device=_dev()), torch.empty((Q, k), dtype=torch.float32, device=_dev()), ws))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            with torch.cuda.stream(s1):
                pm.knn(qa, k, out=outs[0])
            with torch.cuda.stream(s2):
                pm.knn(qb, k, out=outs[1])
        torch.cuda.synchronize()
        for (i, d, _), (ri, rd) in zip(outs, (ra, rb)):
            np.testing.assert_array_equal(i.cpu().numpy(), ri)
            np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(rd))
    finally:
        pm.close()
