"""clusterPoints against a prepared model (knn_cluster.hip) on the GPU, bit for bit.

label, n_clusters, first and sizes of the device tier, and cl_off / members of the host tiers, against the fp32 reference
(tests/cluster_ref.c); every case again with culling off ("knn_nocull") and with the "same root" early-out off
("cluster_noskip").  Families, chains across tiles, the edges (M, r2 = 0, r2 = +inf, non-finite rows, scale), determinism,
the culling rule restated in float64 on the exported tile boxes, the 32u window, the frontier loop over Model.rangesearch, the
host tiers, two streams on one handle and the MEX commands."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import cluster_ref as ref
import knn_cull_ref

pytestmark = pytest.mark.gpu
BOX = np.array([101.0, 56.0, 99.0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


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


def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def _prepared(model):
    from pcreg_amd.device import PreparedModel
    t = _soa(model)
    return PreparedModel(t), t


def _cluster(pm, r2):
    """-> label [M], n_clusters, first [M], sizes [M] as numpy"""
    label, nc, first, sizes = pm.cluster(r2)
    torch.cuda.synchronize()
    return label.cpu().numpy(), int(nc.item()), first.cpu().numpy(), sizes.cpu().numpy()


def _equal_ref(got, want, what=""):
    label, nc, first, sizes = got
    rl, ro, rm = want
    rf, rs = ref.first_and_sizes(rl, ro, rm)
    assert label.dtype == np.int32 and first.dtype == np.int32 and sizes.dtype == np.int32
    assert nc == len(ro) - 1, (what, nc, len(ro) - 1)
    np.testing.assert_array_equal(label, rl, err_msg=what)
    np.testing.assert_array_equal(first[:nc], rf, err_msg=what)
    np.testing.assert_array_equal(sizes[:nc], rs, err_msg=what)
    assert not first[nc:].any() and not sizes[nc:].any(), what      # zeros at and past n_clusters


def _check(model, r2, debug_set, pm=None, want=None):
    """the device tier equals the reference: as it is, with culling off, and with the early-out off; -> the reference result"""
    own = pm is None
    if own:
        pm, _t = _prepared(model)
    try:
        want = ref.cluster(model, r2) if want is None else want
        _equal_ref(_cluster(pm, r2), want, f"r2 = {float(r2)!r}")
        debug_set("knn_nocull", 1)
        _equal_ref(_cluster(pm, r2), want, f"r2 = {float(r2)!r}, knn_nocull")
        debug_set("knn_nocull", 0)
        debug_set("cluster_noskip", 1)
        _equal_ref(_cluster(pm, r2), want, f"r2 = {float(r2)!r}, cluster_noskip")
        debug_set("cluster_noskip", 0)
    finally:
        if own:
            pm.close()
    return want


_FAM = {}


def _family(name):
    """the clouds of tests/test_gpu_range.py's families (same generators and seeds; here only the model side matters)"""
    if name in _FAM:
        return _FAM[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + 70)
    if name == "bench":
        from bench import synth
        model = synth(1_000_000, 50_000)[0]
    elif name == "rod":
        model = (rng.random((120_000, 3)) * [1000.0, 2.0, 1.0]).astype(np.float32)
    elif name == "sheet":
        model = (rng.random((120_000, 3)) * [80.0, 60.0, 0.0] + [0.0, 0.0, 3.0]).astype(np.float32)
    elif name == "duplicates":                             # every row three times, far apart in row order and in tiles
        base = (rng.random((40_000, 3)) * BOX).astype(np.float32)
        model = np.vstack([base, base[::-1], base])
    elif name == "equal":                                  # 20 000 coincident rows and 200 scattered ones
        model = np.vstack([np.tile(np.array([[1.5, -2.25, 7.0]], np.float32), (20_000, 1)), (rng.random((200, 3)) * 10).astype(np.float32)])
        model = model[rng.permutation(len(model))]
    elif name == "outside":                                # a dense box, a group nearby, a far group, rows 7e8 away on one axis
        box = (rng.random((60_000, 3)) * BOX * 0.3).astype(np.float32)
        near = (rng.random((2000, 3)) * 20 + [105.0, 20.0, 30.0]).astype(np.float32)
        far = box[:800] + np.float32(5e3)
        huge = box[800:1000].copy()
        huge[:, 1] = np.float32(-7e8)
        model = np.vstack([box, near, far, huge]).astype(np.float32)
        model = model[rng.permutation(len(model))]
    else:
        raise ValueError(name)
    _FAM[name] = np.ascontiguousarray(model, np.float32)
    return _FAM[name]


# radii (not squared) per family: around the mean spacing of each cloud, so that the partitions run from mostly singletons to a
# few large clusters; 0 for the clouds with coincident rows
RADII = {"rod": (0.1, 0.2, 0.4), "sheet": (0.1, 0.2, 0.35), "duplicates": (0.0, 1.0, 2.5), "equal": (0.0, 0.5, 1.5), "outside": (0.3, 0.6, 30.0)}


def test_bench_model_equals_the_reference(debug_set):
    model = _family("bench")
    pm, _t = _prepared(model)
    try:
        for r in (0.7, 0.75, 1.0, 1.5):
            r2 = np.float32(r) ** 2
            label, off, members = _check(model, r2, debug_set, pm=pm)
            sizes = np.diff(off)
            print(f"bench model, r = {r}: {len(sizes)} clusters, the largest has {int(sizes.max())} rows")
            if r == 0.75:                                   # premise: just above the percolation threshold
                assert len(sizes) > 1000 and sizes.max() > 500_000
            if r == 1.5:
                assert len(sizes) == 1
    finally:
        pm.close()


@pytest.mark.parametrize("name", ["rod", "sheet", "duplicates", "equal", "outside"])
def test_families_equal_the_reference(name, debug_set):
    model = _family(name)
    pm, _t = _prepared(model)
    seen = []
    try:
        for r in RADII[name]:
            label, off, members = _check(model, np.float32(r) ** 2, debug_set, pm=pm)
            sizes = np.diff(off)
            seen.append((len(sizes), int(sizes.max())))
            print(f"{name}: r = {r}: {len(sizes)} clusters, the largest has {int(sizes.max())} rows")
        assert len(set(seen)) == len(seen), seen               # premise: the radii give different partitions
        if name in ("duplicates", "equal"):                    # r2 = 0: the sets of coincident rows
            assert seen[0] == ((40_000, 3) if name == "duplicates" else (201, 20_000)), seen
    finally:
        pm.close()


def _line(offset, gap):
    """5000 rows on a line along x with spacing exactly 1.0 in fp32, optionally with ONE spacing that is the next fp32 number
    above 1.0 at those coordinates; -> rows (shuffled), the largest and smallest fp32 spacing"""
    if offset == 0.0:
        # the gap sits at the origin, where 1 + 2^-23 exists: .., -2, -1, 0 | 1 + 2^-23, 2, 3, ..  (2 - (1 + 2^-23) < 1)
        x = np.concatenate([-np.arange(2500, dtype=np.float32)[::-1], np.arange(1, 2501, dtype=np.float32)])
        if gap:
            x[2500] = np.nextafter(np.float32(1), np.float32(2))
    else:
        x = (np.float32(offset) + np.arange(5000, dtype=np.float32)).astype(np.float32)
        if gap:                                                # one ulp up from row 2500 on: the spacing behind it stays 1.0
            x[2500:] = np.nextafter(x[2500:], np.float32(np.inf))
    d = np.diff(x)
    pts = np.zeros((5000, 3), np.float32)
    pts[:, 0] = x
    pts[:, 1] = np.float32(offset)
    return pts[np.random.default_rng(5).permutation(5000)], float(d.max()), float(d.min())


@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_chains_across_tiles(offset, debug_set):
    pts, dmax, dmin = _line(offset, gap=False)
    assert dmax == 1.0 and dmin == 1.0
    label, off, members = _check(pts, 1.0, debug_set)
    assert len(off) - 1 == 1
    pts, dmax, dmin = _line(offset, gap=True)
    assert dmax > 1.0 and np.float32(dmax) * np.float32(dmax) > 1.0 and dmin > 0.99
    label, off, members = _check(pts, 1.0, debug_set)
    assert np.diff(off).tolist() == [2500, 2500]


def test_small_models(debug_set):
    rng = np.random.default_rng(12)
    for M in (0, 1, 2, 37, 511, 512, 513, 9000):               # (9000: a model without the seeding grid)
        model = (rng.random((M, 3)) * 10).astype(np.float32)
        for r2 in (0.0, 0.3, 4.0, 1e4, np.inf):
            label, off, members = _check(model, r2, debug_set)
            assert len(label) == M
            if M == 0 or r2 == 0.0 or r2 >= 1e4:               # no row; distinct rows; the whole box within the radius
                assert len(off) - 1 == (0 if M == 0 else M if r2 == 0.0 else 1)


def test_non_finite_rows_are_singletons(debug_set):
    rng = np.random.default_rng(31)
    model = (rng.random((30_000, 3)) * 20).astype(np.float32)
    bad = np.sort(rng.choice(30_000, 40, replace=False))
    for k, i in enumerate(bad):
        model[i] = [[np.nan, 1, 1], [np.inf, 1, 1], [3, -np.inf, 1], [np.nan, np.inf, -np.inf], [np.inf, np.inf, np.inf]][k % 5]
    model[bad[5]] = model[bad[10]] = [np.inf, 2.0, 3.0]         # coincident twins
    for r2 in (0.16, 1.0, 1e4, np.inf):
        label, off, members = _check(model, r2, debug_set)
        sizes = np.diff(off)
        assert np.all(sizes[label[bad]] == 1)
        if r2 >= 1e4:                                           # all finite rows are one cluster
            assert len(sizes) == 41 and sizes.max() == 30_000 - 40


@pytest.mark.parametrize("scale", [1e-18, 1e18])
def test_extreme_scales(scale, debug_set):
    """a jittered part of a lattice of spacing `scale`: the squared distances are near the bottom / the top of fp32's range"""
    rng = np.random.default_rng(44)
    g = np.stack(np.meshgrid(*[np.arange(30)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:9000]]
    model = ((g + rng.uniform(-0.05, 0.05, g.shape)) * scale).astype(np.float32)
    seen = set()
    for f in (0.8, 1.2, 1.6):
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(f * scale) * np.float32(f * scale)
        assert 0 < r2 < np.inf
        label, off, members = _check(model, r2, debug_set)
        seen.add(len(off) - 1)
    assert len(seen) == 3 and max(seen) > 1000, seen
    label, off, members = _check(model, np.inf, debug_set)
    assert len(off) - 1 == 1


def _renumber(label):
    """the numbering rule applied to any labelling: clusters in ascending order of their first row"""
    _, first_at, inv = np.unique(label, return_index=True, return_inverse=True)
    rank = np.empty(len(first_at), np.int64)
    rank[np.argsort(first_at)] = np.arange(len(first_at))
    return rank[inv].astype(np.int32)


def test_determinism_and_row_permutations():
    model = _family("bench")[:300_000]
    r2 = np.float32(0.9) ** 2
    outs = []
    for _ in range(2):
        pm, _t = _prepared(model)
        try:
            outs += [_cluster(pm, r2), _cluster(pm, r2)]
        finally:
            pm.close()
    for o in outs[1:]:
        assert o[1] == outs[0][1]
        for a, b in zip((o[0], o[2], o[3]), (outs[0][0], outs[0][2], outs[0][3])):
            np.testing.assert_array_equal(a, b)
    assert 100 < outs[0][1] < len(model)
    order = np.random.default_rng(9).permutation(len(model))
    pm, _t = _prepared(model[order])
    try:
        got = _cluster(pm, r2)
    finally:
        pm.close()
    np.testing.assert_array_equal(got[0], _renumber(outs[0][0][order]))
    _equal_ref(got, ref.cluster(model[order], r2))


def _export(pm):
    from pcreg_amd._lib import check, lib
    nt = (pm.M + 511) // 512
    tb = torch.empty(max(6 * nt, 1), dtype=torch.float32, device=_dev())
    perm = torch.empty(max(pm.M, 1), dtype=torch.int32, device=_dev())
    prep = (C.c_float * 24)()
    check(lib().pcreg_debug_dev_model_export(pm.handle, _p(perm), None, _p(tb), prep, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return perm.cpu().numpy()[:pm.M].copy(), tb.cpu().numpy()[:6 * nt].reshape(nt, 6).copy()


def _visited_pairs(tbox, r2):
    """DESIGN 4.1's rule with D = r2 on the tile boxes, in float64: the (a, b >= a) pairs the walk must visit"""
    n = len(tbox)
    if not np.float32(r2) < np.inf:
        return n * (n + 1) // 2
    total = 0
    for a0 in range(0, n, 256):
        G2 = knn_cull_ref.gap2(tbox[a0:a0 + 256, :3], tbox[a0:a0 + 256, 3:], tbox)
        vis = ~knn_cull_ref.skip(G2, np.full(G2.shape[0], float(np.float32(r2))))
        total += int(np.triu(vis, k=a0).sum())
    return total


def test_culling_follows_the_rule_on_the_exported_boxes(debug_set):
    debug_set("knn_stats", 1)
    for name, radii in (("bench", (0.5, 1.0, 4.0)), ("rod", (0.2,)), ("outside", (0.6, 30.0))):
        model = _family(name)
        pm, _t = _prepared(model)
        try:
            _, tbox = _export(pm)
            n = len(tbox)
            for r in radii:
                r2 = np.float32(r) ** 2
                _stats(reset=True)
                pm.cluster(r2)
                st = _stats(reset=True)
                assert st[0] == 1 and st[2] == n * (n + 1) // 2, st
                assert st[1] == _visited_pairs(tbox, r2), (name, r, st)
                print(f"{name}, r = {r}: visited {st[1]} of {st[2]} (tile, tile) pairs = {st[1] / st[2]:.4f}")
                if name == "bench" and r == 1.0:
                    assert st[1] / st[2] < 0.05
            debug_set("knn_nocull", 1)
            pm.cluster(r2)
            st = _stats(reset=True)
            debug_set("knn_nocull", 0)
            assert st[1] == st[2] == n * (n + 1) // 2, st
            pm.cluster(np.inf)
            st = _stats(reset=True)
            assert st[1] == st[2], st                          # r2 = +inf: nothing is culled
        finally:
            pm.close()


def test_the_32u_window(debug_set):
    """Tile 0 is 512 rows with x <= 0.75, tile 1 begins at x = b in the next cell of the ordering grid; the boxes overlap in y and
    z, so G2 = (b - 0.75)^2.  b is chosen so that g = b - 0.75 is exact in fp32 and fl(g * g) < g^2: with r2 = fl(g * g) the rows
    (0.75, .5, .5) and (b, .5, .5) are adjacent although G2 > r2, and only the 32u margin keeps the pair of tiles."""
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
    assert model[ia].tolist() == [0.75, 0.5, 0.5] and model[ib, 0] == b
    pm, _t = _prepared(model)
    try:
        perm, tbox = _export(pm)
        tile_of = knn_cull_ref.row_tiles(perm)
        assert tile_of[ia] == 0 and tile_of[ib] == 1 and tbox[0, 3] == np.float32(0.75) and tbox[1, 0] == b, "premise: the two tiles"
        G2 = float(knn_cull_ref.gap2(tbox[:1, :3], tbox[:1, 3:], tbox[1:2])[0, 0])
        assert G2 == float(g) ** 2 and G2 > float(r2) >= G2 * (1.0 - 32.0 * U), "premise: the window"
        label, off, members = _check(model, r2, debug_set, pm=pm)
        assert label[ia] == label[ib]
    finally:
        pm.close()


# ---- the parent's own way: clusterPoints.m's frontier loop over Model.rangesearch -------------------------------------------
def _cluster_frontier(pts, r):
    """the frontier loop, one rangesearch per frontier, 0-based"""
    import pcreg_amd as pc
    n = len(pts)
    r2 = np.float32(r) * np.float32(r)
    clusters, unexplored = [], np.ones(n, bool)
    with pc.Model(pts) as h:
        while unexplored.any():
            frontier = np.array([int(np.argmax(unexplored))])
            unexplored[frontier] = False
            explored = np.zeros(0, np.int64)
            while len(frontier):
                _, idx, _ = h.rangesearch(pts[frontier], r2)
                explored = np.union1d(explored, frontier)
                frontier = np.setdiff1d(np.unique(idx), explored)
                unexplored[frontier] = False
            clusters.append(explored.tolist())
    return clusters


def _as_lists(off, members):
    return [members[off[c]:off[c + 1]].tolist() for c in range(len(off) - 1)]


@pytest.mark.parametrize("n_grid, keep, seed", [(8, 0.25, 1), (10, 0.2, 2), (40, 0.3125, 3)])
def test_the_frontier_loop_gives_the_same_clusters(n_grid, keep, seed):
    """sphere-centre-like input: a jittered subset of a grid of spacing d, r = 1.6 d"""
    import pcreg_amd as pc
    rng = np.random.default_rng(seed)
    d = 2.5
    g = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:int(round(keep * len(g)))]]
    pts = ((g + rng.uniform(-0.03, 0.03, g.shape)) * d).astype(np.float32)
    r = 1.6 * d
    label, off, members = pc.cluster_points(pts, np.float32(r) * np.float32(r))
    want = _cluster_frontier(pts, r)
    assert len(want) > 1 and max(len(c) for c in want) > 10
    assert _as_lists(off, members) == want


def test_the_frontier_loop_on_a_subsample_of_the_bench_model():
    import pcreg_amd as pc
    model = _family("bench")
    pts = np.ascontiguousarray(model[np.sort(np.random.default_rng(17).choice(len(model), 100_000, replace=False))])
    import time
    pc.cluster_points(pts[:1000], 1.0)                            # (the first call of a process pays for the library's start)
    t0 = time.perf_counter()
    label, off, members = pc.cluster_points(pts, np.float32(2.0) * np.float32(2.0))
    t1 = time.perf_counter()
    want = _cluster_frontier(pts, 2.0)
    t2 = time.perf_counter()
    assert _as_lists(off, members) == want
    assert np.diff(off).max() > 50_000
    print(f"100 000 rows, r = 2: cluster_points {1e3 * (t1 - t0):.1f} ms (upload and preparation included), the frontier loop {1e3 * (t2 - t1):.1f} ms")
    assert t1 - t0 < t2 - t1, "the one call is faster than the loop of searches it replaces"


# ---- layers -----------------------------------------------------------------------------------------------------------------
def test_host_tiers_equal_the_device_tier():
    import pcreg_amd as pc
    for name, r in (("rod", 0.2), ("duplicates", 0.0), ("outside", 0.6)):
        model = _family(name)
        r2 = np.float32(r) ** 2
        want = ref.cluster(model, r2)
        pm, _t = _prepared(model)
        try:
            _equal_ref(_cluster(pm, r2), want)
        finally:
            pm.close()
        with pc.Model(model) as h:
            a = h.cluster(r2)
        b = pc.cluster_points(model, r2)
        for label, off, members in (a, b):
            assert label.dtype == off.dtype == members.dtype == np.int32
            np.testing.assert_array_equal(label, want[0])
            np.testing.assert_array_equal(off, want[1])
            np.testing.assert_array_equal(members, want[2])
    # label alone: cl_off / members may both be NULL
    from pcreg_amd._lib import check, lib
    mf = np.asfortranarray(model)
    label = np.full(len(model), -1, np.int32)
    nc = C.c_int32(-1)
    check(lib().pcreg_cluster_points_f32(mf.ctypes.data, len(model), len(model), float(r2), label.ctypes.data, C.byref(nc), None, None))
    np.testing.assert_array_equal(label, want[0])
    assert nc.value == len(want[1]) - 1
    assert pc.cluster_points(np.zeros((0, 3)), 1.0)[1].tolist() == [0]


def test_two_streams_on_one_handle():
    from pcreg_amd._lib import lib
    model = _family("rod")
    pm, _t = _prepared(model)
    try:
        radii = (np.float32(0.15) ** 2, np.float32(0.3) ** 2)
        serial = [_cluster(pm, r2) for r2 in radii]
        M = pm.M
        need = int(lib().pcreg_dev_model_cluster_workspace(M))
        outs = [tuple(torch.full((n,), -1, dtype=torch.int32, device=_dev()) for n in (M, 1, M, M)) + (torch.empty(need, dtype=torch.uint8, device=_dev()),)
                for _ in radii]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, r2, o in ((s1, radii[0], outs[0]), (s2, radii[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.cluster(r2, out=o)
        torch.cuda.synchronize()
        for o, want in zip(outs, serial):
            np.testing.assert_array_equal(o[0].cpu().numpy(), want[0])
            assert int(o[1].item()) == want[1]
            np.testing.assert_array_equal(o[2].cpu().numpy(), want[2])
            np.testing.assert_array_equal(o[3].cpu().numpy(), want[3])
        assert serial[0][1] != serial[1][1]
    finally:
        pm.close()


def test_cluster_stats_count_the_unions(debug_set):
    """"cluster_stats": hits, compare-and-swap attempts and failures; every successful attempt removes one set"""
    from pcreg_amd._lib import check, lib
    model = _family("sheet")
    pm, _t = _prepared(model)
    try:
        debug_set("cluster_stats", 1)
        out = (C.c_longlong * 4)()
        check(lib().pcreg_debug_cluster_stats(out, 1))
        label, nc, first, sizes = _cluster(pm, np.float32(0.2) ** 2)
        check(lib().pcreg_debug_cluster_stats(out, 1))
        calls, hits, cas, failed = (int(v) for v in out)
        print(f"sheet, r = 0.2: {hits} hits, {cas} compare-and-swaps, {failed} failed")
        assert calls == 1 and hits >= cas - failed and cas - failed == len(model) - nc
    finally:
        pm.close()


@pytest.fixture(scope="module")
def mexdrv(tmp_path_factory):
    import subprocess
    out = str(tmp_path_factory.mktemp("mexcluster") / "libmexcluster.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexcluster", "cluster_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    drv = C.CDLL(out)
    drv.cd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_char_p, C.c_int]
    return drv


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, r", [(3000, 0.9), (5, 40.0), (0, 1.0), (3000, 0.0)])
def test_mex_round_trip_equals_the_host_tier(mexdrv, via_handle, M, r):
    """[label, clOff, members] = pcreg_mex('modelCluster', h, r) / pcreg_mex('clusterPoints', single(pts), r) through
    tests/mexcluster/cluster_driver.cpp: 1-based rows and labels, r squared once in single"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + 3)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    want = pc.cluster_points(m, np.float32(r) * np.float32(r))
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    label = np.full(max(M, 1), -7, np.int32); off = np.full(M + 1, -7, np.int32); members = np.full(max(M, 1), -7, np.int32)
    e = C.create_string_buffer(1024); nc = C.c_int(-1)
    assert mexdrv.cd_round_trip(via_handle, mf.ctypes.data, M, float(r), label.ctypes.data, off.ctypes.data, C.byref(nc), members.ctypes.data,
                                e, 1024) == 0, e.value
    assert mexdrv.cd_live_arrays() == 0
    assert nc.value == len(want[1]) - 1
    np.testing.assert_array_equal(label[:M], want[0] + 1)
    np.testing.assert_array_equal(off[:nc.value + 1], want[1])
    np.testing.assert_array_equal(members[:M], want[2] + 1)
