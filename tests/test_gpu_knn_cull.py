"""Tile culling of the point search (knn_mfma16.hip) checked against the float64 host reference of the rule.

test_gpu_spatial_order.py compares results only: it stays green if the rule culls nothing, or less than it should, and the
exhaustive tail hides a tile that was culled wrongly whenever the certificate happens to fail.  Here the library's test
hooks expose what the search did -- the prepared model (perm, sorted copy, tile boxes, preparation record), the call's query
order and seed distances, and the visited (query block, tile) pairs ("knn_stats") -- and every test compares them with
tests/knn_cull_ref.py or numpy: the visited count exactly, the answers' tiles inside their block's visited set, culling off
("knn_nocull") giving the same bits, constructed cases on the boundary of the rule, launch shapes with several tile rounds,
and models so small that sigma^2 leaves fp32."""
import ctypes as C
import itertools
import os
import zlib

import numpy as np
import pytest
import torch

import knn_cull_ref as ref

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
BOX = np.array([101.0, 56.0, 99.0])
U = 2.0 ** -24


def _dev():
    return torch.device("cuda", 0)


def _soa(x):
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T)))
    return t


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


class Model:
    """A prepared model and what it exports."""

    def __init__(self, model):
        from pcreg_amd._lib import check, lib
        from pcreg_amd.device import PreparedModel
        self.points = np.asarray(model, np.float32)
        self.M = len(self.points)
        self.t = _soa(self.points)
        self.pm = PreparedModel(self.t)
        nt = (self.M + ref.TILE - 1) // ref.TILE
        perm = torch.empty(max(self.M, 1), dtype=torch.int32, device=_dev())
        ms = torch.empty(max(3 * self.M, 1), dtype=torch.float32, device=_dev())
        tb = torch.empty(max(6 * nt, 1), dtype=torch.float32, device=_dev())
        prep = (C.c_float * 24)()
        check(lib().pcreg_debug_dev_model_export(self.pm.handle, _p(perm), _p(ms), _p(tb), prep, _stream()))
        torch.cuda.synchronize()
        self.perm = perm.cpu().numpy()[:self.M].copy()
        self.ms = ms.cpu().numpy()[:3 * self.M].reshape(3, self.M).T.copy()
        self.tbox = tb.cpu().numpy()[:6 * nt].reshape(nt, 6).copy()
        self.prep = np.frombuffer(bytes(prep), np.float32).copy()
        self.n_tiles = nt

    def search(self, surf, nocull=False, debug_set=None):
        """(idx, dist, qperm, dk, stats) of one search call on this model"""
        from pcreg_amd._lib import check, lib
        from pcreg_amd.device import HipOps
        surf = np.asarray(surf, np.float32)
        Q = len(surf)
        ops = HipOps(Q, max(self.M, 1), _dev())
        if debug_set is not None:
            debug_set("knn_nocull", 1 if nocull else 0)
        torch.cuda.synchronize()
        _stats(reset=True)
        idx, dist = ops.local_top2(_soa(surf), self.pm, 0)
        qperm = torch.empty(Q, dtype=torch.int32, device=_dev())
        dk = torch.empty(Q, dtype=torch.float32, device=_dev())
        check(lib().pcreg_debug_search_export(_p(ops.ws), C.c_size_t(ops.ws.numel()), Q, self.M, _p(qperm), _p(dk), _stream()))
        torch.cuda.synchronize()
        st = _stats(reset=True)
        if debug_set is not None and nocull:
            debug_set("knn_nocull", 0)
        return idx.cpu().numpy().copy(), dist.cpu().numpy().copy(), qperm.cpu().numpy().copy(), dk.cpu().numpy().copy(), st

    def close(self):
        self.pm.close()


@pytest.fixture
def stats_on(debug_set):
    debug_set("knn_stats", 1)
    _stats(reset=True)
    return debug_set


# ---- numpy restatements of the ordering grid ------------------------------------------------------------------------
def _spread(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def _sort_keys(x, prep):
    """Morton key of the ordering-grid cell of every point, in float32 from the exported record (words 16-19)"""
    x = np.asarray(x, np.float32)
    s0, inv_s = prep[16:19].astype(np.float32), np.float32(prep[19])
    with np.errstate(invalid="ignore"):
        c = np.floor((x - s0) * inv_s)
    c = np.fmin(np.fmax(c, np.float32(0)), np.float32(63)).astype(np.uint32)
    return _spread(c[:, 0]) | (_spread(c[:, 1]) << np.uint32(1)) | (_spread(c[:, 2]) << np.uint32(2))


def _seed_cells(x, prep):
    """seeding-grid cell of every point (words 8-15), -1 outside the grid"""
    x = np.asarray(x, np.float32)
    g0, ih = prep[8:11].astype(np.float32), np.float32(prep[11])
    n = prep.view(np.int32)[12:15]
    f = np.floor((x - g0) * ih)
    inside = np.all((f >= 0) & (f < n.astype(np.float32)), axis=1)
    f = np.where(inside[:, None], f, 0).astype(np.int64)
    return np.where(inside, (f[:, 2] * n[1] + f[:, 1]) * n[0] + f[:, 0], -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _crop(model, Q, centre, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    d2 = ((model - centre) ** 2).sum(axis=1)
    sel = np.sort(np.argpartition(d2, Q - 1)[:Q])
    return (model[sel] + rng.normal(0, noise, (Q, 3))).astype(np.float32)


# ---- 1. the prepared model ------------------------------------------------------------------------------------------
def _model_kind(kind):
    rng = np.random.default_rng(zlib.crc32(str(kind).encode()) % 1000)
    if isinstance(kind, int):
        return (rng.random((kind, 3)) * BOX).astype(np.float32)
    if kind == "flat":
        return (rng.random((40_000, 3)) * [80.0, 60.0, 0.0] + [0.0, 0.0, 3.0]).astype(np.float32)
    if kind == "rod":
        return (rng.random((40_000, 3)) * [1000.0, 2.0, 1.0]).astype(np.float32)
    if kind == "equal":
        return np.tile(np.array([[1.5, -2.25, 7.0]], np.float32), (20_000, 1))
    if kind == "offset":
        return (rng.random((50_000, 3)) * BOX + [1e4, -3e4, 2e4]).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", [16384, 16385, 512 * 45, 512 * 45 + 1, 100_003, 1_000_000, "flat", "rod", "equal", "offset"])
def test_prepared_model_order_and_tile_boxes(kind):
    model = _model_kind(kind)
    M = len(model)
    pm = Model(model)
    try:
        assert np.array_equal(np.sort(pm.perm), np.arange(M)), "perm is not a permutation"
        np.testing.assert_array_equal(_bits(pm.ms), _bits(model[pm.perm]))
        keys = _sort_keys(pm.ms, pm.prep)
        assert np.all(np.diff(keys.astype(np.int64)) >= 0), "sorted rows are not in Morton order"
        starts = np.arange(0, M, ref.TILE)
        lo = np.minimum.reduceat(pm.ms, starts, axis=0)
        hi = np.maximum.reduceat(pm.ms, starts, axis=0)
        assert pm.n_tiles == len(starts)
        np.testing.assert_array_equal(_bits(pm.tbox[:, :3]), _bits(lo))
        np.testing.assert_array_equal(_bits(pm.tbox[:, 3:]), _bits(hi))
    finally:
        pm.close()


# ---- 2. query order and seed distances ------------------------------------------------------------------------------
def test_query_order_and_seed_distances(stats_on, oracle_c):
    rng = np.random.default_rng(21)
    model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
    crop = _crop(model, 20_000, BOX * 0.4, 22)
    surf = np.vstack([crop, rng.random((2000, 3)) * BOX * 1.2 - 5.0]).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = pm.search(surf)
        assert np.array_equal(np.sort(qperm), np.arange(len(surf)))
        parent = _sort_keys(surf[qperm], pm.prep) >> np.uint32(3)
        assert np.all(np.diff(parent.astype(np.int64)) >= 0), "query slots are not in parent-cell order"
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(dist, rd)
        fin = np.isfinite(dk)
        assert np.all(dk[fin] >= rd[fin, 1]), "a seed distance below the true second distance"
        inside = np.all((crop >= model.min(axis=0)) & (crop <= model.max(axis=0)), axis=1)
        assert inside.sum() > 15_000 and np.all(np.isfinite(dk[:len(crop)][inside]))
    finally:
        pm.close()
    small = model[:9000]
    pm = Model(small)
    try:
        idx, dist, qperm, dk, st = pm.search(surf[:3000])
        assert np.all(dk == np.inf)
        assert st[1] == st[2], "culling with M < kSeedMinM"
    finally:
        pm.close()


# ---- 3. the rule, evaluated exactly ---------------------------------------------------------------------------------
def _family(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + 30)
    if name == "bench":
        from bench import synth
        model, surf, _ = synth(1_000_000, 50_000)
        return model, surf
    if name == "scattered":
        model = (rng.random((150_000, 3)) * BOX).astype(np.float32)
        return model, (rng.random((12_000, 3)) * BOX).astype(np.float32)
    if name in ("rod", "sheet", "duplicates"):
        if name == "rod":
            model = (rng.random((120_000, 3)) * [1000.0, 2.0, 1.0]).astype(np.float32)
        elif name == "sheet":
            model = (rng.random((120_000, 3)) * [80.0, 60.0, 0.0] + [0.0, 0.0, 3.0]).astype(np.float32)
        else:
            base = (rng.random((40_000, 3)) * BOX).astype(np.float32)
            model = np.vstack([base, base[::-1], base])
        q = model[rng.choice(len(model), 8000, replace=False)]
        return model, np.vstack([q + rng.normal(0, 0.05, q.shape), q[:2000]]).astype(np.float32)
    if name == "outside":
        model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
        crop = _crop(model, 8000, BOX * 0.3, 13)
        near = (rng.random((3000, 3)) * 20 + [105.0, 20.0, 30.0]).astype(np.float32)
        far = crop[:1000] + np.float32(5e3)
        huge = crop[1000:1200].copy()
        huge[:, 1] = np.float32(-7e8)                     # not scored
        surf = np.vstack([crop, near, far, huge]).astype(np.float32)
        return model, surf[rng.permutation(len(surf))]
    if name == "blobs":                                   # dense blobs with empty space between them
        centres = rng.random((12, 3)) * BOX
        model = np.vstack([c + rng.normal(0, 2.5, (15_000, 3)) for c in centres]).astype(np.float32)
        surf = np.vstack([_crop(model, 4000, centres[0], 31), rng.random((3000, 3)) * BOX]).astype(np.float32)
        return model, surf
    raise ValueError(name)


def _answers_visited(pm, surf, idx, qperm, dk):
    """every query's two answers lie in tiles its block visits (the reference's visited set)"""
    vis = ref.visited_pairs(surf, qperm, dk, pm.tbox, pm.prep)
    blk = ref.query_blocks(qperm)
    tiles = ref.row_tiles(pm.perm)
    ok = ref.scored(surf, pm.prep)
    for k in range(2):
        t = tiles[idx[ok, k]]
        assert np.all(vis[blk[ok], t]), f"answer {k} of {int((~vis[blk[ok], t]).sum())} queries in an unvisited tile"
    return vis


@pytest.mark.parametrize("name", ["bench", "scattered", "rod", "sheet", "duplicates", "outside", "blobs"])
def test_visited_pairs_match_the_reference(name, stats_on, oracle_c):
    model, surf = _family(name)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        nb = (len(surf) + ref.BLOCK - 1) // ref.BLOCK
        assert st[0] == 1 and st[2] == nb * pm.n_tiles
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep)
        sel = np.random.default_rng(7).choice(len(surf), min(len(surf), 2000), replace=False)
        ri, rd = oracle_c.knn2_points_f32(surf[sel], model, nthreads=CORES)
        np.testing.assert_array_equal(idx[sel], ri)
        np.testing.assert_array_equal(dist[sel], rd)
        import pcreg_amd as pc
        stats_on("knn_exact", 1)
        ei, ed = pc.knn2_points(surf, model)
        stats_on("knn_exact", 0)
        np.testing.assert_array_equal(idx, ei)
        np.testing.assert_array_equal(dist, ed)
        _answers_visited(pm, surf, idx, qperm, dk)
        i2, d2, qperm2, dk2, st2 = pm.search(surf, nocull=True, debug_set=stats_on)
        assert st2[1] == st2[2] == st[2]
        np.testing.assert_array_equal(i2, idx)
        np.testing.assert_array_equal(_bits(d2), _bits(dist))
        if name == "bench":
            share = st[1] / st[2]
            print(f"bench crop: visited {st[1]} of {st[2]} (block, tile) pairs = {share:.4f}; unproven {st[3]}")
            assert share < 0.06, "culling no longer effective at the bench shape"
    finally:
        pm.close()


# ---- 4. constructed cases on the boundary of the rule ---------------------------------------------------------------
def _lattice_case(a, stats_on, oracle_c, n=32):
    """An n^3 lattice of spacing a (coordinates i * a exact in fp32).  Its ordering cells are narrower than a, so every
    cell holds one node and the sorted order (hence every tile) is fixed.  A query sits on a node q whose +-axis
    neighbour m lies in another tile T whose box is exactly a away on that axis only: G2 = a^2 in float64, while the two
    nearest are q itself (0) and the six neighbours at fl32(a^2) = dk.  m gets the lowest original row of the model, so it
    is the second answer, and q's own tile holds at most three groups within fl32(a^2), so the certificate passes and
    nothing but the rule keeps T."""
    g = np.arange(n, dtype=np.float32) * np.float32(a)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    base = Model(nodes)
    try:
        tile_of = ref.row_tiles(base.perm)
        pos = np.empty(len(nodes), np.int64)
        pos[base.perm] = np.arange(len(nodes))
        seed_cell = _seed_cells(nodes, base.prep)
        seed_cnt = np.bincount(seed_cell[seed_cell >= 0])
        tb = base.tbox.astype(np.float64)
        lut = {tuple(np.round(p / np.float32(a)).astype(int)): i for i, p in enumerate(nodes)}
        d_a = float(np.float32(a) * np.float32(a))
        picks = []                                         # (query row, far-neighbour row)
        used = np.zeros(len(nodes), bool)
        for qi in np.random.default_rng(3).permutation(len(nodes)):
            if len(picks) >= 6:
                break
            ijk = np.round(nodes[qi] / np.float32(a)).astype(int)
            if np.any(ijk < 2) or np.any(ijk > n - 3) or used[qi]:
                continue
            nb = [lut[tuple(ijk + d)] for d in np.vstack([np.eye(3, dtype=int), -np.eye(3, dtype=int)])]
            q64 = nodes[qi].astype(np.float64)
            far = []
            for m in nb:
                t = tile_of[m]
                if t == tile_of[qi]:
                    continue
                gap = np.maximum(0.0, np.maximum(tb[t, :3] - q64, q64 - tb[t, 3:]))
                if float((gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2]) == float(a) * float(a):
                    far.append(m)
            if not far:
                continue
            # q's own tile: groups (32-row sub-tile, half) holding q or one of its neighbours
            grp = {(pos[m] // 32, (pos[m] % 8) // 4) for m in [qi] + nb if tile_of[m] == tile_of[qi]}
            if len(grp) > 3:
                continue
            if max(seed_cnt[seed_cell[qi]], max(seed_cnt[seed_cell[m]] for m in far)) > 4:
                continue                                   # every point of those seeding cells is seeded
            cube = [lut[tuple(ijk + np.array(d))] for d in itertools.product(range(-2, 3), repeat=3)]
            if used[cube].any():                           # picks 5 apart: no neighbour of one is a neighbour of another
                continue
            used[cube] = True
            picks.append((qi, far))
        assert len(picks) >= 3, f"only {len(picks)} query nodes meet the premise"
    finally:
        base.close()
    first = [m for _, far in picks for m in far]
    rest = np.setdiff1d(np.arange(len(nodes)), first)
    order = np.concatenate([np.array(first, np.int64), rest])
    model = nodes[order]                                   # the far neighbours get the lowest rows
    new_row = np.empty(len(nodes), np.int64)
    new_row[order] = np.arange(len(nodes))
    pm = Model(model)
    try:
        np.testing.assert_array_equal(_bits(pm.ms), _bits(nodes[base.perm]))      # same sorted coordinates: same tiles
        for qi, far in picks:
            q = nodes[qi:qi + 1]
            idx, dist, qperm, dk, st = pm.search(q, debug_set=stats_on)
            assert float(dk[0]) == d_a, "premise: dk = fl32(a^2)"
            G2 = ref.gap2(q, q, pm.tbox)[0]
            t_far = ref.row_tiles(pm.perm)[new_row[far]]
            assert np.all(G2[t_far] == float(a) * float(a))
            assert st[1] == ref.visited_count(q, qperm, dk, pm.tbox, pm.prep)
            ri, rd = oracle_c.knn2_points_f32(q, model, nthreads=CORES)
            np.testing.assert_array_equal(idx, ri)
            np.testing.assert_array_equal(dist, rd)
            assert ri[0, 0] == new_row[qi] and ri[0, 1] == min(new_row[far]), "premise: the far neighbour is the answer"
            _answers_visited(pm, q, idx, qperm, dk)
        return G2, d_a
    finally:
        pm.close()


def test_strict_tie_gap_equal_to_dk(stats_on, oracle_c):
    """spacing 0.5: squares are exact, G2 == dk == 0.25 for the far neighbour's tile"""
    G2, d = _lattice_case(0.5, stats_on, oracle_c)
    assert d == 0.25


def test_tie_inside_the_margin_window(stats_on, oracle_c):
    """spacing a = 32769/65536: fl32(a^2) = 0.2500152587890625 < a^2 = G2, and G2 (1 - 32u) <= dk; a rule without the
    margin culls the tile of the tied neighbour"""
    a = 32769 / 65536
    G2, d = _lattice_case(a, stats_on, oracle_c)
    assert d == 0.2500152587890625 < a * a and a * a * (1 - 32 * U) <= d


def test_unseeded_query_turns_culling_off_for_its_block(stats_on, oracle_c):
    """The model's corner x > 80, y > 50, z > 50 is empty; one scored query at (95, 95, 95) finds its 27 seeding cells
    empty (dk = +inf) and shares the only block with a compact crop at z ~ 20.  Its answers sit near x = 80, in tiles that
    the crop's largest dk alone would cull."""
    rng = np.random.default_rng(41)
    model = (rng.random((260_000, 3)) * 100.0).astype(np.float32)
    model = model[~((model[:, 0] > 80) & (model[:, 1] > 50) & (model[:, 2] > 50))]
    crop = _crop(model, 400, np.array([95.0, 95.0, 20.0]), 42, noise=0.02)
    corner = np.array([[95.0, 95.0, 95.0]], np.float32)
    surf = np.vstack([crop, corner]).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        assert dk[-1] == np.inf and np.all(np.isfinite(dk[:-1])), "premise: only the corner query is unseeded"
        assert ref.scored(corner, pm.prep).all()
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep) == pm.n_tiles
        tiles = ref.row_tiles(pm.perm)
        dk_crop = dk.copy()
        dk_crop[-1] = 0.0
        vis_crop = ref.visited_pairs(surf, qperm, dk_crop, pm.tbox, pm.prep)[0]
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        assert not vis_crop[tiles[ri[-1, 0]]] and not vis_crop[tiles[ri[-1, 1]]], "premise: the crop alone culls the answers"
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(dist, rd)
    finally:
        pm.close()


def test_coincident_rows_at_dk_zero(stats_on, oracle_c):
    """Every query coincides with two model rows (dk = 0, so every tile with G2 > 1e-30 is culled), and a third coincident
    row with a LOWER original row was placed so that the cell straddles a tile boundary: both tiles have G2 = 0 and stay."""
    rng = np.random.default_rng(51)
    g = np.arange(32, dtype=np.float32) * np.float32(0.5)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nodes = nodes[rng.permutation(len(nodes))]
    probe = Model(nodes)
    try:
        pos = np.empty(len(nodes), np.int64)
        pos[probe.perm] = np.arange(len(nodes))
    finally:
        probe.close()
    # sorted position of a node after adding two copies of every chosen node before it: choose nodes whose triple starts
    # at 510 or 511 mod 512 (one cell per node: the order of cells is fixed)
    chosen, shift = [], 0
    for r in np.argsort(pos):
        if (pos[r] + shift) % ref.TILE in (510, 511) and len(chosen) < 24:
            chosen.append(r)
            shift += 2
    chosen = np.array(chosen)
    Mc, N = len(chosen), len(nodes)
    model = np.vstack([nodes[chosen], nodes, nodes[chosen]]).astype(np.float32)     # three copies; the lowest rows first
    surf = nodes[chosen]
    pm = Model(model)
    try:
        tiles = ref.row_tiles(pm.perm)
        for k in range(Mc):
            rows = [k, Mc + chosen[k], Mc + N + k]
            assert len({tiles[r] for r in rows}) == 2, "premise: the coincident rows span two tiles"
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep)
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(dist, rd)
        assert np.all(rd == 0) and np.array_equal(ri[:, 0], np.arange(Mc)) and np.array_equal(ri[:, 1], Mc + chosen)
        assert (dk == 0).sum() >= Mc // 2, "premise: most queries are seeded at dk = 0"
        _answers_visited(pm, surf, idx, qperm, dk)
    finally:
        pm.close()


# ---- 5. launch shapes with several tile rounds ----------------------------------------------------------------------
def _shape(Q, M, target=4096, max_s=80):
    """knn_f16_shape: query blocks and workgroups per block"""
    qb = (Q + 511) // 512
    nt = (M + 511) // 512
    s = max(target // qb, 1)
    s = min(s, max_s, nt)
    if s >= 8:
        s = (s + 7) // 8 * 8
    return qb, s, nt


@pytest.mark.parametrize("Q,M,W,rounds", [(300_000, 1_000_000, 6, 2), (1_100_000, 300_000, 1, 3), (20_481, 200_000, 80, 1)])
def test_launch_shapes_with_tile_rounds(Q, M, W, rounds, stats_on, oracle_c):
    rng = np.random.default_rng(Q % 997)
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    near = model[rng.integers(0, M, Q // 2)] + rng.normal(0, 0.05, (Q // 2, 3))      # (Q may exceed M)
    surf = np.vstack([near, rng.random((Q - Q // 2, 3)) * BOX]).astype(np.float32)
    qb, w, nt = _shape(Q, M)
    assert (w, -(-nt // (256 * w))) == (W, rounds)
    if Q % 512 == 1:
        assert qb * 512 - Q == 511                          # the last block holds one query
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        assert st[2] % qb == 0 and st[2] // qb == nt == pm.n_tiles
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep)
        import pcreg_amd as pc
        stats_on("knn_exact", 1)
        ei, ed = pc.knn2_points(surf, model)
        stats_on("knn_exact", 0)
        np.testing.assert_array_equal(idx, ei)
        np.testing.assert_array_equal(_bits(dist), _bits(ed))
        sel = np.random.default_rng(9).choice(Q, 2000, replace=False)
        ri, rd = oracle_c.knn2_points_f32(surf[sel], model, nthreads=CORES)
        np.testing.assert_array_equal(idx[sel], ri)
        np.testing.assert_array_equal(dist[sel], rd)
    finally:
        pm.close()


# ---- 6. scale extremes ----------------------------------------------------------------------------------------------
def test_model_so_small_that_sigma_squared_overflows(stats_on, oracle_c):
    """A 28^3 lattice of spacing 2^-62 (half extent ~2.9e-18 < 2^-58): sigma = 2^64, sigma^2 is +inf in fp32.  Queries are
    lattice nodes and nodes moved by half a spacing (every square a normal fp32 number).  The scaled thresholds used to come
    out as 0 * inf and 32 of 6000 answers were wrong with a passing certificate; such a model now scores no query."""
    s = np.float32(2.0 ** -62)
    g = np.arange(28, dtype=np.float32) * s
    model = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(71)
    model = model[rng.permutation(len(model))]
    base = model[rng.choice(len(model), 3000, replace=False)]
    surf = np.vstack([base[:1500], base[1500:] + rng.integers(-1, 2, (1500, 3)).astype(np.float32) * (s / 2)]).astype(np.float32)
    pm = Model(model)
    try:
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(pm.prep[4]) * np.float32(pm.prep[4])), "premise: sigma^2 overflows fp32"
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        # no query is scored on the matrix cores: nothing visited, every query answered by the exact tail
        assert st[1] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep) == 0 and st[3] == len(surf)
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(_bits(dist), _bits(rd))
    finally:
        pm.close()


def test_model_so_small_that_no_gap_reaches_1e_30(stats_on, oracle_c):
    """Points on a grid of 2^-60 within a cube of 2^-51 (~4.4e-16): every G2 < 1e-30, nothing may be culled."""
    rng = np.random.default_rng(81)
    s = np.float32(2.0 ** -60)
    model = (rng.integers(0, 512, (20_000, 3)).astype(np.float32) * s).astype(np.float32)
    surf = (model[rng.choice(len(model), 4000, replace=False)] + rng.integers(-2, 3, (4000, 3)).astype(np.float32) * s).astype(np.float32)
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = pm.search(surf, debug_set=stats_on)
        ext = float(np.ptp(np.vstack([model, surf]).astype(np.float64), axis=0).max())
        assert 3.0 * ext * ext < 1e-30, "premise: no gap reaches 1e-30"
        assert st[1] == st[2] == ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep)
        ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(_bits(dist), _bits(rd))
    finally:
        pm.close()
