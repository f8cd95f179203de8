"""The four launch-sized kernels of the point search after their loads were batched: seed_query_kernel (all
cells of a lane in flight), knn_plan_kernel (consecutive tiles per thread, one scan), knn_finalize_kernel (the list kept in
registers, an entry's sixteen rows loaded together) and the few-form of knn_tail_kernel (survivor list, segments dealt over
the waves).

Every case compares idx and the bits of dist with the plain-C oracle, the visited (query block, tile) pairs with
tests/knn_cull_ref.py on the exported query order and seed distances, and runs again with culling off ("knn_nocull")."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_cull_ref as ref
from test_gpu_knn_cull import BOX, CORES, Model, _bits, _dev, _p, _shape, _soa, _stats, _stream, stats_on  # noqa: F401  (stats_on: a fixture)

pytestmark = pytest.mark.gpu
K_FEW = 1024                     # knn_fast.hip: more unproven queries than this take the tail's tiled all-pairs form
LONG_LIST = 128                  # entries; knn_fast.hip keeps LPQ * kOwnEnt = 64 of a query's list in registers: any retuning stays below this
SEED_SLOTS = 4                   # knn_fast_common.hpp: model points remembered per seeding-grid cell


def _check(pm, surf, model, oracle_c, stats_on, want=None):
    """one culled search and one with culling off against the oracle; returns (idx, dist, qperm, dk, stats) of the culled one"""
    if want is None:
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    nb = (len(surf) + ref.BLOCK - 1) // ref.BLOCK
    out = None
    for nocull in (False, True):
        idx, dist, qperm, dk, st = pm.search(surf, nocull=nocull, debug_set=stats_on)
        assert st[0] == 1 and st[2] == nb * pm.n_tiles
        assert st[1] == (st[2] if nocull else ref.visited_count(surf, qperm, dk, pm.tbox, pm.prep))
        np.testing.assert_array_equal(idx, want[0])
        np.testing.assert_array_equal(_bits(dist), _bits(want[1]))
        out = out or (idx, dist, qperm, dk, st)
    return out


def _point_survivors(q, dk, tbox):
    """[Q, n_tiles] bool: the tiles the tail's few-form scans for each query (the rule with the box shrunk to the query)"""
    keep = ~ref.skip(ref.gap2(q, q, tbox), np.asarray(dk, np.float64))
    keep[~(np.isfinite(dk) & np.all(np.isfinite(q), axis=1))] = True
    return keep


# ---- 1. row groups across the end of the model ----------------------------------------------------------------------
@pytest.mark.parametrize("M", [16385, 16387, 20001, 16384 + 511])
def test_row_groups_across_the_end_of_the_model(M, stats_on, oracle_c):
    """M % 4 is 1 or 3 and the last tile is ragged: the entries of queries on the last sorted rows hold rows >= M."""
    rng = np.random.default_rng(M)
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    try:
        tail_rows = pm.ms[-20:]
        on_end = tail_rows[rng.integers(0, 20, 64)].copy()
        on_end[:20] = tail_rows
        surf = np.vstack([rng.random((1936, 3)) * BOX, on_end]).astype(np.float32)
        surf = surf[rng.permutation(len(surf))]
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert np.isin(pm.perm[-20:], idx[:, 0]).all(), "the last sorted rows must appear as answers"
    finally:
        pm.close()


# ---- 2. ties --------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_original_row_in_both_columns(stats_on, oracle_c):
    """Every point four times, shuffled: both neighbours of a query are copies at one distance, and the sixteen rows of a
    list entry hold several equal distances."""
    rng = np.random.default_rng(202)
    base = (rng.random((4500, 3)) * BOX).astype(np.float32)
    model = np.repeat(base, 4, axis=0)
    model = model[rng.permutation(len(model))]
    on = base[rng.choice(len(base), 1000, replace=False)]
    near = base[rng.choice(len(base), 1000, replace=False)] + rng.normal(0, 1e-3, (1000, 3))
    surf = np.vstack([on, near]).astype(np.float32)
    pm = Model(model)
    try:
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        assert np.all(want[1][:, 0] == want[1][:, 1]) and np.all(want[0][:, 0] < want[0][:, 1]), "premise: both neighbours tie"
        _check(pm, surf, model, oracle_c, stats_on, want=want)
    finally:
        pm.close()


# ---- 3. long lists --------------------------------------------------------------------------------------------------
def _list_lengths(ws, Q):
    """cand_cnt of the last search on workspace `ws` (search_ws_layout: counters, gthr, flag_list, cand_cnt).  The library
    exports no count, so the offset is rebuilt here; the caller checks that what it reads behaves as the counts must, query
    by query, which neither neighbouring array (threshold words, places within a cell) does."""
    def up(x):
        return (x + 255) // 256 * 256
    ctr = up((32 + 32 + 4096 + 2048) * 4)                  # SearchCounters (knn_fast_common.hpp)
    off = ctr + 2 * up(4 * Q)
    return ws[off:off + 4 * Q].cpu().numpy().view(np.int32).copy()


def test_lists_longer_than_a_lane_keeps_in_registers(stats_on, oracle_c):
    """W = 80 workgroups per block; queries in an empty corner of the model find no seed, so their block is not culled and
    each of its 49 live workgroups lists its best groups for them: lists beyond the LPQ * kOwnEnt entries kept in registers (the remainder loop of knn_finalize_kernel)."""
    from pcreg_amd.device import HipOps
    rng = np.random.default_rng(303)
    model = (rng.random((110_000, 3)) * 100.0).astype(np.float32)
    model = model[~np.all(model > 60.0, axis=1)][:100_000]
    void = (rng.random((24, 3)) * 6.0 + 82.0)
    surf = np.vstack([rng.random((1976, 3)) * 100.0, void]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    Q, M = len(surf), len(model)
    qb, W, nt = _shape(Q, M)
    assert W >= 16
    pm = Model(model)
    try:
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert np.isinf(dk).sum() >= 12, "premise: the queries in the empty corner are unseeded"
        ops = HipOps(Q, M, _dev())
        i2, d2 = ops.local_top2(_soa(surf), pm.pm, 0)
        torch.cuda.synchronize()
        n = _list_lengths(ops.ws, Q)
        # no list exceeds its capacity, and the long lists are
        # those of the unseeded queries (every live workgroup of their block lists for them)
        layout = "not the candidate counts: the workspace layout has changed"
        assert n.min() >= 0 and n.max() <= W * 4, layout
        void_q = np.isinf(dk)
        print("list lengths: max", n.max(), "queries over", LONG_LIST, ":", int((n > LONG_LIST).sum()), "unseeded:", int(void_q.sum()),
              "shortest unseeded:", n[void_q].min(), "longest seeded:", n[~void_q].max())
        assert n[void_q].min() > n[~void_q].max(), layout
        assert n[void_q].max() > LONG_LIST, "premise: a list far longer than the entries a lane keeps in registers"
        np.testing.assert_array_equal(i2.cpu().numpy(), idx)
        np.testing.assert_array_equal(_bits(d2.cpu().numpy()), _bits(dist))
    finally:
        pm.close()


# ---- 4. seeding edges -----------------------------------------------------------------------------------------------
def test_seeding_edges(stats_on, oracle_c):
    """Queries outside the model's box on every side and at its corners (clamped cells, most of the 27 excluded), in an empty
    region (dk = +inf), with NaN / +-inf coordinates, and in a region of more than kSeedSlots points per cell.  Every finite dk
    is an upper bound of the true second distance and the fmaf-chain distance to some model row, bit for bit."""
    rng = np.random.default_rng(404)
    base = (rng.random((30_000, 3)) * 100.0).astype(np.float32)
    base = base[~np.all(base > 70.0, axis=1)][:24_000]
    dense = (rng.random((3000, 3)) * 0.5 + 20.0).astype(np.float32)
    model = np.vstack([base, dense]).astype(np.float32)
    model = model[rng.permutation(len(model))]
    inside = rng.random((500, 3)) * 100.0
    in_dense = rng.random((200, 3)) * 0.6 + 19.95
    outside = []
    for off in (3.0, 40.0, 9000.0):
        for ax in range(3):
            for side in (-1, 1):
                p = rng.random((6, 3)) * 100.0
                p[:, ax] = -off if side < 0 else 100.0 + off
                outside.append(p)
        corners = np.array([[x, y, z] for x in (-off, 100.0 + off) for y in (-off, 100.0 + off) for z in (-off, 100.0 + off)])
        outside.append(corners)
    void = rng.random((30, 3)) * 4.0 + 84.0
    odd = np.array([[np.nan, 5.0, 5.0], [5.0, np.inf, 5.0], [5.0, 5.0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 50.0],
                    [50.0, np.nan, np.inf]])
    surf = np.vstack([inside, in_dense, np.vstack(outside), void, odd]).astype(np.float32)
    order = rng.permutation(len(surf))
    surf = surf[order]
    is_void = np.isin(order, np.arange(len(surf) - len(odd) - len(void), len(surf) - len(odd)))
    is_odd = order >= len(surf) - len(odd)
    pm = Model(model)
    try:
        cells = np.bincount(_seed_cells_of(model, pm.prep))
        assert cells.max() > SEED_SLOTS, "premise: a cell with more points than the grid remembers"
        with np.errstate(invalid="ignore"):
            want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
            idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on, want=want)
        assert np.all(np.isinf(dk[is_void])), "premise: the 27 cells of a query in the empty region hold fewer than two points"
        assert np.all(dk[is_odd] == np.inf) and np.all(idx[is_odd] == -1)
        fin = np.isfinite(dk)
        assert fin.sum() > 700 and np.all(dk[fin] >= want[1][fin, 1]), "a seed distance below the true second distance"
        m64 = model.astype(np.float64)
        for qi in np.flatnonzero(fin):
            d64 = ((surf[qi].astype(np.float64) - m64) ** 2).sum(axis=1)
            rows = np.flatnonzero(np.abs(d64 - float(dk[qi])) <= 1e-5 * float(dk[qi]) + 1e-30)
            assert len(rows) > 0, f"query {qi}: no model row near its seed distance"
            rows = rows[np.argsort(np.abs(d64[rows] - float(dk[qi])))]
            exact = np.concatenate([oracle_c.knn2_points_f32(surf[qi:qi + 1], model[r:r + 1], nthreads=1)[1][:, 0] for r in rows[:8]])
            assert np.any(_bits(exact) == _bits(dk[qi:qi + 1])[0]), f"query {qi}: dk is no model row's distance"
    finally:
        pm.close()


def _seed_cells_of(x, prep):
    from test_gpu_knn_cull import _seed_cells
    c = _seed_cells(x, prep)
    return c[c >= 0]


# ---- 5. the tail's few-form -----------------------------------------------------------------------------------------
def _copies_model(rng):
    """24 points with 512 copies each and 6 points with 2048, a lattice of spacing 10: a tile is 512 copies of one point, and the
    2048 copies of a point are four tiles next to each other in the sorted order"""
    centres = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(2.0), indexing="ij"), -1).reshape(-1, 3)[:30] * 10.0 + 0.25
    model = np.vstack([np.repeat(centres[:24], 512, axis=0), np.repeat(centres[24:], 2048, axis=0)]).astype(np.float32)
    return centres.astype(np.float32), model[rng.permutation(len(model))]


@pytest.mark.parametrize("pass_tiles", [0, 8])
def test_tail_few_form(pass_tiles, stats_on, oracle_c):
    """Unscored queries far away (no cull: every tile is scanned, survivors of every wave's share) next to scored ones that no
    list can prove: a query on a point with 512 copies (its D = 0 culls every tile but one) and on a point with 2048 (four
    surviving tiles, neighbours in the sorted order).  pass_tiles = 8: the survivor list takes 8 tiles per pass."""
    rng = np.random.default_rng(505)
    centres, model = _copies_model(rng)
    far = rng.uniform(-1, 1, (24, 3)) * 100.0 + 3e6
    one = centres[rng.integers(0, 24, 16)]
    four = centres[24 + rng.integers(0, 6, 16)]
    surf = np.vstack([far, one, four]).astype(np.float32)
    order = rng.permutation(len(surf))
    surf = surf[order]
    pm = Model(model)
    try:
        assert pm.n_tiles == 48 and np.all(pm.tbox[:, 3:] == pm.tbox[:, :3]), "premise: every tile is copies of one point"
        if pass_tiles:
            stats_on("knn_tail_cap", pass_tiles)
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert len(surf) == st[3] and 1 <= st[3] <= K_FEW, f"premise: every query is unproven and the few-form answers, got {st[3]}"
        assert not ref.scored(surf, pm.prep)[order < 24].any() and ref.scored(surf, pm.prep)[order >= 24].all()
        keep = _point_survivors(surf, dk, pm.tbox)
        n_keep = keep.sum(axis=1)
        assert np.all(dk[order >= 24] == 0.0)
        assert np.all(n_keep[(order >= 24) & (order < 40)] == 1), "premise: D culls every tile but one"
        for k in np.flatnonzero(order >= 40):
            t = np.flatnonzero(keep[k])
            assert len(t) == 4 and t[-1] - t[0] == 3, "premise: four surviving tiles, neighbours in the sorted order"
        assert np.all(n_keep[order < 24] > 8), "premise: more survivors than a pass of 8 tiles lists"
        assert np.all(dist[order >= 24] == 0.0)
    finally:
        pm.close()


# ---- 6. the plan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tiles", [1, 255, 256, 257, 513])
def test_plan_with_consecutive_tiles_per_thread(n_tiles, stats_on, oracle_c):
    """A thread of knn_plan_kernel owns per = ceil(n_tiles / 256) consecutive tiles.  Three clusters of 512 queries: on rows of
    the first tile, of the last tile, and of the two tiles either side of a thread's range boundary."""
    M = n_tiles * 512 - 3
    rng = np.random.default_rng(600 + n_tiles)
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    try:
        assert pm.n_tiles == n_tiles
        per = -(-n_tiles // 256)
        edge = min(per * (100 // per + 1), n_tiles - 1)     # first tile of some thread's range
        tiles = sorted({0, n_tiles - 1, max(edge - 1, 0), edge})
        groups = [[0], [n_tiles - 1], [max(edge - 1, 0), edge]]
        surf = np.vstack([pm.ms[t * 512 + rng.integers(0, min(512, M - t * 512), 512 // len(g))] for g in groups for t in g])
        surf = (surf + rng.normal(0, 0.01, surf.shape)).astype(np.float32)
        surf = surf[rng.permutation(len(surf))]
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        seen = ref.visited_pairs(surf, qperm, dk, pm.tbox, pm.prep)
        assert seen.any(axis=0)[tiles].all(), "premise: the first, the last and the boundary tiles are visited"
        if len(tiles) == 4:
            assert (seen[:, edge - 1] & seen[:, edge]).any(), "premise: a block's run crosses a thread's range boundary"
        if M < 16384:
            assert np.all(dk == np.inf) and st[1] == st[2]
        else:
            assert st[1] < st[2], "premise: the plan culls"
    finally:
        pm.close()


# ---- 7. a workspace used twice --------------------------------------------------------------------------------------
def test_two_searches_on_one_workspace(stats_on, oracle_c):
    """Q = 3000, then Q = 1100 on the same workspace and prepared model: the answers of fresh workspaces (stale lists, counters
    or places in the query order would show)."""
    from pcreg_amd._lib import check, lib
    rng = np.random.default_rng(707)
    model = (rng.random((30_000, 3)) * BOX).astype(np.float32)
    far = rng.uniform(-1, 1, (20, 3)) * 50.0 + [4e6, -2e6, 3e6]
    a = np.vstack([rng.random((2980, 3)) * BOX, far]).astype(np.float32)
    b = np.vstack([far[:7], model[rng.choice(len(model), 1093, replace=False)] + rng.normal(0, 0.05, (1093, 3))]).astype(np.float32)
    pm = Model(model)
    try:
        L = lib()
        ws = torch.empty(max(L.pcreg_dev_model_search_workspace(len(a), pm.M), L.pcreg_dev_model_search_workspace(len(b), pm.M)),
                         dtype=torch.uint8, device=_dev())
        for surf in (a, b, a):
            Q = len(surf)
            q = _soa(surf)
            idx = torch.empty((Q, 2), dtype=torch.int32, device=_dev())
            dist = torch.empty((Q, 2), dtype=torch.float32, device=_dev())
            check(L.pcreg_dev_model_search_f32(pm.pm.handle, _p(q), Q, q.stride(0), C.c_int32(0), _p(idx), _p(dist), _p(ws),
                                               C.c_size_t(ws.numel()), _stream()))
            torch.cuda.synchronize()
            fi, fd, _, _, _ = pm.search(surf)
            np.testing.assert_array_equal(idx.cpu().numpy(), fi)
            np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(fd))
            want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
            np.testing.assert_array_equal(fi, want[0])
            np.testing.assert_array_equal(_bits(fd), _bits(want[1]))
    finally:
        pm.close()
