"""seed_query_kernel and knn_finalize_kernel after their gathers were dealt over the lanes of a query's group:
a seeding-grid cell's four slots are read by the four lanes of a quad, two cells per load instruction and 14 rounds for the
27 cells; a list entry's sixteen rows are ranked by the group's eight lanes, two rows each, and the group walks the entries
that pass the cut together.

Every case goes through _check (tests/test_gpu_knn_chains.py): idx and the bits of dist of the culled and of the unculled
search against the plain-C oracle, and the visited pairs against tests/knn_cull_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_knn_chains import _check, _list_lengths
from test_gpu_knn_cull import BOX, CORES, Model, _bits, _dev, _p, _seed_cells, _soa, _stream, stats_on  # noqa: F401  (stats_on: a fixture)

pytestmark = pytest.mark.gpu
SEED_SLOTS = 4                   # knn_fast_common.hpp: model points remembered per seeding-grid cell
OWN_ENTRIES = 64                 # knn_fast.hip: LPQ * kOwnEnt entries of a list stay in registers, the rest goes through the remainder loop


# ---- the seeding grid restated (fp32, as seed_query_kernel has it) ----------------------------------------------------
def _grid(prep):
    return prep[8:11].astype(np.float32), np.float32(prep[11]), prep.view(np.int32)[12:15].astype(np.int64)


def _query_cells(q, prep):
    """[Q, 3] cell of every query, clamped into the grid (seed_cell)"""
    g0, ih, n = _grid(prep)
    f = np.floor((np.asarray(q, np.float32) - g0) * ih).astype(np.float64)
    return np.clip(f, 0, (n - 1).astype(np.float64)).astype(np.int64)


def _rows_of_27(q, model, prep):
    """per query: the model rows of the 27 cells around its own, neighbours outside the grid excluded; and the occupancies of
    the cells it reads"""
    g0, ih, n = _grid(prep)
    mc = _seed_cells(model, prep)
    assert np.all(mc >= 0), "a model row outside the seeding grid"
    order = np.argsort(mc, kind="stable")
    counts = np.bincount(mc, minlength=int(n.prod()))
    starts = np.concatenate([[0], np.cumsum(counts)])
    qc = _query_cells(q, prep)
    rows, occ = [], []
    for c in qc:
        r, o = [], []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    x, y, z = c[0] + dx, c[1] + dy, c[2] + dz
                    if 0 <= x < n[0] and 0 <= y < n[1] and 0 <= z < n[2]:
                        cell = (z * n[1] + y) * n[0] + x
                        r.append(order[starts[cell]:starts[cell + 1]])
                        o.append(counts[cell])
        rows.append(np.concatenate(r))
        occ.append(np.array(o))
    return rows, occ, qc


def _thinned_model(rng, M):
    """M uniform rows, then no seeding-grid cell with more than SEED_SLOTS of them: the surplus rows of over-full cells are
    dropped (never a row that spans the bounding box) and as many fresh rows go into cells that hold at most two, one each,
    so that M and the box -- all the grid's geometry depends on -- stay and the second preparation lays the same grid."""
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    prep = pm.prep
    pm.close()
    cells = _seed_cells(model, prep)
    spans = np.zeros(M, bool)
    spans[np.concatenate([model.argmin(axis=0), model.argmax(axis=0)])] = True
    keep = np.ones(M, bool)
    order = np.lexsort((~spans, cells))                      # by cell, the spanning rows first inside a cell
    sc = cells[order]
    first = np.concatenate([[0], np.flatnonzero(np.diff(sc)) + 1])
    place = np.arange(M) - np.repeat(first, np.diff(np.concatenate([first, [M]])))
    keep[order[place >= SEED_SLOTS]] = False
    assert keep[spans].all()
    kept = model[keep]
    need = M - len(kept)
    counts = np.bincount(cells[keep], minlength=int(prep.view(np.int32)[15]))
    lo, hi = model.min(axis=0), model.max(axis=0)
    cand = (lo + rng.random((40 * need + 100, 3)) * (hi - lo)).astype(np.float32)
    cc = _seed_cells(cand, prep)
    ok = (cc >= 0) & (counts[np.maximum(cc, 0)] <= 2)
    cand, cc = cand[ok], cc[ok]
    _, firsts = np.unique(cc, return_index=True)             # one fresh row per cell
    firsts = np.sort(firsts)[:need]
    assert len(firsts) == need
    out = np.vstack([kept, cand[firsts]]).astype(np.float32)
    return out[rng.permutation(len(out))]


# ---- 1. every slot of every cell is read exactly once -----------------------------------------------------------------
def test_every_slot_of_every_cell_counts_once(stats_on, oracle_c):
    """No cell holds more than kSeedSlots rows, so the slots hold ALL rows of their cells whatever the arrival order, and dk
    is the second-smallest distance over the rows of the query's 27 cells, bit for bit: a (cell, slot) pair left out makes
    it larger for some query, one counted twice smaller (its nearest row would also be its second)."""
    rng = np.random.default_rng(1101)
    model = _thinned_model(rng, 24_000)
    pm = Model(model)
    try:
        g0, ih, n = _grid(pm.prep)
        occupancy = np.bincount(_seed_cells(model, pm.prep), minlength=int(n.prod()))
        assert occupancy.max() <= SEED_SLOTS, "premise: no cell holds more rows than the grid remembers"
        h = np.float32(1.0) / ih
        lo, hi = model.min(axis=0), model.max(axis=0)
        inside = lo + rng.random((1500, 3)) * (hi - lo)
        # the grid's margin cells (index 0 and n - 1): on 1, 2 or 3 axes at once = faces, edges, corners of the grid
        border = []
        for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
            for signs in np.ndindex(*(2,) * len(axes)):
                p = lo + rng.random((9, 3)) * (hi - lo)
                for ax, s in zip(axes, signs):
                    p[:, ax] = lo[ax] - 0.5 * h if s == 0 else g0[ax] + (n[ax] - 0.5) * h
                border.append(p)
        border = np.vstack(border)
        outside = []
        for off in (3.0 * h, 40.0, 9000.0):
            for ax in range(3):
                for side in (-1, 1):
                    p = lo + rng.random((8, 3)) * (hi - lo)
                    p[:, ax] = lo[ax] - off if side < 0 else hi[ax] + off
                    outside.append(p)
            outside.append(np.array([[x, y, z] for x in (lo[0] - off, hi[0] + off) for y in (lo[1] - off, hi[1] + off)
                                     for z in (lo[2] - off, hi[2] + off)]))
        outside = np.vstack(outside)
        on_rows = model[rng.choice(len(model), 2003 - len(inside) - len(border) - len(outside), replace=False)]
        surf = np.vstack([inside, border, outside, on_rows]).astype(np.float32)
        surf = surf[rng.permutation(len(surf))]
        assert len(surf) == 2003, "the last group and the last wave are ragged"
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        rows, occ, qc = _rows_of_27(surf, model, pm.prep)
        top = n - 1
        on_border = ((qc == 0) | (qc == top)).sum(axis=1)
        assert all((on_border == k).sum() >= 20 for k in (0, 1, 2, 3)), "premise: queries inside, on faces, on edges and on corners of the grid"
        seen = np.concatenate(occ)
        assert all((seen == k).any() for k in (1, 2, 3, 4)), "premise: cells of 1, 2, 3 and 4 rows among those the queries read"
        want = np.full(len(surf), np.inf, np.float32)
        for qi, r in enumerate(rows):
            if len(r) >= 2:
                want[qi] = oracle_c.knn2_points_f32(surf[qi:qi + 1], model[r], nthreads=1)[1][0, 1]
        print("seed distances: finite", int(np.isfinite(want).sum()), "+inf", int(np.isinf(want).sum()))
        assert np.isfinite(want).sum() >= 1800
        bad = np.flatnonzero(_bits(dk) != _bits(want))
        assert len(bad) == 0, f"{len(bad)} seed distances differ, first: query {bad[0]} got {dk[bad[0]]!r} want {want[bad[0]]!r}"
    finally:
        pm.close()


# ---- 2. over-full cells -----------------------------------------------------------------------------------------------
def test_over_full_cells_keep_a_valid_seed_distance(stats_on, oracle_c):
    """The dense clump of test_seeding_edges: more than kSeedSlots rows per cell, the slots hold whoever arrived first.  Every
    finite dk is at or above the true second distance, and the fmaf-chain distance to some model row, bit for bit."""
    rng = np.random.default_rng(404)
    base = (rng.random((30_000, 3)) * 100.0).astype(np.float32)
    base = base[~np.all(base > 70.0, axis=1)][:24_000]
    dense = (rng.random((3000, 3)) * 0.5 + 20.0).astype(np.float32)
    model = np.vstack([base, dense]).astype(np.float32)
    model = model[rng.permutation(len(model))]
    in_dense = rng.random((600, 3)) * 0.6 + 19.95
    surf = np.vstack([rng.random((1403, 3)) * 100.0, in_dense]).astype(np.float32)
    order = rng.permutation(len(surf))
    surf = surf[order]
    pm = Model(model)
    try:
        cells = _seed_cells(model, pm.prep)
        assert np.all(cells >= 0)
        occupancy = np.bincount(cells, minlength=int(pm.prep.view(np.int32)[15]))
        assert occupancy.max() > SEED_SLOTS, "premise: a cell with more rows than the grid remembers"
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on, want=want)
        fin = np.isfinite(dk)
        assert fin.sum() > 1500 and np.all(dk[fin] >= want[1][fin, 1]), "a seed distance below the true second distance"
        qcell = _seed_cells(surf, pm.prep)
        crowded = np.flatnonzero(fin & (qcell >= 0) & (occupancy[np.maximum(qcell, 0)] > SEED_SLOTS))
        assert len(crowded) >= 25, "premise: queries whose own cell is over-full"
        sample = np.concatenate([crowded[:25], rng.choice(np.flatnonzero(fin), 25, replace=False)])
        m64 = model.astype(np.float64)
        for qi in sample:
            d64 = ((surf[qi].astype(np.float64) - m64) ** 2).sum(axis=1)
            rows = np.flatnonzero(np.abs(d64 - float(dk[qi])) <= 1e-5 * float(dk[qi]) + 1e-30)
            assert len(rows) > 0, f"query {qi}: no model row near its seed distance"
            rows = rows[np.argsort(np.abs(d64[rows] - float(dk[qi])))]
            exact = np.concatenate([oracle_c.knn2_points_f32(surf[qi:qi + 1], model[r:r + 1], nthreads=1)[1][:, 0] for r in rows[:8]])
            assert np.any(_bits(exact) == _bits(dk[qi:qi + 1])[0]), f"query {qi}: dk is no model row's distance"
    finally:
        pm.close()


# ---- 3. uneven expansion inside one wave --------------------------------------------------------------------------------
def test_uneven_expansion_inside_one_wave(stats_on, oracle_c):
    """Four kinds of query in one random permutation, so that the eight groups of a wave expand 0, 1 and many entries in the
    same trip: on a part of the model that holds every point four times (many entries under the cut, equal distances),
    ordinary ones, unseeded ones in an empty corner (lists beyond the entries kept in registers: the remainder loop expands
    cooperatively too) and NaN / +-inf ones (their lists are as long as an unseeded query's and are expanded whole: no score
    of theirs is a number, so no cut exists).

    M = 36 000: an unseeded query's list holds 4 entries per live workgroup of its block, ceil(n_tiles / 4) of them, so a list
    beyond 64 entries needs more than 64 tiles of 512 rows -- the smallest model that has the premise.  The empty corner is the
    low one: a NaN coordinate sorts into the query order's first cell, so the NaN queries share the unseeded queries' block,
    which is visited whole whatever the plan makes of a NaN."""
    from pcreg_amd.device import HipOps
    rng = np.random.default_rng(1303)

    def outside_corner(n, corner=40.0):
        p = (rng.random((2 * n, 3)) * 100.0).astype(np.float32)
        return p[~np.all(p < corner, axis=1)][:n]

    base = outside_corner(4500)
    model = np.vstack([np.repeat(base, 4, axis=0), outside_corner(18_000)]).astype(np.float32)
    model = model[rng.permutation(len(model))]
    on = base[rng.choice(len(base), 500, replace=False)]
    near = base[rng.choice(len(base), 500, replace=False)] + rng.normal(0, 1e-3, (500, 3))
    ordinary = outside_corner(940, 50.0)               # (well inside the model: seeded)
    void = rng.random((24, 3)) * 6.0 + 12.0
    odd = np.array([[np.nan, 5.0, 5.0], [5.0, np.inf, 5.0], [5.0, 5.0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 50.0],
                    [50.0, np.nan, np.inf]])
    odd = np.vstack([odd] * 6)
    surf = np.vstack([on, near, ordinary, void, odd]).astype(np.float32)
    order = rng.permutation(len(surf))
    surf = surf[order]
    is_copy = order < 1000
    is_void = (order >= 1940) & (order < 1964)
    is_odd = order >= 1964
    Q, M = len(surf), len(model)
    pm = Model(model)
    try:
        with np.errstate(invalid="ignore"):
            want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
            assert np.all(want[1][is_copy, 0] == want[1][is_copy, 1]) and np.all(want[0][is_copy, 0] < want[0][is_copy, 1]), \
                "premise: both neighbours of the queries on the copies tie"
            idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on, want=want)
        assert np.all(np.isinf(dk[is_void])), "premise: the queries in the empty corner are unseeded"
        ops = HipOps(Q, M, _dev())
        i2, d2 = ops.local_top2(_soa(surf), pm.pm, 0)
        torch.cuda.synchronize()
        n = _list_lengths(ops.ws, Q)
        layout = "not the candidate counts: the workspace layout has changed"
        seeded = ~is_void & ~is_odd
        has_nan = np.isnan(surf).any(axis=1)
        assert n.min() >= 0 and n[is_void].min() > n[seeded].max(), layout
        print("list lengths: unseeded", n[is_void].min(), "..", n[is_void].max(), "longest seeded", n[seeded].max(),
              "inf without NaN", n[is_odd & ~has_nan].max(), "NaN", n[has_nan].min(), "..", n[has_nan].max())
        assert n[is_void].max() > OWN_ENTRIES, "premise: a list longer than the entries a lane keeps in registers"
        # The candidate kernel lists for a NaN / +-inf query as for an unseeded one (its threshold word was never lowered); the
        # entries' scores are no numbers, so no cut exists and the group expands the whole list, to distances that rank nowhere.
        assert np.all(idx[is_odd] == -1)
        np.testing.assert_array_equal(i2.cpu().numpy(), idx)
        np.testing.assert_array_equal(_bits(d2.cpu().numpy()), _bits(dist))
    finally:
        pm.close()


# ---- 4. rows past the end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [16385, 16387])
def test_rows_past_the_end_with_two_rows_per_lane(M, stats_on, oracle_c):
    """M % 4 is 1 and 3 and the last tile is ragged: the entries of queries on the last sorted rows hold rows >= M, which
    the lanes that own them read as row M - 1 and leave out."""
    rng = np.random.default_rng(1400 + M)
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    pm = Model(model)
    try:
        tail_rows = pm.ms[-20:]
        on_end = tail_rows[rng.integers(0, 20, 84)].copy()
        on_end[:20] = tail_rows
        on_end[20:] += rng.normal(0, 0.01, (64, 3))
        surf = np.vstack([rng.random((1919, 3)) * BOX, on_end]).astype(np.float32)
        surf = surf[rng.permutation(len(surf))]
        idx, dist, qperm, dk, st = _check(pm, surf, model, oracle_c, stats_on)
        assert np.isin(pm.perm[-20:], idx[:, 0]).all(), "the last sorted rows must appear as answers"
    finally:
        pm.close()


# ---- 5. two searches on one workspace -----------------------------------------------------------------------------------
def test_two_searches_on_one_workspace_agree(oracle_c):
    """The same queries twice on one workspace: the counters are left as found, so both calls return the same bits."""
    from pcreg_amd._lib import check, lib
    rng = np.random.default_rng(1505)
    model = (rng.random((20_000, 3)) * BOX).astype(np.float32)
    far = rng.uniform(-1, 1, (11, 3)) * 50.0 + [4e6, -2e6, 3e6]
    surf = np.vstack([rng.random((1992, 3)) * BOX, far]).astype(np.float32)
    Q = len(surf)
    pm = Model(model)
    try:
        L = lib()
        ws = torch.empty(L.pcreg_dev_model_search_workspace(Q, pm.M), dtype=torch.uint8, device=_dev())
        q = _soa(surf)
        got = []
        for _ in range(2):
            idx = torch.empty((Q, 2), dtype=torch.int32, device=_dev())
            dist = torch.empty((Q, 2), dtype=torch.float32, device=_dev())
            check(L.pcreg_dev_model_search_f32(pm.pm.handle, _p(q), Q, q.stride(0), C.c_int32(0), _p(idx), _p(dist), _p(ws),
                                               C.c_size_t(ws.numel()), _stream()))
            torch.cuda.synchronize()
            got.append((idx.cpu().numpy(), dist.cpu().numpy()))
        np.testing.assert_array_equal(got[0][0], got[1][0])
        np.testing.assert_array_equal(_bits(got[0][1]), _bits(got[1][1]))
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        np.testing.assert_array_equal(got[0][0], want[0])
        np.testing.assert_array_equal(_bits(got[0][1]), _bits(want[1]))
    finally:
        pm.close()
