"""Direct answers of the two-nearest search (knn_fast.hip: knn_direct_kernel; DESIGN 4.1 "Direct answers"): a seeded query
whose dk-box covers at most 27 ordering-grid cells holding at most 512 rows is answered from those cells, everything else
takes the tile walk.

Every case compares every idx and the bits of every dist with the plain-C oracle and with a second search on the walk alone
("knn_direct" = 1), and the direct counters ("knn_direct_stats") exactly with tests/knn_direct_ref.py evaluated on the
exported seed distances and preparation record.  Which side of the caps a case's queries fall on is stated as a premise
assert, decided by the reference alone.

The models pin the box to [0, 128] x [0, 64] x [0, zt] with two corner rows, so the ordering grid has cells of edge 2 whose
faces are the even numbers.  Most rows fill that slab uniformly: with zt = 4 about six rows per ordering-grid cell and two per
seeding-grid cell, the proportions of a scanned surface against its model, so dk is close to the true second distance.  The
constructions stand in regions of the slab that are left empty."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_direct_ref as ref
from test_gpu_knn_cull import CORES, Model, _bits, _dev, _p, _soa, _stream

pytestmark = pytest.mark.gpu
F32 = np.float32


def _slab(rng, n, zt=4.0, holes=()):
    """n uniform rows of [0, 128] x [0, 64] x [0, zt] outside the holes (x0, x1, y0, y1), and the two corner rows"""
    out = np.empty((0, 3))
    while len(out) < n - 2:
        p = rng.random((2 * n, 3)) * [128.0, 64.0, zt]
        for x0, x1, y0, y1 in holes:
            p = p[~((p[:, 0] > x0) & (p[:, 0] < x1) & (p[:, 1] > y0) & (p[:, 1] < y1))]
        out = np.vstack([out, p])
    return np.vstack([out[:n - 2], [[0.0, 0.0, 0.0], [128.0, 64.0, zt]]]).astype(F32)


def _near(rng, rows, n, noise=0.05):
    return (rows[rng.choice(len(rows), n, replace=len(rows) < n)] + rng.normal(0, noise, (n, 3))).astype(F32)


def _dstats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 3)()
    check(lib().pcreg_debug_knn_direct_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def _counters(ws):
    """(n_flag, n_direct, direct_rows) of the last search on workspace `ws`: SearchCounters sits at its head (words 0, 4, 5)"""
    w = ws[:32].cpu().numpy().view(np.int32)
    return int(w[0]), int(w[4]), int(w[5])


def _search(pm, surf, ops=None, idx_base=0):
    """one search call -> (idx, dist, dk, (n_flag, n_direct, direct_rows), the process-wide direct counters of the call)"""
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import HipOps
    Q = len(surf)
    ops = ops or HipOps(Q, pm.M, _dev())
    torch.cuda.synchronize()
    _dstats(reset=True)
    idx, dist = ops.local_top2(_soa(surf), pm.pm, idx_base)
    dk = torch.empty(Q, dtype=torch.float32, device=_dev())
    check(lib().pcreg_debug_search_export(_p(ops.ws), C.c_size_t(ops.ws.numel()), Q, pm.M, None, _p(dk), _stream()))
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), dist.cpu().numpy().copy(), dk.cpu().numpy().copy(), _counters(ops.ws), _dstats(reset=True)


def _eligible(pm, surf, dk):
    return ref.eligible(surf, dk, pm.ms, pm.prep[16:19], pm.prep[19])


def _check(pm, surf, model, oracle_c, debug_set, idx_base=0, want=None):
    """direct and walk-only search against the oracle and each other, the counters against the reference -> (idx, dist, dk, e, ctr)"""
    surf = np.ascontiguousarray(surf, F32)
    if want is None:
        with np.errstate(invalid="ignore", over="ignore"):
            want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    wi = np.where(want[0] >= 0, want[0] + idx_base, -1)
    debug_set("knn_direct_stats", 1)
    idx, dist, dk, ctr, st = _search(pm, surf, idx_base=idx_base)
    debug_set("knn_direct", 1)
    idx_w, dist_w, dk_w, ctr_w, st_w = _search(pm, surf, idx_base=idx_base)
    debug_set("knn_direct", 0)
    e = _eligible(pm, surf, dk)
    print(f"Q {len(surf)}: eligible {int(e['ok'].sum())}, rows {int(e['rows'][e['ok']].sum())}, over the cell cap "
          f"{int((e['finite'] & (e['cells'] > ref.CELLS)).sum())}, over the row cap {int((e['rows'] > ref.ROWS).sum())}, not finite "
          f"{int((~e['finite']).sum())}; device {st}, unproven {ctr[0]} (walk alone {ctr_w[0]})")
    np.testing.assert_array_equal(idx_w, wi)
    np.testing.assert_array_equal(_bits(dist_w), _bits(want[1]))
    np.testing.assert_array_equal(idx, wi)
    np.testing.assert_array_equal(_bits(dist), _bits(want[1]))
    np.testing.assert_array_equal(_bits(dk), _bits(dk_w))
    assert st == [1, int(e["ok"].sum()), int(e["rows"][e["ok"]].sum())]
    assert ctr[1:] == (st[1], st[2])
    assert st_w == [1, 0, 0] and ctr_w[1:] == (0, 0), "knn_direct = 1: every query takes the walk"
    return idx, dist, dk, e, ctr


EMPTY = (100.0, 128.0, 44.0, 64.0)               # the shared model's empty corner region (but for the box's corner row)


@pytest.fixture(scope="module")
def slab_model():
    rng = np.random.default_rng(2401)
    model = _slab(rng, 24_000, holes=[EMPTY])
    model = model[rng.permutation(len(model))]
    pm = Model(model)
    assert pm.prep[16:19].tolist() == [0.0, 0.0, 0.0] and pm.prep[19] == 0.5, "premise: cells of edge 2 from the origin"
    yield model, pm
    pm.close()


# ---- 1. a crop-like surface: every query is answered directly -------------------------------------------------------------
def test_crop_like_surface_is_answered_whole(slab_model, oracle_c, debug_set):
    model, pm = slab_model
    rng = np.random.default_rng(1)
    d2 = ((model - np.array([50.0, 24.0, 2.0])) ** 2).sum(axis=1)
    surf = _near(rng, model[np.argsort(d2)[:2003]], 2003)
    idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set)
    assert e["ok"].all(), "premise: every query inside both caps"
    assert ctr == (0, len(surf), int(e["rows"].sum())), "every query answered directly, none unproven"


# ---- 2. every kind of query in one wave and block ---------------------------------------------------------------------------
def test_mixed_wave_and_block(oracle_c, debug_set):
    """zt = 16: seeding-grid cells of edge 2.2, so two rows 2.1 from a query always lie in its 27 cells"""
    rng = np.random.default_rng(2)
    hole = (8.0, 128.5, 40.0, 60.0)              # (open towards x = 128: the queries beyond it see no row)
    wide_q, wide_rows = [], []
    for k in range(24):                          # isolated rows far apart: the query's box spans 4 x 3 x 3 cells
        c = np.array([12.0 + 4.0 * k + 2.05, 45.0 + 6.0 * (k % 2), 9.0])
        wide_q.append(c)
        wide_rows += [c - [2.1, 0, 0], c + [2.1, 0, 0]]
    wide_rows = np.array(wide_rows)
    blob = rng.random((700, 3)) * 0.5 + [112.5, 56.5, 4.5]          # > 512 rows in the cell [112, 114) x [56, 58) x [4, 6)
    model = np.vstack([_slab(rng, 24_000 - len(wide_rows) - len(blob), 16.0, [hole]), wide_rows, blob]).astype(F32)
    model = model[rng.permutation(len(model))]
    assert len(model) == 24_000
    dense = model[(model[:, 1] < 38.0)]
    kinds = dict(
        near=_near(rng, dense, 360),
        wide=np.array(wide_q, F32),
        blob=_near(rng, blob.astype(F32), 60, 0.02),
        unseeded=(rng.random((40, 3)) * [8.0, 8.0, 16.0] + [150.0, 46.0, 0.0]).astype(F32),
        odd=np.array([[np.nan, 5, 5], [5, np.inf, 5], [5, 5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 50], [50, np.nan, np.inf]], F32),
        far=np.array([[40000.0, 10.0, 10.0], [64.0, -34000.0, 8.0]], F32),       # beyond kQueryScaledMax = 16384 scaled units (sigma = 1/2)
    )
    surf = np.vstack(list(kinds.values())).astype(F32)
    kind = np.concatenate([np.full(len(v), k) for k, v in enumerate(kinds.values())])
    order = rng.permutation(len(surf))
    surf, kind = surf[order], kind[order]
    pm = Model(model)
    try:
        assert pm.prep[19] == 0.5 and pm.prep[4] == 0.5, "premise: cells of edge 2, sigma = 1/2"
        with np.errstate(invalid="ignore", over="ignore"):
            idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set)
        ok, fin = e["ok"], e["finite"]
        assert ok[kind == 0].sum() >= 300, "premise: the queries in the dense part are eligible"
        assert (fin & (e["cells"] == 36))[kind == 1].all(), "premise: ranges over kDirectCells around the isolated rows"
        assert (e["rows"] > ref.ROWS)[kind == 2].all(), "premise: ranges over kDirectRows in the blob"
        assert np.isinf(dk[kind == 3]).all(), "premise: unseeded queries outside the box"
        assert not fin[kind == 4].any() and not ok[kind == 5].any() and np.isfinite(surf[kind == 5]).all()
        assert np.all(idx[kind == 4] == -1)
        assert ctr[1] == int(ok.sum()) < len(surf)
        # a wave (128 consecutive slots of the query order, inside one block of 512) holds answered and walking queries of several kinds
        _, _, qperm, _, _ = pm.search(surf)
        n_w = len(surf) // 128
        w_ok, w_kind = ok[qperm][:n_w * 128].reshape(n_w, 128), kind[qperm][:n_w * 128].reshape(n_w, 128)
        assert len(surf) < 512 and len(set(kind[~ok])) >= 5, "premise: one block holds every kind"
        assert any(0 < w_ok[w].sum() < 128 for w in range(n_w)), "premise: a mixed wave"
        print("kinds walking per wave:", [sorted(set(w_kind[w][~w_ok[w]].tolist())) for w in range(n_w)])
    finally:
        pm.close()


# ---- 3. / 4. ties, rows exactly at dk, dk = 0 on a cell face ----------------------------------------------------------------
def _tie_model(rng):
    """the slab with an empty strip, and in the strip groups of rows tied in distance from a query (6 apart: no group sees another)"""
    groups, queries = [], []
    for k in range(8):
        x = 14.0 + 12.0 * k
        c = np.array([x, 48.0, 2.0])                                        # on the face x = 2 k' of two cells
        a, b = c - [0.25, 0, 0], c + [0.25, 0, 0]                          # chain distance 0.0625 each, exactly: dk itself
        groups.append(np.array([a, b, b, a, a, b]))
        queries.append(c)
        c2 = np.array([x + 6.25, 54.0, 2.0])                                # the lower bound q - rho falls just below the face x + 6
        groups.append(np.array([[x + 6.0, 54.0, 2.0]] * 2 + [[x + 6.5, 54.0, 2.0]] * 2))
        queries.append(c2)
    pile = np.array([[20.0, 42.0, 1.0]] * 70)                               # 70 coincident rows: they straddle a 64-row unit
    queries.append(np.array([20.125, 42.0, 1.0]))                           # all 70 tied at 0.015625
    face = np.array([[90.0, 42.0, 2.0]] * 5)                                # coincident rows ON the corner of eight cells ...
    queries.append(np.array([90.0, 42.0, 2.0]))                             # ... and the query on them: dk = 0
    extra = np.vstack(groups + [pile, face])
    model = np.vstack([_slab(rng, 24_000 - len(extra), holes=[(4.0, 124.0, 36.0, 60.0)]), extra]).astype(F32)
    return model[rng.permutation(len(model))], np.array(queries, F32)


def test_ties_and_rows_exactly_at_dk(oracle_c, debug_set):
    rng = np.random.default_rng(3)
    model, special = _tie_model(rng)
    ns = len(special)
    surf = np.vstack([special, _near(rng, model[model[:, 1] < 34.0], 2003 - ns)]).astype(F32)
    pm = Model(model)
    try:
        assert pm.prep[19] == 0.5 and pm.prep[16:19].tolist() == [0.0, 0.0, 0.0]
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        assert np.all(want[1][:ns, 0] == want[1][:ns, 1]) and np.all(want[0][:ns, 0] < want[0][:ns, 1]), "premise: both answers tie"
        idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set, want=want)
        assert e["ok"][:ns].all(), "premise: the constructed queries are answered directly"
        assert np.all(_bits(dk[:ns]) == _bits(want[1][:ns, 1])), "premise: the tied rows lie at chain distance exactly dk"

        def tied(i):             # (the constructions' coordinates and distances are exact in fp32 and in float64)
            d = ((surf[i].astype(np.float64) - model.astype(np.float64)) ** 2).sum(axis=1)
            return np.flatnonzero(d == float(dk[i]))
        for i in range(ns):
            t = tied(i)
            assert len(t) == (6, 4)[i % 2] if i < ns - 2 else len(t) == (70, 5)[i - (ns - 2)]
            assert idx[i].tolist() == sorted(t)[:2], "the lowest original rows win in both columns"
        # the tied rows of the first construction lie in two cells across a face, within the rule's slack of the bounds
        assert len(set(ref.cell(model[tied(0), 0], 0.0, 0.5).tolist())) == 2
        lo_f, hi_f = ref.bounds(surf[:1], dk[:1])
        assert lo_f[0, 0] < model[tied(0), 0].min() and model[tied(0), 0].min() - lo_f[0, 0] < 1e-5
        # ... and the pile straddles a 64-row unit of the sorted copy
        at = np.flatnonzero(np.isin(pm.perm, tied(ns - 2)))
        assert at.max() - at.min() == 69 and at.min() // 64 != at.max() // 64
        # dk = 0 on the corner of eight cells: rho (4e-23) is far below the spacing of the floats at 90, the bounds are the query's
        # own coordinates and the range is the one cell the coincident rows share with it
        assert dk[ns - 1] == 0.0 and (e["hi"][ns - 1] - e["lo"][ns - 1]).tolist() == [0, 0, 0] and e["lo"][ns - 1].tolist() == [45, 21, 1]
        assert dist[ns - 1].tolist() == [0.0, 0.0] and e["rows"][ns - 1] == 5
    finally:
        pm.close()


# ---- 5. seeded queries just outside the model box ---------------------------------------------------------------------------
def test_seeded_queries_just_outside_the_box(slab_model, oracle_c, debug_set):
    model, pm = slab_model
    rng = np.random.default_rng(5)
    x_lo, x_hi, y_lo = model[model[:, 0] < 0.6], model[(model[:, 0] > 127.4) & (model[:, 1] < 40.0)], model[model[:, 1] < 0.6]
    out = [_near(rng, x_lo, 150) * [0, 1, 1] - [0.3, 0, 0], _near(rng, x_hi, 150) * [0, 1, 1] + [128.3, 0, 0],
           _near(rng, y_lo, 150) * [1, 0, 1] - [0, 0.3, 0]]
    surf = np.vstack(out + [_near(rng, model, 1553)]).astype(F32)
    idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set)
    assert np.any((surf[:450] < 0) | (surf[:450] > [128.0, 64.0, 4.0]), axis=1).all() and np.isfinite(dk[:450]).sum() >= 400, \
        "premise: seeded queries outside the box"
    assert e["ok"][:450].sum() >= 400
    assert (e["lo"][:150, 0] == 0).all() and (e["hi"][150:300, 0] == 63).all() and (e["lo"][300:450, 1] == 0).all(), "the ranges clamp"


# ---- 6. ragged, flat and sharded models, and the entry without a handle ------------------------------------------------------
def test_ragged_last_tile_and_cell(oracle_c, debug_set):
    rng = np.random.default_rng(6)
    model = _slab(rng, 30_037)
    model = model[rng.permutation(len(model))]
    assert len(model) == 30_037 and len(model) % 512 and len(model) % 64
    pm = Model(model)
    try:
        last = pm.ms[-40:]                                       # the last sorted rows: the ragged tile, the last occupied cells
        surf = np.vstack([_near(rng, last, 200, 0.02), _near(rng, model, 1803)]).astype(F32)
        idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set)
        assert e["ok"][:200].sum() >= 150 and np.isin(pm.perm[-40:], idx[e["ok"]]).any()
    finally:
        pm.close()


def test_flat_model_with_an_index_base(oracle_c, debug_set):
    rng = np.random.default_rng(7)
    model = _slab(rng, 24_000)
    model[:, 2] = 7.0
    model = model[rng.permutation(len(model))]
    pm = Model(model)
    try:
        surf = _near(rng, model, 2003)
        idx, dist, dk, e, ctr = _check(pm, surf, model, oracle_c, debug_set, idx_base=100_000)
        assert e["ok"].sum() >= 1500 and idx.min() >= 100_000
    finally:
        pm.close()


def test_entry_without_a_handle(slab_model, oracle_c, debug_set):
    from pcreg_amd._lib import check, lib
    model, pm = slab_model
    rng = np.random.default_rng(8)
    surf = _near(rng, model, 2003)
    Q, M = len(surf), len(model)
    L = lib()
    q, m = _soa(surf), _soa(model)
    want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    debug_set("knn_direct_stats", 1)
    got = []
    for walk in (0, 1):
        debug_set("knn_direct", walk)
        ws = torch.empty(L.pcreg_dev_knn2_points_f32_workspace(Q, M), dtype=torch.uint8, device=_dev())
        idx = torch.empty((Q, 2), dtype=torch.int32, device=_dev())
        dist = torch.empty((Q, 2), dtype=torch.float32, device=_dev())
        _dstats(reset=True)
        check(L.pcreg_dev_knn2_points_f32(_p(q), Q, q.stride(0), _p(m), M, m.stride(0), C.c_int32(5), _p(idx), _p(dist), _p(ws),
                                          C.c_size_t(ws.numel()), _stream()))
        torch.cuda.synchronize()
        got.append(_dstats(reset=True))
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0] + 5)
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want[1]))
    # the same model, the same queries: the handle's search answers the same set
    debug_set("knn_direct", 0)
    _, _, dk, ctr, st = _search(pm, surf)
    e = _eligible(pm, surf, dk)
    assert e["ok"].sum() >= 1900 and st == [1, int(e["ok"].sum()), int(e["rows"][e["ok"]].sum())]
    # The entry without a handle prepares the model anew and exports nothing: which rows its seeding grid remembers (whoever
    # arrived first), hence dk and the ranges, differ from the handle's from run to run, so its counters have no exact reference.
    # What holds whatever the grid remembered: one search; every answered query ranked at least its two answers and at most
    # kDirectRows rows; and the premise that the direct path ran at all (the answers above are the oracle's either way).
    assert got[1] == [1, 0, 0] and got[0][0] == 1 and got[0][1] > 0
    assert 2 * got[0][1] <= got[0][2] <= ref.ROWS * got[0][1]


# ---- 7. two searches on one workspace: no mark survives a call -----------------------------------------------------------------
@pytest.mark.parametrize("first", ["eligible", "unseeded"])
def test_two_searches_on_one_workspace(first, slab_model, oracle_c, debug_set):
    from pcreg_amd.device import HipOps
    model, pm = slab_model
    rng = np.random.default_rng(9)
    Q = 2003
    inner = model[(model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40)]
    sets = dict(eligible=_near(rng, inner, Q), unseeded=(rng.random((Q, 3)) * [10.0, 8.0, 4.0] + [140.0, 50.0, 0.0]).astype(F32))
    debug_set("knn_direct_stats", 1)
    ops = HipOps(Q, pm.M, _dev())
    for name in (first, "unseeded" if first == "eligible" else "eligible"):
        surf = sets[name]
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        idx, dist, dk, ctr, st = _search(pm, surf, ops=ops)
        np.testing.assert_array_equal(idx, want[0])
        np.testing.assert_array_equal(_bits(dist), _bits(want[1]))
        e = _eligible(pm, surf, dk)
        assert st[1] == ctr[1] == int(e["ok"].sum())
        if name == "eligible":
            assert e["ok"].all(), "premise: every query of this set is answered directly"
        else:
            assert np.isinf(dk).all() and st[1] == 0, "premise: no query of this set is seeded"


# ---- 8. the match stage with Unique after an all-direct search: the query grid is complete -------------------------------------
def test_match_with_unique_after_direct_answers(slab_model, oracle_c, debug_set):
    import pcreg_amd as pc
    model, _ = slab_model
    rng = np.random.default_rng(10)
    inner = np.flatnonzero((model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40))
    picks = rng.choice(inner, 1500, replace=False)
    surf = np.vstack([model[picks] + rng.normal(0, 0.02, (1500, 3)), model[picks[:503]] + rng.normal(0, 0.03, (503, 3))]).astype(F32)
    debug_set("knn_direct_stats", 1)
    _dstats(reset=True)
    pairs = pc.match_points(surf, model, 0.25, 0.8, True)
    st = _dstats(reset=True)
    ref_pairs = oracle_c.match_points_f32(surf, model, 0.25, 0.8, True)
    assert st[0] == 1 and st[1] == len(surf), "premise: every query was answered directly"
    assert 1000 < len(ref_pairs) < len(surf), "premise: Unique drops the second query of a model row"
    np.testing.assert_array_equal(pairs, ref_pairs)
    debug_set("knn_direct", 1)
    np.testing.assert_array_equal(pc.match_points(surf, model, 0.25, 0.8, True), ref_pairs)
