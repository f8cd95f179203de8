"""Seeding and the direct answers in one launch (knn_fast.hip: seed_direct_kernel; DESIGN 4.1 "Direct answers").

Every case runs the search twice, with "knn_seed_fused" = 0 (one launch, the default) and = 1 (seed_query_kernel and
knn_direct_kernel, two launches), and compares every idx and the bits of every dist with the plain-C oracle and between the
two; between the two paths also what the search leaves in its workspace for the launches that follow -- the seed distances
(pcreg_debug_search_export), the threshold words gthr, the cand_cnt words (the mark of an answered query or 0) and each query's
place in its parent cell -- and the direct counters, both the call's own (SearchCounters, words 4 and 5 of the workspace) and
the process-wide sums of "knn_direct_stats".

A query's place in its cell is the return value of an atomic: which query of a cell gets which place differs from run to run
in either path.  What is compared is what the order needs: the places of a cell's queries are distinct and below the cell's
count, and, whenever somebody reads it, the exported query order is a permutation in parent-cell order.

The seeding grid is only built for models of at least 16 384 rows, so the small models the shapes name (M = 3, 300, 5 000) never
reach the direct phase in either path: they hold the one-launch path's other side (seed_query_kernel alone) to the oracle.  The
same query counts run against a seeded model of 24 000 rows, where the fused kernel does run."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_knn_cull import CORES, Model, _bits, _dev, _p, _soa, _sort_keys, _stream
from test_gpu_knn_direct import EMPTY, _dstats, _near, _slab

pytestmark = pytest.mark.gpu
F32 = np.float32
CTR_BYTES = 4 * (32 + 32 + 4096 + 2048)          # sizeof(SearchCounters), a multiple of 256: gthr, flag_list, cand_cnt follow
MARK = -2**31                                    # kDirectMark
PARTS_ALL = 2048                                 # kDirectPartsAll: above it only one workgroup of the query order sums the pairs


def _words(ws, Q, k):
    """array k (0 gthr, 1 flag_list, 2 cand_cnt) of the search workspace: Q words each, every array rounded up to 256 bytes"""
    step = (4 * Q + 255) // 256 * 256
    return ws[CTR_BYTES + k * step:CTR_BYTES + k * step + 4 * Q].cpu().numpy().view(np.int32).copy()


def _search(pm, surf, fused_key, debug_set, ops=None, idx_base=0, pad=0):
    """one search with "knn_seed_fused" = fused_key -> what it returned and what it left in the workspace"""
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import HipOps
    Q = len(surf)
    ops = ops or HipOps(Q, max(pm.M, 1), _dev())
    q = _soa(surf)
    if pad:                                      # ldq > Q
        wide = torch.full((3, Q + pad), float("nan"), dtype=torch.float32, device=_dev())
        wide[:, :Q] = q
        q = wide[:, :Q]
        assert q.stride(0) == Q + pad
    debug_set("knn_direct_stats", 1)
    debug_set("knn_seed_fused", fused_key)
    torch.cuda.synchronize()
    _dstats(reset=True)
    idx, dist = ops.local_top2(q, pm.pm, idx_base)
    qperm = torch.empty(Q, dtype=torch.int32, device=_dev())
    dk = torch.empty(Q, dtype=torch.float32, device=_dev())
    check(lib().pcreg_debug_search_export(_p(ops.ws), C.c_size_t(ops.ws.numel()), Q, pm.M, _p(qperm), _p(dk), _stream()))
    torch.cuda.synchronize()
    ctr = ops.ws[:32].cpu().numpy().view(np.int32)
    out = dict(idx=idx.cpu().numpy().copy(), dist=dist.cpu().numpy().copy(), dk=dk.cpu().numpy().copy(), qperm=qperm.cpu().numpy().copy(),
               gthr=_words(ops.ws, Q, 0), place=_words(ops.ws, Q, 1), cand_cnt=_words(ops.ws, Q, 2),
               n_flag=int(ctr[0]), n_direct=int(ctr[4]), direct_rows=int(ctr[5]), st=_dstats(reset=True))
    debug_set("knn_seed_fused", 0)
    return out


def _check_order(pm, surf, r):
    """the places and, where it is read, the query order (module docstring)"""
    Q = len(surf)
    parent = (_sort_keys(surf, pm.prep) >> np.uint32(3)).astype(np.int64)
    count = np.bincount(parent, minlength=int(parent.max()) + 1)
    # knn_finalize_kernel lists the n_flag unproven queries over the head of the places' array
    keep = np.arange(Q) >= r["n_flag"]
    place = r["place"].astype(np.int64)
    assert np.all((place[keep] >= 0) & (place[keep] < count[parent[keep]]))
    pairs = parent[keep] * (Q + 1) + place[keep]
    assert len(np.unique(pairs)) == len(pairs), "two queries of a cell share a place"
    if r["n_direct"] < Q:
        assert np.array_equal(np.sort(r["qperm"]), np.arange(Q)), "qperm is not a permutation"
        assert np.all(np.diff(parent[r["qperm"]]) >= 0), "query slots are not in parent-cell order"


def _check(pm, surf, model, oracle_c, debug_set, idx_base=0, pad=0, want=None, ops=None):
    """fused and two-launch search against the oracle and each other -> the fused run"""
    surf = np.ascontiguousarray(surf, F32)
    if want is None:
        with np.errstate(invalid="ignore", over="ignore"):
            want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    wi = np.where(want[0] >= 0, want[0] + idx_base, -1)
    one = _search(pm, surf, 0, debug_set, ops=ops, idx_base=idx_base, pad=pad)
    two = _search(pm, surf, 1, debug_set, ops=ops, idx_base=idx_base, pad=pad)
    print(f"Q {len(surf)} M {pm.M}: answered {one['n_direct']} ({two['n_direct']}), rows {one['direct_rows']} ({two['direct_rows']}), "
          f"unproven {one['n_flag']} ({two['n_flag']})")
    for r in (one, two):
        np.testing.assert_array_equal(r["idx"], wi)
        np.testing.assert_array_equal(_bits(r["dist"]), _bits(want[1]))
        assert r["st"] == [1, r["n_direct"], r["direct_rows"]]
        assert int((r["cand_cnt"] == MARK).sum()) == r["n_direct"] and np.all((r["cand_cnt"] == MARK) | (r["cand_cnt"] >= 0))
        _check_order(pm, surf, r)
    np.testing.assert_array_equal(_bits(one["dk"]), _bits(two["dk"]))
    np.testing.assert_array_equal(one["gthr"], two["gthr"])
    np.testing.assert_array_equal(one["cand_cnt"] == MARK, two["cand_cnt"] == MARK)       # (an unanswered query's word: its list's length)
    assert (one["n_direct"], one["direct_rows"], one["n_flag"] == 0) == (two["n_direct"], two["direct_rows"], two["n_flag"] == 0)
    return one


@pytest.fixture(scope="module")
def slab():
    rng = np.random.default_rng(2601)
    model = _slab(rng, 24_000, holes=[EMPTY])
    model = model[rng.permutation(len(model))]
    pm = Model(model)
    assert pm.prep[16:19].tolist() == [0.0, 0.0, 0.0] and pm.prep[19] == 0.5, "premise: cells of edge 2 from the origin"
    yield model, pm
    pm.close()


@pytest.fixture(scope="module")
def small_models():
    rng = np.random.default_rng(2602)
    made = {M: (rng.random((M, 3)) * [40.0, 30.0, 8.0]).astype(F32) for M in (3, 300, 5000)}
    pms = {M: Model(m) for M, m in made.items()}
    yield made, pms
    for pm in pms.values():
        pm.close()


# ---- 1. the group, wave and workgroup edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 7, 31, 32, 33, 257])
def test_query_counts_on_a_seeded_model(Q, slab, oracle_c, debug_set):
    model, pm = slab
    rng = np.random.default_rng(Q)
    inner = model[(model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40)]
    for idx_base, pad in ((0, 0), (1, 5)):
        r = _check(pm, _near(rng, inner, Q), model, oracle_c, debug_set, idx_base=idx_base, pad=pad)
        assert r["n_direct"] == Q, "premise: every query of this surface is answered directly"


@pytest.mark.parametrize("M", [300, 5000])
@pytest.mark.parametrize("Q", [1, 7, 31, 32, 33, 257])
def test_query_counts_on_an_unseeded_model(Q, M, small_models, oracle_c, debug_set):
    made, pms = small_models
    rng = np.random.default_rng(100 * Q + M)
    for idx_base, pad in ((0, 0), (1, 3)):
        r = _check(pms[M], _near(rng, made[M], Q, 0.2), made[M], oracle_c, debug_set, idx_base=idx_base, pad=pad)
        assert r["n_direct"] == 0 and np.isinf(r["dk"]).all(), "no seeding grid: the fused kernel does not run"


def test_model_of_three_rows(small_models, oracle_c, debug_set):
    made, pms = small_models
    rng = np.random.default_rng(3)
    r = _check(pms[3], (rng.random((33, 3)) * 50.0).astype(F32), made[3], oracle_c, debug_set)
    assert r["n_direct"] == 0 and np.isinf(r["dk"]).all()


# ---- 2. every verdict in one workgroup ------------------------------------------------------------------------------------------
def test_mixed_verdicts_in_one_workgroup(oracle_c, debug_set):
    """zt = 16: seeding-grid cells of edge 2.2, so two rows 2.1 from a query always lie in its 27 cells.  A workgroup holds 32
    consecutive queries, a wave 8: the kinds are dealt round-robin, so every wave holds eligible queries beside the others."""
    rng = np.random.default_rng(12)
    hole = (8.0, 128.5, 40.0, 60.0)
    wide_q, wide_rows = [], []
    for k in range(12):                          # isolated rows far apart: the query's box spans 4 x 3 x 3 cells, over kDirectCells
        c = np.array([12.0 + 8.0 * k + 2.05, 45.0 + 6.0 * (k % 2), 9.0])
        wide_q.append(c)
        wide_rows += [c - [2.1, 0, 0], c + [2.1, 0, 0]]
    blob = rng.random((700, 3)) * 0.5 + [112.5, 56.5, 4.5]          # over kDirectRows rows in one cell
    model = np.vstack([_slab(rng, 24_000 - len(wide_rows) - len(blob), 16.0, [hole]), np.array(wide_rows), blob]).astype(F32)
    model = model[rng.permutation(len(model))]
    dense = model[model[:, 1] < 38.0]
    kinds = [
        _near(rng, dense, 12),                                                                         # 0 eligible
        np.array(wide_q, F32),                                                                         # 1 over the cell cap
        _near(rng, blob.astype(F32), 12, 0.02),                                                        # 2 over the row cap
        (rng.random((12, 3)) * [8.0, 8.0, 16.0] + [150.0, 46.0, 0.0]).astype(F32),                      # 3 no finite dk
        np.array([[np.nan, 5, 5], [5, np.inf, 5], [5, 5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 50], [50, np.nan, np.inf],
                  [-np.inf, 5, 5], [5, 5, np.nan], [np.inf, np.inf, np.inf], [5, -np.inf, np.nan], [np.nan, 5, np.inf], [5, np.nan, 5]], F32),   # 4
        np.array([[40000.0, 10.0, 10.0], [64.0, -34000.0, 8.0], [-1e6, 3.0, 3.0], [10.0, 10.0, 1e7], [90000.0, -70000.0, 1.0], [5.0, 5.0, -50000.0]] * 2, F32),   # 5 far
        _near(rng, dense, 12), _near(rng, dense, 12),                                                  # 6, 7 eligible
    ]
    assert all(len(k) == 12 for k in kinds)
    surf = np.stack(kinds, axis=1).reshape(-1, 3).astype(F32)       # query i is of kind i % 8: one of each in every wave
    kind = np.arange(len(surf)) % 8
    pm = Model(model)
    try:
        assert pm.prep[19] == 0.5, "premise: cells of edge 2"
        with np.errstate(invalid="ignore", over="ignore"):
            r = _check(pm, surf, model, oracle_c, debug_set)
        ok = r["cand_cnt"] == MARK
        assert ok[np.isin(kind, (0, 6, 7))].sum() >= 30, "premise: the queries in the dense part are answered"
        assert not ok[np.isin(kind, (1, 2, 3, 4, 5))].any(), "premise: none of the others is"
        assert np.isfinite(r["dk"][kind == 1]).all() and np.isfinite(r["dk"][kind == 2]).all() and np.isinf(r["dk"][kind == 3]).all()
        assert np.all(r["idx"][kind == 4] == -1)
    finally:
        pm.close()


def test_query_in_ordering_cell_zero(slab, oracle_c, debug_set):
    model, pm = slab
    rng = np.random.default_rng(13)
    corner = model[(model[:, 0] < 2.0) & (model[:, 1] < 2.0) & (model[:, 2] < 2.0)]
    assert len(corner) >= 2, "premise: rows in the cell of Morton key 0"
    surf = np.vstack([_near(rng, corner, 9, 0.02), _near(rng, model, 24)]).astype(F32)
    r = _check(pm, surf, model, oracle_c, debug_set)
    in_zero = _sort_keys(surf[:9], pm.prep) == 0
    assert (in_zero & (r["cand_cnt"][:9] == MARK)).sum() >= 5, "premise: queries in the cell of key 0 are answered directly"


# ---- 3. all answered, none answered, and what a workspace held before ----------------------------------------------------------
def _sets(model, rng, Q):
    inner = model[(model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40)]
    unseeded = (rng.random((Q, 3)) * [10.0, 8.0, 4.0] + [140.0, 50.0, 0.0]).astype(F32)
    a, b = _near(rng, inner, Q), _near(rng, inner, Q)
    mixed = np.where((np.arange(Q) % 3 == 0)[:, None], unseeded, _near(rng, inner, Q)).astype(F32)
    return a, b, mixed, unseeded


def test_searches_in_a_row_on_one_workspace(slab, oracle_c, debug_set):
    """all answered (the query order leaves early), another set all answered, a mixed set (the order is read again), none
    answered: every call gives its own set's answers and counts, whatever the call before left"""
    from pcreg_amd.device import HipOps
    model, pm = slab
    rng = np.random.default_rng(14)
    Q = 1003
    a, b, mixed, unseeded = _sets(model, rng, Q)
    ops = HipOps(Q, pm.M, _dev())
    got = [_check(pm, s, model, oracle_c, debug_set, ops=ops) for s in (a, b, mixed, unseeded, a)]
    assert [g["n_direct"] for g in got[:2]] == [Q, Q] and got[4]["n_direct"] == Q, "premise: every query answered"
    assert 0 < got[2]["n_direct"] < Q and got[3]["n_direct"] == 0 and np.isinf(got[3]["dk"]).all()
    assert got[4]["direct_rows"] == got[0]["direct_rows"]


@pytest.mark.parametrize("fused_key", [0, 1])
def test_counters_do_not_depend_on_the_workspace(fused_key, slab, oracle_c, debug_set):
    from pcreg_amd.device import HipOps
    model, pm = slab
    rng = np.random.default_rng(15)
    Q = 1003
    a, _, mixed, _ = _sets(model, rng, Q)
    for surf in (a, mixed):
        want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
        runs = []
        for fill in (0x00, 0xFF):
            ops = HipOps(Q, pm.M, _dev())
            ops.ws.fill_(fill)
            r = _search(pm, surf, fused_key, debug_set, ops=ops)
            np.testing.assert_array_equal(r["idx"], want[0])
            np.testing.assert_array_equal(_bits(r["dist"]), _bits(want[1]))
            runs.append((r["n_direct"], r["direct_rows"], r["st"]))
        assert runs[0] == runs[1] and runs[0][2] == [1, runs[0][0], runs[0][1]]


@pytest.mark.parametrize("extra", [0, 1])
def test_more_pairs_than_every_workgroup_sums(extra, slab, oracle_c, debug_set):
    """Q / 32 > kDirectPartsAll: workgroup 0 of the query order alone sums the direct phase's pairs; all answered (extra = 0) and
    all but one"""
    model, pm = slab
    rng = np.random.default_rng(16)
    Q = 32 * PARTS_ALL + 33
    inner = model[(model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40)]
    surf = _near(rng, inner, Q)
    if extra:
        surf[Q // 2] = [145.0, 55.0, 2.0]
    r = _check(pm, surf, model, oracle_c, debug_set)
    assert r["n_direct"] == Q - extra


# ---- 4. the match stage, the entry without a handle, and the paths on which the fused kernel does not run -------------------
def test_match_with_unique_after_either_path(slab, oracle_c, debug_set):
    import pcreg_amd as pc
    model, _ = slab
    rng = np.random.default_rng(17)
    inner = np.flatnonzero((model[:, 0] > 10) & (model[:, 0] < 90) & (model[:, 1] > 8) & (model[:, 1] < 40))
    picks = rng.choice(inner, 1500, replace=False)
    surf = np.vstack([model[picks] + rng.normal(0, 0.02, (1500, 3)), model[picks[:503]] + rng.normal(0, 0.03, (503, 3))]).astype(F32)
    ref_pairs = oracle_c.match_points_f32(surf, model, 0.25, 0.8, True)
    assert 1000 < len(ref_pairs) < len(surf), "premise: Unique drops the second query of a model row"
    debug_set("knn_direct_stats", 1)
    for key in (0, 1):
        debug_set("knn_seed_fused", key)
        _dstats(reset=True)
        pairs = pc.match_points(surf, model, 0.25, 0.8, True)
        assert _dstats(reset=True)[:2] == [1, len(surf)], "premise: every query was answered directly"
        np.testing.assert_array_equal(pairs, ref_pairs)


def test_entry_without_a_handle(slab, oracle_c, debug_set):
    """no query grid (with_grid off); the model is prepared anew in every call, so only the answers are comparable"""
    from pcreg_amd._lib import check, lib
    model, _ = slab
    rng = np.random.default_rng(18)
    surf = np.vstack([_near(rng, model, 1000), (rng.random((3, 3)) * 5.0 + [150.0, 50.0, 0.0])]).astype(F32)
    Q, M = len(surf), len(model)
    L = lib()
    q, m = _soa(surf), _soa(model)
    want = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    debug_set("knn_direct_stats", 1)
    for key in (0, 1):
        debug_set("knn_seed_fused", key)
        ws = torch.full((L.pcreg_dev_knn2_points_f32_workspace(Q, M),), 0xFF, dtype=torch.uint8, device=_dev())
        idx = torch.empty((Q, 2), dtype=torch.int32, device=_dev())
        dist = torch.empty((Q, 2), dtype=torch.float32, device=_dev())
        _dstats(reset=True)
        check(L.pcreg_dev_knn2_points_f32(_p(q), Q, q.stride(0), _p(m), M, m.stride(0), C.c_int32(1), _p(idx), _p(dist), _p(ws),
                                          C.c_size_t(ws.numel()), _stream()))
        torch.cuda.synchronize()
        st = _dstats(reset=True)
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0] + 1)
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want[1]))
        assert st[0] == 1 and 0 < st[1] < Q and 2 * st[1] <= st[2] <= 512 * st[1]


def test_walk_alone_runs_no_direct_phase(slab, oracle_c, debug_set):
    model, pm = slab
    rng = np.random.default_rng(19)
    surf = _near(rng, model, 515)
    debug_set("knn_direct", 1)
    r = _check(pm, surf, model, oracle_c, debug_set)
    assert r["n_direct"] == 0 and not (r["cand_cnt"] == MARK).any() and np.isfinite(r["dk"]).sum() > 400
