"""The point search over a spatially ordered model with tile culling (knn_fast.hip, knn_mfma16.hip).

A prepared model's rows are stored in Morton order, each call orders its queries the same way, and the candidate kernel
skips every model tile that is provably farther from a block of queries than two real model points.  None of that may
show in the results: indices (ORIGINAL rows, ties to the lowest) and fp32 distances stay the oracle's bits, whatever the
query order, the model's shape, or how the equidistant points fall into tiles."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
BOX = np.array([101.0, 56.0, 99.0])


def _dev():
    return torch.device("cuda", 0)


def _soa(x):
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())    # [3, N] with strides (N, 1), also for N = 1
    t.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
    return t


def _search(model, surf, m_lo=0):
    """device tier: prepared handle + pcreg_dev_model_search_f32 (idx_base = m_lo); returns numpy idx, dist"""
    from pcreg_amd.device import HipOps, PreparedModel
    pm = PreparedModel(_soa(model))
    ops = HipOps(len(surf), max(pm.M, 1), _dev())
    idx, dist = ops.local_top2(_soa(surf), pm, m_lo)
    out = idx.cpu().numpy().copy(), dist.cpu().numpy().copy()
    pm.close()
    return out


def _check(model, surf, oracle_c, **kw):
    idx, dist = _search(model, surf, **kw)
    ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist, rd)
    return idx, dist


def _crop(model, Q, centre, seed):
    rng = np.random.default_rng(seed)
    d2 = ((model - centre) ** 2).sum(axis=1)
    sel = np.sort(np.argpartition(d2, Q - 1)[:Q])
    return (model[sel] + rng.normal(0, 0.05, (Q, 3))).astype(np.float32)


def test_bench_shape_spot_check(oracle_c):
    """bench.py's default shape (50 k crop against 1 M rows): 1000 random queries against the exhaustive oracle."""
    from bench import synth
    model, surf, _ = synth(1_000_000, 50_000)
    idx, dist = _search(model, surf)
    sel = np.random.default_rng(11).choice(len(surf), 1000, replace=False)
    ri, rd = oracle_c.knn2_points_f32(surf[sel], model, nthreads=CORES)
    np.testing.assert_array_equal(idx[sel], ri)
    np.testing.assert_array_equal(dist[sel], rd)


def test_query_order_does_not_change_a_bit(oracle_c):
    """one crop in model order, shuffled, and spatially sorted: the same bits per query"""
    rng = np.random.default_rng(3)
    model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
    surf = _crop(model, 20_000, BOX * 0.5, 4)
    idx0, dist0 = _check(model, surf, oracle_c)
    for order in (rng.permutation(len(surf)), np.lexsort((surf[:, 0], surf[:, 1], (surf[:, 2] // 2)))):
        idx, dist = _search(model, surf[order])
        np.testing.assert_array_equal(idx, idx0[order])
        np.testing.assert_array_equal(dist, dist0[order])


def test_scattered_queries_nothing_to_cull(oracle_c):
    """queries spread over the whole box: every block's box spans the model, every tile is visited"""
    rng = np.random.default_rng(5)
    model = (rng.random((150_000, 3)) * BOX).astype(np.float32)
    surf = (rng.random((12_000, 3)) * BOX).astype(np.float32)
    _check(model, surf, oracle_c)


@pytest.mark.parametrize("shape", ["rod", "sheet", "duplicates"])
def test_anisotropic_flat_and_duplicated_models(shape, oracle_c):
    rng = np.random.default_rng({"rod": 6, "sheet": 7, "duplicates": 8}[shape])
    if shape == "rod":                                   # 1000 x 2 x 1: one axis carries nearly all of the ordering grid
        model = (rng.random((120_000, 3)) * [1000.0, 2.0, 1.0]).astype(np.float32)
    elif shape == "sheet":                               # z = const: a flat axis, exact ties in z
        model = (rng.random((120_000, 3)) * [80.0, 60.0, 0.0] + [0.0, 0.0, 3.0]).astype(np.float32)
    else:                                                # every point three times (equal distances, rows far apart)
        base = (rng.random((40_000, 3)) * BOX).astype(np.float32)
        model = np.vstack([base, base[::-1], base])
    q = model[rng.choice(len(model), 8000, replace=False)]
    surf = np.vstack([q + rng.normal(0, 0.05, q.shape), q[:2000]]).astype(np.float32)
    _check(model, surf, oracle_c)


def test_equidistant_points_in_different_tiles(oracle_c):
    """Around each of 32 queries (20 apart) the model is emptied to radius 6 and four points are planted at distance
    exactly 5 (+x, +y, -x, -y: 10 apart, so in different tiles).  Morton order is monotone along each axis, so the +x / +y
    points sort AFTER the -x / -y ones; they get the LOWER original rows, and must win the tie."""
    rng = np.random.default_rng(9)
    model = (rng.random((300_000, 3)) * BOX).astype(np.float32)
    centres = np.array([[x, y, z] for x in (15, 35, 55, 75) for y in (15, 35) for z in (15, 35, 55, 75)], np.float32)
    keep = np.ones(len(model), bool)
    for c in centres:
        keep &= ((model - c) ** 2).sum(axis=1) > 36.0
    model = model[keep]
    low, high = [], []
    for c in centres:
        low += [c + [5.0, 0, 0], c + [0, 5.0, 0]]
        high += [c - [5.0, 0, 0], c - [0, 5.0, 0]]
    low, high = np.array(low, np.float32), np.array(high, np.float32)
    model = np.vstack([low, model, high]).astype(np.float32)           # rows 0..63 (+x, +y), then the cloud, then (-x, -y)
    surf = np.vstack([centres, _crop(model, 6000, BOX * 0.5, 10)]).astype(np.float32)
    idx, dist = _check(model, surf, oracle_c)
    assert np.all(dist[:32] == 25.0)
    np.testing.assert_array_equal(idx[:32], np.stack([np.arange(0, 64, 2), np.arange(1, 64, 2)], axis=1))


@pytest.mark.parametrize("M", [1, 2, 3, 9000, 100_003])
def test_model_sizes(M, oracle_c):
    """M not a multiple of the tile (512), M <= 2, and M below the seeding grid's minimum (no culling): handle and
    one-shot entry"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M)
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    surf = np.vstack([model[rng.choice(M, min(M, 3000), replace=False)] + rng.normal(0, 0.05, (min(M, 3000), 3)),
                      rng.random((500, 3)) * BOX]).astype(np.float32)
    _check(model, surf, oracle_c)
    idx, dist = pc.knn2_points(surf, model)
    ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist, rd)


def test_queries_outside_the_model_box(oracle_c):
    """blocks that mix a crop with points outside the box (near, far, and so far that they are not scored)"""
    rng = np.random.default_rng(12)
    model = (rng.random((200_000, 3)) * BOX).astype(np.float32)
    crop = _crop(model, 8000, BOX * 0.3, 13)
    near = (rng.random((3000, 3)) * 20 + [105.0, 20.0, 30.0]).astype(np.float32)
    far = crop[:1000] + np.float32(5e3)
    huge = crop[1000:1200].copy(); huge[:, 1] = np.float32(-7e8)
    surf = np.vstack([crop, near, far, huge]).astype(np.float32)
    surf = surf[rng.permutation(len(surf))]
    _check(model, surf, oracle_c)


def test_two_shards_merged_with_idx_base(oracle_c):
    """two prepared shards of one model (rows [0, m1) and [m1, M)), searched with idx_base, merged by (distance, index)"""
    from pcreg_amd.device import HipOps
    rng = np.random.default_rng(14)
    M, m1 = 240_000, 97_301
    model = (rng.random((M, 3)) * BOX).astype(np.float32)
    surf = np.vstack([_crop(model, 10_000, BOX * 0.6, 15), model[:500], model[m1:m1 + 500]]).astype(np.float32)
    parts = [_search(model[:m1], surf, m_lo=0), _search(model[m1:], surf, m_lo=m1)]
    ops = HipOps(len(surf), M, _dev())
    idx_all = torch.from_numpy(np.stack([p[0] for p in parts])).to(_dev())
    dist_all = torch.from_numpy(np.stack([p[1] for p in parts])).to(_dev())
    idx, dist = ops.merge_top2(idx_all, dist_all)
    ri, rd = oracle_c.knn2_points_f32(surf, model, nthreads=CORES)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(dist.cpu().numpy(), rd)
