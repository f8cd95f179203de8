"""Candidate transforms scored against a prepared model (knn_score.hip) on the GPU, bit for bit.

idx, the distance bits and n_close against tests/score_ref.py (numpy float64 transformed queries, the brute-force fp32 nearest
row, the `<= r2` filter); sum_d2 against math.fsum within the bound of any summation order; every case again with culling off
("knn_nocull"), with the eight transforms in three batches ("score_batch_slots") and a second time as it is: the same bits, sum_d2
included.  Then the edges (M, B * Q, Q = 0, B = 0, ldq > Q, no rows asked for, a query on a tile box's face, argument errors, the
workspace formula), the visited share at the bench shape, two streams on one handle, the host tier and score_trials."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import score_ref as ref
from test_gpu_range import _bits, _dev, _family, _prepared, _soa, _stats

pytestmark = pytest.mark.gpu
CORES = min(len(os.sched_getaffinity(0)), 16)
RADII = [np.float32(0.0), np.float32(0.1) ** 2, np.float32(0.5) ** 2, np.float32(1.5) ** 2, np.float32(np.inf)]


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _transforms(model, seed=5):
    """the eight: identity, a small rotation and shift, a large rigid motion that throws the cloud out of the model's box, a shift
    of 7e8, a reflection (z mirrored about the model's middle), a non-rigid matrix, all zeros, a NaN entry"""
    rng = np.random.default_rng(seed)
    mid = (model.min(axis=0).astype(np.float64) + model.max(axis=0)) / 2 if len(model) else np.zeros(3)
    ext = float(np.ptp(model, axis=0).max()) if len(model) else 1.0
    T = np.tile(np.eye(4), (8, 1, 1))
    a = np.array([0.004, -0.003, 0.005])
    T[1, :3, :3] += np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T[1, 3, :3] = [0.05, -0.04, 0.03]
    T[2, :3, :3] = _rot(rng)
    T[2, 3, :3] = 30.0 * ext + rng.normal(size=3)
    T[3, 3, :3] = [7e8, 0.0, 0.0]
    T[4, 2, 2], T[4, 3, 2] = -1.0, 2.0 * mid[2]
    T[5, :3, :3] = np.diag([1.02, 0.97, 1.01]) + 0.01 * rng.normal(size=(3, 3))
    T[5, 3, :3] = -0.01 * mid
    T[6] = 0.0
    T[7, 1, 2] = np.nan
    return T


def _t16(T):
    """[B, 4, 4] -> the [B, 16] block on the device, each transform column-major"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    return torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)).to(_dev())


def _score(pm, q, Td, r2, rows=True):
    out = pm.score_transforms(q, Td, r2, rows=rows)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same(a, b):
    """idx, dist, n_close and the BITS of sum_d2"""
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    if len(a) > 2:
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_array_equal(_bits(a[3]), _bits(b[3]))


def _check(got, nn, r2, Q):
    """against the reference: idx, dist, n_close exactly; sum_d2 within (Q - 1) 2^-53 fsum, the bound of ANY order of summation of
    non-negative terms (each of the Q - 1 additions rounds a partial sum that is at most the total, by at most 2^-53 of it)"""
    n_close, sum_d2, idx, dist = got
    ri, rd = ref.within(nn[0], nn[1], r2)
    B = len(n_close)
    ri, rd = ri.reshape(B, Q), rd.reshape(B, Q)
    rn, rs = ref.sums(ri, rd)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and n_close.dtype == np.int32 and sum_d2.dtype == np.float64
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(_bits(dist), _bits(rd))
    np.testing.assert_array_equal(n_close, rn)
    for b in range(B):
        print(f"  b = {b}: n_close {n_close[b]}, sum_d2 {sum_d2[b]!r}, fsum {rs[b]!r}")
        if np.isfinite(rs[b]):
            assert abs(sum_d2[b] - rs[b]) <= max(Q - 1, 0) * 2.0 ** -53 * rs[b], (b, sum_d2[b], rs[b])
        else:
            assert sum_d2[b] == rs[b], (b, sum_d2[b], rs[b])
    return rn


_CASE = {}


def _case(name):
    """(model, surf, T, nearest): the family's clouds (500 model rows copied into the surface: exact hits under the identity), the
    eight transforms, and the reference's nearest row of every transformed query, computed once for all radii"""
    if name in _CASE:
        return _CASE[name]
    if name == "synth":
        from bench import synth
        model, surf, _ = synth(120_000, 3000)
        surf = surf[:2500]
    else:
        model, surf = _family(name)
        surf = surf[np.sort(np.random.default_rng(2).choice(len(surf), 1000, replace=False))]
    model, surf = np.asarray(model, np.float32), np.asarray(surf, np.float32)
    own = np.random.default_rng(4).choice(len(model), 500, replace=False)
    surf = np.vstack([surf, model[own]]).astype(np.float32)
    T = _transforms(model)
    nn = ref.nearest(ref.transformed(surf, T).reshape(-1, 3), model, threads=CORES)
    _CASE[name] = (model, surf, T, nn)
    return _CASE[name]


@pytest.mark.parametrize("name", ["synth", "duplicates", "sheet", "outside"])
def test_families_equal_the_reference_with_culling_off_in_three_batches_and_twice(name, debug_set):
    model, surf, T, nn = _case(name)
    Q = len(surf)
    pm, _t = _prepared(model)
    q, Td = _soa(surf), _t16(T)
    try:
        debug_set("knn_stats", 1)
        seen = []
        for r2 in RADII:
            _stats(reset=True)
            got = _score(pm, q, Td, r2)
            st = _stats(reset=True)
            print(f"{name}: r2 = {float(r2):.6g}: visited {st[1]} of {st[2]}")
            n = _check(got, nn, r2, Q)
            seen.append(n)
            assert st[0] == 1 and st[2] == ((8 * Q + 511) // 512) * ((len(model) + 511) // 512), st
            _same(_score(pm, q, Td, r2), got)                      # two identical calls
            _stats(reset=True)
            debug_set("knn_nocull", 1)
            g0 = _score(pm, q, Td, r2)
            st0 = _stats(reset=True)
            debug_set("knn_nocull", 0)
            assert st0[1] == st0[2] == st[2], (st0, st)            # every (block, tile) pair visited
            _stats(reset=True)
            debug_set("score_batch_slots", 3 * Q)
            g1 = _score(pm, q, Td, r2)
            st1 = _stats(reset=True)
            debug_set("score_batch_slots", 0)
            assert st1[0] == 3, st1                                # premise: 3 + 3 + 2 transforms
            _same(g0, got)
            _same(g1, got)
            _same(_score(pm, q, Td, r2, rows=False), got[:2])      # no rows asked for: the same counts and sums
            assert (got[0][6:] == 0).all() and (got[1][6:] == 0).all()          # the empty transform and the NaN entry
        seen = np.array(seen)
        # premises: r2 = 0 finds the copied rows under the identity, exactly; at one radius both outcomes occur
        assert seen[0, 0] >= 500 and (seen[0, [1, 2, 3, 5, 6, 7]] == 0).all(), seen[0]         # (the sheet is its own mirror image)
        assert (seen[4, :6] == Q).all(), seen[4]
        assert seen[3, 2] == 0 and seen[3, 3] == 0 and seen[3, 0] > 500, seen[3]
        if name == "synth":
            # none, a handful, a few hundred and all of the rows, each at some (radius, transform)
            assert seen[3, 0] == Q and seen[3, 1] == Q and 0 < seen[1, 1] < 100 and 100 < seen[2, 4] < 1500, seen
        if name == "duplicates":                                   # every row three times: the lowest of the three
            idx0 = _score(pm, q, Td, 0.0)[2][0, -500:]
            np.testing.assert_array_equal(model[idx0], surf[-500:])
            first = np.array([np.flatnonzero((model == p).all(axis=1))[0] for p in surf[-20:]])
            np.testing.assert_array_equal(idx0[-20:], first)
    finally:
        pm.close()


def _edge_transforms():
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1, 3, :3] = [0.3, -0.2, 0.1]
    T[2, :3, :3] = _rot(np.random.default_rng(9))
    return T


def test_small_models_and_slot_counts(debug_set):
    """M around a tile of 512 rows and around 16 384; B * Q around the 64 queries of a workgroup, the 512 slots of a block and the
    2048 queries of a reduce chunk, with one transform and with three (totals that 3 divides, and 66 and 510 from the other side
    of their boundaries)"""
    rng = np.random.default_rng(12)
    shapes = [(1, n) for n in (1, 63, 64, 65, 511, 512, 513, 2049)] + [(3, n) for n in (21, 22, 170, 171, 683)]
    T = _edge_transforms()
    for M in (0, 1, 511, 512, 513, 16_383, 16_384):
        model = (rng.random((M, 3)) * 20).astype(np.float32)
        pm, _t = _prepared(model)
        try:
            hits = 0
            for B, Q in shapes:
                surf = (rng.random((Q, 3)) * 22 - 1).astype(np.float32)
                if M:
                    surf[0] = model[M // 2]
                nn = ref.nearest(ref.transformed(surf, T[:B]).reshape(-1, 3), model, threads=CORES)
                for r2 in (0.0, 1.0, np.inf):
                    got = _score(pm, _soa(surf), _t16(T[:B]), r2)
                    hits += int(_check(got, nn, r2, Q).sum())
                    if B == 3:
                        debug_set("score_batch_slots", Q)          # one transform a batch
                        _same(_score(pm, _soa(surf), _t16(T[:B]), r2), got)
                        debug_set("score_batch_slots", 0)
                    if M == 0:
                        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == -1).all() and np.isposinf(got[3]).all()
            assert (hits > 0) == (M > 0)
        finally:
            pm.close()


def test_no_queries_no_transforms_and_a_wider_buffer():
    rng = np.random.default_rng(13)
    model = (rng.random((5000, 3)) * 20).astype(np.float32)
    surf = (rng.random((300, 3)) * 22 - 1).astype(np.float32)
    T = _edge_transforms()
    pm, _t = _prepared(model)
    try:
        n, s, idx, dist = _score(pm, _soa(surf[:0]), _t16(T), 1.0)
        assert n.tolist() == [0, 0, 0] and s.tolist() == [0.0, 0.0, 0.0] and idx.shape == (3, 0) and dist.shape == (3, 0)
        n, s, idx, dist = _score(pm, _soa(surf), _t16(T[:0]), 1.0)
        assert n.shape == (0,) and s.shape == (0,) and idx.shape == (0, 300)
        # B = 0 through the C ABI: nothing is written
        from pcreg_amd._lib import check, lib
        L = lib()
        q = _soa(surf)
        guard = torch.full((4,), -7, dtype=torch.int32, device=_dev())
        ws = torch.empty(int(L.pcreg_dev_model_score_workspace(300, 0, pm.M)), dtype=torch.uint8, device=_dev())
        check(L.pcreg_dev_model_score_f32(pm.handle, q.data_ptr(), 300, 300, None, 0, 1.0, guard.data_ptr(), None, guard.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(), None))
        torch.cuda.synchronize()
        assert guard.tolist() == [-7] * 4
        # ldq > Q: the queries are columns 100 .. 399 of a wider buffer
        wide = torch.full((3, 1000), 1e30, dtype=torch.float32, device=_dev())
        wide[:, 100:400] = q
        qw = wide[:, 100:400]
        assert qw.stride(0) == 1000 and qw.shape[1] == 300
        nn = ref.nearest(ref.transformed(surf, T).reshape(-1, 3), model, threads=CORES)
        got = _score(pm, qw, _t16(T), 2.0)
        assert _check(got, nn, 2.0, 300).sum() > 100
        _same(_score(pm, q, _t16(T), 2.0), got)
    finally:
        pm.close()


def test_a_query_on_a_tile_box_face_with_r2_equal_to_a_distance(debug_set):
    """tests/test_gpu_range.py's two-tile model: tile 1's box begins at the lone row (7, 1.5, 1.5).  (7, 2, 2) lies ON that face,
    0.5 from the lone row; (6, 1.5, 1.5) is 1 from the box AND 1 from the lone row: a gap equal to r2 must not be skipped.  One
    query a call, so the block's box is the query."""
    rng = np.random.default_rng(8)
    near = (rng.random((511, 3)) * 2.5 + 0.5).astype(np.float32)
    far = np.column_stack([rng.uniform(10, 12, 100), rng.uniform(0.5, 3, 100), rng.uniform(0.5, 3, 100)]).astype(np.float32)
    model = np.vstack([[[400, 400, 400]], far, [[7.0, 1.5, 1.5]], near, [[0, 0, 0]]]).astype(np.float32)
    lone = 101
    pm, _t = _prepared(model)
    try:
        from pcreg_amd._lib import check, lib
        tbox = torch.empty((2, 6), dtype=torch.float32, device=_dev())
        prep = (C.c_float * 24)()
        check(lib().pcreg_debug_dev_model_export(pm.handle, None, None, tbox.data_ptr(), prep, None))
        torch.cuda.synchronize()
        tb = tbox.cpu().numpy()
        assert tb[1, 0] == 7.0 and tb[1, 1] <= 1.5 and tb[1, 4] >= 2.0 and tb[0, 3] < 6.0, tb      # premise: the face x = 7 of tile 1
        debug_set("knn_stats", 1)
        I = _t16(np.eye(4)[None])
        for p, r2, want in (((7.0, 2.0, 2.0), 0.5, lone), ((7.0, 2.0, 2.0), np.nextafter(np.float32(0.5), np.float32(0)), -1),
                            ((6.0, 1.5, 1.5), 1.0, lone), ((6.0, 1.5, 1.5), np.nextafter(np.float32(1.0), np.float32(0)), -1)):
            surf = np.array([p], np.float32)
            _stats(reset=True)
            got = _score(pm, _soa(surf), I, r2)
            st = _stats(reset=True)
            nn = ref.nearest(surf, model)
            _check(got, nn, r2, 1)
            assert nn[0][0] == lone and nn[1][0] == np.float32(0.5 if p[0] == 7.0 else 1.0)
            assert got[2][0, 0] == want and st[2] == 2 and st[1] == 1, (p, r2, got, st)      # tile 1 walked, tile 0 (> 3 away) skipped
    finally:
        pm.close()


def test_argument_errors_and_the_workspace_formula():
    from pcreg_amd._lib import PCREG_E_ARG, PCREG_OK, lib
    L = lib()
    rng = np.random.default_rng(14)
    model = (rng.random((700, 3)) * 20).astype(np.float32)
    pm, _t = _prepared(model)
    try:
        q, Td = _soa(model[:40]), _t16(_edge_transforms())
        n = torch.zeros(3, dtype=torch.int32, device=_dev())
        s = torch.zeros(3, dtype=torch.float64, device=_dev())
        need = int(L.pcreg_dev_model_score_workspace(40, 3, pm.M))
        ws = torch.empty(need, dtype=torch.uint8, device=_dev())

        def call(Q=40, ldq=40, B=3, r2=1.0, wsb=need, qp=q.data_ptr(), tp=Td.data_ptr(), h=pm.handle):
            return L.pcreg_dev_model_score_f32(h, qp, Q, ldq, tp, B, r2, n.data_ptr(), s.data_ptr(), None, None, ws.data_ptr(), wsb, None)
        assert call() == PCREG_OK
        for kw in (dict(r2=float("nan")), dict(r2=-1.0), dict(r2=float("-inf")), dict(Q=(4 << 20) + 1, ldq=(4 << 20) + 1, wsb=1 << 40),
                   dict(B=-1), dict(Q=-1), dict(ldq=39), dict(wsb=need - 1), dict(qp=None), dict(tp=None), dict(h=None)):
            assert call(**kw) == PCREG_E_ARG, kw
            assert b"bad argument" in L.pcreg_last_error()
        assert call(r2=float("inf")) == PCREG_OK and call(r2=0.0) == PCREG_OK
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            pm.score_transforms(q, Td, -1.0)
        with pytest.raises(TypeError):
            pm.score_transforms(q, Td.float(), 1.0)
    finally:
        pm.close()
    # include/pcreg.h: nb = max(1, min(B, floor(4 Mi / max(Q, 1)))), S = max(nb Q, 1), P = nb max(ceil(Q / 2048), 1);
    # 131 328 + roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256)
    up = lambda x: (x + 255) // 256 * 256
    for Q, B in ((0, 0), (1, 1), (3000, 8), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        nb = max(1, min(B, (4 << 20) // max(Q, 1)))
        S, P = max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)
        want = 131_328 + up(12 * S) + 2 * up(4 * S) + up(8 * P) + up(4 * P)
        assert L.pcreg_dev_model_score_workspace(Q, B, 0) == L.pcreg_dev_model_score_workspace(Q, B, 1 << 20) == want, (Q, B)
        assert want <= 131_328 + 24 * (4 << 20) + 13 * nb + 5 * 256


def test_culling_is_real_at_the_bench_shape(debug_set):
    """synth(1 000 000, 50 000) under the eight transforms at r = 1.5: fewer tiles listed than (block, tile) pairs.  The whole
    result equals the walk with culling off (every tile visited: the brute force on the device), and 2000 sampled (b, i) pairs
    equal the reference."""
    from bench import synth
    model, surf, _ = synth(1_000_000, 50_000)
    model, surf = np.asarray(model, np.float32), np.asarray(surf, np.float32)
    T = _transforms(model)
    r2 = np.float32(1.5) ** 2
    pm, _t = _prepared(model)
    q, Td = _soa(surf), _t16(T)
    Q = len(surf)
    try:
        debug_set("knn_stats", 1)
        _stats(reset=True)
        got = _score(pm, q, Td, r2)
        st = _stats(reset=True)
        print(f"bench shape, 8 transforms, r = 1.5: listed {st[1]} of {st[2]} (block, tile) pairs = {st[1] / st[2]:.4f}; n_close {got[0].tolist()}")
        assert st[0] == 1 and st[2] == ((8 * Q + 511) // 512) * ((len(model) + 511) // 512) and st[3] == 0, st
        assert st[1] < st[2]
        debug_set("knn_nocull", 1)
        g0 = _score(pm, q, Td, r2)
        debug_set("knn_nocull", 0)
        _same(g0, got)
        assert got[0][0] > Q // 2 and got[0][2] == 0 and got[0][3] == 0 and got[0][6] == 0 and got[0][7] == 0, got[0]
        pick = np.sort(np.random.default_rng(6).choice(6 * Q, 2000, replace=False))        # (the last two transforms' queries are NaN)
        tq = ref.transformed(surf, T).reshape(-1, 3)[pick]
        ri, rd = ref.within(*ref.nearest(tq, model, threads=CORES), r2)
        np.testing.assert_array_equal(got[2].reshape(-1)[pick], ri)
        np.testing.assert_array_equal(_bits(got[3].reshape(-1)[pick]), _bits(rd))
        assert (ri >= 0).any() and (ri < 0).any()
    finally:
        pm.close()


def test_two_streams_the_host_tier_and_score_trials():
    import pcreg_amd as pc
    from pcreg_amd._lib import lib
    from pcreg_amd.sweep import score_trials
    model, surf, T, nn = _case("synth")
    Q = len(surf)
    r2 = np.float32(0.5) ** 2
    pm, _t = _prepared(model)
    L = lib()
    try:
        q, Td = _soa(surf), _t16(T)
        got = _score(pm, q, Td, r2)
        _check(got, nn, r2, Q)
        # the host tier, bit for bit
        with pc.Model(model) as h:
            r = h.score_transforms(surf, T, r2, rows=True)
            r_sums = h.score_transforms(surf, list(T[:6]) + [None, T[7]], r2)
        _same((r["n_close"], r["sum_d2"], r["idx"], r["dist"]), got)
        _same((r_sums["n_close"], r_sums["sum_d2"]), got[:2])
        assert "idx" not in r_sums
        np.testing.assert_array_equal(r["fitness"], got[0] / Q)
        np.testing.assert_array_equal(r["rmse"][:2], np.sqrt(got[1][:2] / got[0][:2]))
        assert np.isnan(r["rmse"][6:]).all()
        # two streams on one handle, each call with its own workspace and outputs
        halves = ((q[:, :2000].contiguous(), Td[:5].contiguous()), (q[:, 1000:].contiguous(), Td[3:].contiguous()))
        want = [_score(pm, a, b, r2) for a, b in halves]
        outs = []
        for a, b in halves:
            Qh, Bh = a.shape[1], b.shape[0]
            outs.append((torch.empty(Bh, dtype=torch.int32, device=_dev()), torch.empty(Bh, dtype=torch.float64, device=_dev()),
                         torch.empty((Bh, Qh), dtype=torch.int32, device=_dev()), torch.empty((Bh, Qh), dtype=torch.float32, device=_dev()),
                         torch.empty(int(L.pcreg_dev_model_score_workspace(Qh, Bh, pm.M)), dtype=torch.uint8, device=_dev())))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(3):
            for s, (a, b), o in ((s1, halves[0], outs[0]), (s2, halves[1], outs[1])):
                with torch.cuda.stream(s):
                    pm.score_transforms(a, b, r2, rows=True, out=o)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            _same(tuple(t.cpu().numpy() for t in o[:4]), w)
        # score_trials: ransac's transforms map the model onto the surface, so the sweep's entry is invertTF of ours; one failed
        rigid = [T[0], T[1], T[2]]
        result = dict(trial=np.array([4, 9, 11, 30]), transforms=[pc.invertTF(rigid[0]), None, pc.invertTF(rigid[1]), pc.invertTF(rigid[2])])
        sc = score_trials(result, pm, q, 0.5)
        inv = np.stack([pc.invertTF(np.asarray(t)) if t is not None else np.zeros((4, 4)) for t in result["transforms"]])
        ri, rd, rn, rs = ref.score(surf, model, inv, r2, threads=CORES)
        np.testing.assert_array_equal(sc["n_close"], rn)
        assert sc["n_close"][1] == 0 and sc["sum_d2"][1] == 0.0 and sc["n_close"][0] > 0 and len(sc["fitness"]) == len(result["trial"])
        assert np.all(np.abs(sc["sum_d2"] - rs) <= (Q - 1) * 2.0 ** -53 * rs)
        np.testing.assert_array_equal(sc["fitness"], rn / Q)
        ok = rn > 0
        np.testing.assert_array_equal(sc["rmse"][ok], np.sqrt(sc["sum_d2"][ok] / rn[ok]))
        assert np.isnan(sc["rmse"][~ok]).all()
    finally:
        pm.close()
