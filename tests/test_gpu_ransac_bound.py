"""The staged chain's bounded second pass against the full pass and the oracle.

The staged chain runs for ONE registration of n > 2048 correspondences on the device tier (pcreg_dev_ransac; the host tier
hands the launcher per-registration offsets and takes the batched kernels), so every case here calls pcreg_dev_ransac with
device tensors, a device n and, where given, a device sample table.  pcreg_debug_set("ransac_pass2", 2) forces the bounded
pass and 1 the full pass; both must give the oracle's inlier list, numSuccess and maxInliers, the same transform bits and the
same winner.  The "ransac_stats" counters prove that the bounded kernels ran on one side and not on the other.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rigid_case

pytestmark = pytest.mark.gpu

T_TOL = 1e-5


def _stats(reset=False):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 3)()
    check(lib().pcreg_debug_ransac_stats(out, 1 if reset else 0))
    return list(out)


def _dev_ransac(p1, p2, coef, seed, sample_idx=None, extra_cap=0, ws=None, alloc=None):
    """pcreg_dev_ransac on [3, cap] device tensors with n = len(p1) <= cap on the device.  ws: the caller's (workspace tensor, the
    workspace_bytes to pass) in place of one of the reported size.  alloc(shape, dtype): the caller's allocator of the two outputs
    in place of zeroed tensors."""
    import torch
    from pcreg_amd import _lib
    from pcreg_amd._lib import DevRansacResult, RansacOpts
    from pcreg_amd.device import _p, _stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = len(p1); cap = n + extra_cap
    t1 = torch.zeros(3, cap, dtype=torch.float64, device=dev); t2 = torch.zeros_like(t1)
    t1[:, :n] = torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev); t2[:, :n] = torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)
    nd = torch.tensor([n], dtype=torch.int32, device=dev)
    o = RansacOpts(int(coef["minPtNum"]), int(coef["iterNum"]), float(coef["thDist"]), float(coef["thInlrRatio"]), int(bool(coef["REFINE"])), 0, int(seed))
    si = None if sample_idx is None else torch.from_numpy(np.ascontiguousarray(sample_idx, dtype=np.int32)).to(dev)
    ws, ws_bytes = ws if ws is not None else (torch.empty(L.pcreg_dev_ransac_workspace(cap, o.iterNum), dtype=torch.uint8, device=dev), None)
    alloc = alloc or (lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev))
    res = alloc(C.sizeof(DevRansacResult), torch.uint8); inl = alloc(cap, torch.int32)
    _lib.check(L.pcreg_dev_ransac(_p(t1), _p(t2), _p(nd), cap, cap, C.byref(o), _p(si) if si is not None else None, _p(res), _p(inl),
                                  _p(ws), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes), _stream()))
    r = DevRansacResult.from_buffer_copy(res.cpu().numpy().tobytes())
    return dict(T=np.array(r.T[:]).reshape(4, 4, order="F"), num_success=r.num_success, max_inliers=r.max_inliers, failed=r.failed,
                n=r.n, winner=r.winner, inl=inl[:r.n_inliers].cpu().numpy().astype(np.int64))


def _run_both(p1, p2, coef, debug_set, seed, sample_idx=None, extra_cap=0):
    debug_set("ransac_stats", 1)
    _stats(reset=True)                                               # (returns the counts before the reset)
    debug_set("ransac_pass2", 2)
    bounded = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap)
    s1 = _stats()
    debug_set("ransac_pass2", 1)
    full = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap)
    s2 = _stats()
    debug_set("ransac_pass2", 0)
    auto = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap)
    assert s1[0] == 1, "the bounded pass did not run"
    assert 0 <= s1[1] <= s1[2], s1
    assert s2 == s1, "the forced full pass ran the bounded kernels"
    for k in ("T", "num_success", "max_inliers", "failed", "winner", "inl"):
        np.testing.assert_array_equal(auto[k], full[k], err_msg=k)
    return bounded, full, s1


def _check(bounded, full, ref):
    for name, r in (("bounded", bounded), ("full", full)):
        assert r["failed"] == int(bool(ref["failed"])), name
        if ref["failed"]:
            continue
        assert r["num_success"] == ref["numSuccess"] and r["max_inliers"] == ref["maxInliers"], name
        np.testing.assert_array_equal(r["inl"], ref["inlierIdx"], err_msg=name)
        assert np.linalg.norm(r["T"] - ref["T"]) < T_TOL, name
    for k in ("T", "num_success", "max_inliers", "failed", "winner", "inl", "n"):   # same winner row: same bits
        np.testing.assert_array_equal(bounded[k], full[k], err_msg=k)


def _bench_like(n, seed, outlier_frac=0.03):
    # residuals spread up to the threshold like the bench scene's (thDist 0.3 on squared distances)
    return rigid_case(n, seed, noise=0.12, outlier_frac=outlier_frac)


@pytest.mark.parametrize("n,iters", [(20000, 1500), (32558, 1000)])
def test_bench_like_scene(n, iters, oracle_c, debug_set):
    p1, p2, _ = _bench_like(n, 500 + n)
    coef = dict(minPtNum=3, iterNum=iters, thDist=0.3, thInlrRatio=0.08, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, seed=5)
    assert not ref["failed"] and ref["numSuccess"] > iters // 2
    bounded, full, st = _run_both(p1, p2, coef, debug_set, 5)
    _check(bounded, full, ref)
    assert st[1] < 0.7 * st[2], st                                   # most (refit, block) units were not scanned


def test_ties_at_the_maximum_first_index_wins(oracle_c, debug_set):
    """Every correspondence four times over and a clean motion: many refits share the maximal inlier set (and so the same count);
    the first of them must win in both passes."""
    base1, base2, _ = rigid_case(1500, 77, noise=0.05, outlier_frac=0.1)
    p1 = np.tile(base1, (4, 1)); p2 = np.tile(base2, (4, 1))
    coef = dict(minPtNum=3, iterNum=800, thDist=0.05, thInlrRatio=0.1, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, seed=13)
    c2 = np.asarray(ref["inlrNum_refined"])
    assert (c2 == c2.max()).sum() > 1, "the case must tie at the maximum"
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 13)
    _check(bounded, full, ref)


def test_counts_at_the_success_threshold(oracle_c, debug_set):
    """Refit counts straddle thInlr: a second motion B holds 3000 correspondences, 600 of them offset to squared residuals
    thDist (1 +- 3 %), and every sample is drawn from B's other rows.  thInlr is set to the median refit count, so many refits
    land within a few counts of it on either side and numSuccess is decided at its edge."""
    from oracle import pcreg_oracle as o
    n, nb, ne, th, iters = 9000, 3000, 600, 0.05, 500
    rng = np.random.default_rng(5)
    p1, p2, _ = rigid_case(n, 5, noise=0.02, outlier_frac=0.2)
    R = o.eul2rotm(rng.uniform(-1, 1, 3)); t = rng.uniform(-5, 5, 3)
    B = np.arange(n - nb, n)
    p1[B] = p2[B] @ R + t + rng.normal(0, 2e-3, (nb, 3))
    E = B[:ne]
    v = rng.normal(size=(ne, 3)); v *= (np.sqrt(th * (1.0 + rng.uniform(-0.03, 0.03, ne))) / np.linalg.norm(v, axis=1))[:, None]
    p1[E] += v
    trng = np.random.default_rng(1)
    table = np.stack([trng.choice(B[ne:], 3, replace=False) + 1 for _ in range(iters)]).astype(np.int32)
    coef = dict(minPtNum=3, iterNum=iters, thDist=th, thInlrRatio=0.01, REFINE=True, VERBOSE=0)
    probe = oracle_c.ransac(p1, p2, coef, sample_idx=table, seed=0)
    thInlr = int(np.median(probe["inlrNum_refined"]))
    coef["thInlrRatio"] = thInlr / n
    ref = oracle_c.ransac(p1, p2, coef, sample_idx=table, seed=0)
    c2 = np.asarray(ref["inlrNum_refined"])
    assert (np.abs(c2 - thInlr) <= 3).sum() > 10 and 0 < ref["numSuccess"] < (c2 > 0).sum()
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 0, sample_idx=table)
    _check(bounded, full, ref)


@pytest.mark.parametrize("n,iters,frac", [(6000, 700, 0.85), (4097, 300, 0.6)])
def test_low_inlier_ratio(n, iters, frac, oracle_c, debug_set):
    p1, p2, _ = rigid_case(n, 900 + n, noise=0.02, outlier_frac=frac)
    coef = dict(minPtNum=3, iterNum=iters, thDist=0.05, thInlrRatio=0.05, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, seed=23)
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 23)
    _check(bounded, full, ref)


@pytest.mark.parametrize("n,iters", [(4097, 3), (5001, 17), (8191, 64), (12345, 65), (4607, 129)])
def test_ragged_sizes_and_small_iter_num(n, iters, oracle_c, debug_set):
    """n not a multiple of the 512-correspondence block, fewer refits than seeds, seeds of one refit each."""
    p1, p2, _ = _bench_like(n, 40 + n, outlier_frac=0.2)
    coef = dict(minPtNum=3, iterNum=iters, thDist=0.3, thInlrRatio=0.08, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, seed=29)
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 29)
    _check(bounded, full, ref)


def test_sample_table_and_failures(oracle_c, debug_set):
    """A caller's sample table, with rank-deficient samples (no fit) mixed in."""
    n, iters = 7000, 400
    p1, p2, _ = rigid_case(n, 61, noise=0.05, outlier_frac=0.3)
    rng = np.random.default_rng(4)
    table = np.stack([rng.permutation(n)[:3] + 1 for _ in range(iters)]).astype(np.int32)
    table[::7, 1] = table[::7, 0]                                    # repeated row: no fit
    coef = dict(minPtNum=3, iterNum=iters, thDist=0.1, thInlrRatio=0.1, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, sample_idx=table, seed=0)
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 0, sample_idx=table)
    _check(bounded, full, ref)


def test_device_n_below_capacity_and_repeated_calls(oracle_c, debug_set):
    """n on the device below the capacity, and back-to-back calls on one stream: the pass's counters are cleared by every call."""
    p1, p2, _ = _bench_like(16000, 99)
    coef = dict(minPtNum=3, iterNum=1200, thDist=0.3, thInlrRatio=0.08, REFINE=True, VERBOSE=0)
    ref = oracle_c.ransac(p1, p2, coef, seed=41)
    debug_set("ransac_pass2", 2)
    runs = [_dev_ransac(p1, p2, coef, 41, extra_cap=700) for _ in range(3)]
    bounded, full, _ = _run_both(p1, p2, coef, debug_set, 41, extra_cap=700)
    _check(bounded, full, ref)
    for r in runs:
        for k in ("T", "num_success", "max_inliers", "winner", "inl"):
            np.testing.assert_array_equal(r[k], bounded[k], err_msg=k)
