"""The handover of the staged chain's bounded second pass: rs_bounded_kernel walks a refit for kBHand blocks of 512
correspondences, hands what is still undecided to a list, and rs_bfinish_kernel adds the exact counts of the remaining rows.

Every case runs three ways through pcreg_dev_ransac (device n, "ransac_pass2" as in test_gpu_ransac_bound.py): the bounded pass
with the handover ("ransac_bhand" 0, the default), the bounded pass that walks every refit to its stop ("ransac_bhand" 1, the walk
as it was before the handover) and the full pass ("ransac_pass2" 1).  The three must agree bit for bit -- T, winner, num_success,
max_inliers, failed, n, the inlier list -- and with the C oracle.  With "ransac_stats" on, scanned <= full holds in every case and
the finish's own unit counter equals (refits handed over) x (blocks behind the handover): each listed refit is scored over each
remaining block exactly once, by a launch whose grid knows neither n nor the list's length.

kBHand comes from the library (pcreg_debug_ransac_handover's out[2]); the sizes are built from it.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rigid_case
from test_gpu_ransac_bound import _bench_like, _check, _dev_ransac, _stats

pytestmark = pytest.mark.gpu

BLK = 512
KEYS = ("T", "num_success", "max_inliers", "failed", "winner", "inl", "n")


def _handover(reset=False):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 3)()
    check(lib().pcreg_debug_ransac_handover(out, 1 if reset else 0))
    return list(out)


def _k():
    k = _handover()[2]
    assert k >= 4 and k % 4 == 0, k
    return k


def _run3(p1, p2, coef, debug_set, seed, sample_idx=None, extra_cap=0, ws=None):
    """(handover, walk, full, counters of the handover run): st = pcreg_debug_ransac_stats, ho = pcreg_debug_ransac_handover."""
    n, k = len(p1), _k()
    nb = (n + BLK - 1) // BLK
    debug_set("ransac_stats", 1)
    debug_set("ransac_pass2", 2)
    debug_set("ransac_bhand", 0)
    _stats(reset=True); _handover(reset=True)
    hand = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap, ws)
    st, ho = _stats(reset=True), _handover(reset=True)
    debug_set("ransac_bhand", 1)
    walk = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap, ws)
    st_w, ho_w = _stats(reset=True), _handover(reset=True)
    debug_set("ransac_bhand", 0)
    debug_set("ransac_pass2", 1)
    full = _dev_ransac(p1, p2, coef, seed, sample_idx, extra_cap, ws)
    st_f, ho_f = _stats(), _handover()
    debug_set("ransac_pass2", 0)
    print("\nHANDOVER n %d iterNum %d blocks %d kBHand %d: stats %s handed %d finish units %d | walk alone: stats %s"
          % (n, coef["iterNum"], nb, k, st, ho[0], ho[1], st_w))
    assert st[0] == 1 and st_w[0] == 1, "the bounded pass did not run"
    assert 0 <= st[1] <= st[2] and 0 <= st_w[1] <= st_w[2], (st, st_w)
    assert st[2] == st_w[2] and st[2] % nb == 0
    exist = st[2] // nb
    assert ho[1] == ho[0] * max(nb - k, 0), (ho, nb, k)              # each listed refit over each remaining block, once
    assert 0 <= ho[0] <= exist
    if nb <= k:
        assert ho[0] == 0 and st == st_w, "nothing to hand over: the walk as it was"
    assert ho_w[:2] == [0, 0], "the walk alone handed refits over"
    assert st_f == [0, 0, 0] and ho_f[:2] == [0, 0], "the forced full pass ran the bounded kernels"
    for kk in KEYS:
        np.testing.assert_array_equal(hand[kk], full[kk], err_msg="handover against the full pass: " + kk)
        np.testing.assert_array_equal(walk[kk], full[kk], err_msg="walk against the full pass: " + kk)
    return hand, walk, full, dict(st=st, ho=ho, exist=exist, nb=nb, k=k)


def _seeds(ref, iters, n, ratio, exist):
    """The seed refits, from the oracle's first-pass counts: a refit exists where the sample's fit reached thInlr inliers, and a seed
    is the first maximum of those counts among the existing refits of one of min(64, iterNum) slices.  None if the device's
    count of existing refits says otherwise (a fit that failed for another reason)."""
    c1 = np.asarray(ref["inlrNum"])
    ex = c1 >= int(np.floor(ratio * n + 0.5))
    if int(ex.sum()) != exist:
        return None
    S = min(64, iters)
    out = set()
    for s in range(S):
        lo, hi = s * iters // S, (s + 1) * iters // S
        if ex[lo:hi].any():
            out.add(lo + int(np.argmax(np.where(ex[lo:hi], c1[lo:hi], -1))))
    return out


def _oracle_check(hand, walk, full, ref):
    _check(hand, full, ref)
    _check(walk, full, ref)


def _coef(iters, th=0.3, ratio=0.08):
    return dict(minPtNum=3, iterNum=iters, thDist=th, thInlrRatio=ratio, REFINE=True, VERBOSE=0)


@pytest.mark.parametrize("past", [0, 1, 2049], ids=["no_block_behind", "one_row_behind", "ragged_second_workgroup"])
def test_sizes_at_the_handover(past, oracle_c, debug_set):
    """n = kBHand x 512: nothing behind the handover, nothing handed over.  One row more: a block of one row for the finish.
    2049 rows more: a full workgroup of the finish and a second one with a single row."""
    n = _k() * BLK + past
    p1, p2, _ = _bench_like(n, 700 + past, outlier_frac=0.2)
    coef = _coef(200)
    ref = oracle_c.ransac(p1, p2, coef, seed=31)
    hand, walk, full, c = _run3(p1, p2, coef, debug_set, 31)
    _oracle_check(hand, walk, full, ref)
    if past:
        assert c["ho"][0] > 0, "the case must hand refits over"


def test_device_n_far_below_the_capacity(oracle_c, debug_set):
    """The finish's grid covers the capacity: its point-block workgroups past n (two whole ones here) stay idle."""
    n = _k() * BLK + 2049
    p1, p2, _ = _bench_like(n, 811, outlier_frac=0.2)
    coef = _coef(200)
    ref = oracle_c.ransac(p1, p2, coef, seed=37)
    hand, walk, full, c = _run3(p1, p2, coef, debug_set, 37, extra_cap=2 * 2048 + 700)
    _oracle_check(hand, walk, full, ref)
    assert c["ho"][0] > 0


@pytest.mark.parametrize("iters", [3, 33, 64, 65, 70])
def test_small_iter_num(iters, oracle_c, debug_set):
    """Up to 64 refits every refit is a seed (scored in full by rs_bprep_kernel): the list stays empty and the finish's workgroups
    all return at once.  65 and 70: a list shorter than one chunk of 32."""
    n = _k() * BLK + 2049
    p1, p2, _ = _bench_like(n, 40 + n, outlier_frac=0.2)
    coef = _coef(iters)
    ref = oracle_c.ransac(p1, p2, coef, seed=29)
    hand, walk, full, c = _run3(p1, p2, coef, debug_set, 29)
    _oracle_check(hand, walk, full, ref)
    assert c["ho"][0] <= max(iters - 64, 0)
    if iters <= 64:
        assert c["ho"] [0] == 0 and c["st"][1] == c["st"][2], "every refit is a seed"


@pytest.mark.parametrize("iters", [97, 800])
def test_ties_at_the_maximum_are_handed_over_and_the_first_wins(iters, oracle_c, debug_set):
    """test_gpu_ransac_bound.py's tiled scene, 6000 correspondences (12 blocks): the refits that share the maximal inlier set never
    meet out > n - LB, so each of them is a seed (at most 64, one per slice of the refits) or handed over, and the first index
    wins.  97 refits: up to 33 listed, one chunk of the finish and one more."""
    base1, base2, _ = rigid_case(1500, 77, noise=0.05, outlier_frac=0.1)
    p1 = np.tile(base1, (4, 1)); p2 = np.tile(base2, (4, 1))
    assert len(p1) > _k() * BLK
    coef = _coef(iters, th=0.05, ratio=0.1)
    ref = oracle_c.ransac(p1, p2, coef, seed=13)
    c2 = np.asarray(ref["inlrNum_refined"])
    ties = int((c2 == c2.max()).sum())
    assert ties > 1, "the case must tie at the maximum"
    hand, walk, full, c = _run3(p1, p2, coef, debug_set, 13)
    _oracle_check(hand, walk, full, ref)
    seeds = min(64, iters)
    print("TIES iterNum %d: %d refits at the maximum, %d handed over, %d exist" % (iters, ties, c["ho"][0], c["exist"]))
    assert ties - seeds <= c["ho"][0] <= c["exist"]                   # a tie is a seed (at most `seeds` of them) or on the list
    sd = _seeds(ref, iters, len(p1), coef["thInlrRatio"], c["exist"])
    assert sd is not None
    assert c["ho"][0] >= ties - sum(1 for h in sd if c2[h] == c2.max()), "a tie that is no seed was not handed over"
    assert hand["winner"] == int(np.argmax(c2 == c2.max())), "the first index at the maximum must win"


def test_counts_at_the_success_threshold_among_the_handed_over(oracle_c, debug_set):
    """test_gpu_ransac_bound.py's scene of two motions (9000 correspondences, 18 blocks; every sample from motion B's 2400 clean
    rows).  Under a refit of B the 6000 rows of the other motion are outliers, about as many as n - LB, so out > n - LB can first
    hold after block 12: behind the handover.  Every refit that is no seed is therefore handed over, and thInlr is a count that
    several refits have exactly: numSuccess is decided by the finish's exact counts at its edge."""
    from oracle import pcreg_oracle as o
    n, nb_, ne, th, iters = 9000, 3000, 600, 0.05, 500
    assert _k() <= 8
    rng = np.random.default_rng(5)
    p1, p2, _ = rigid_case(n, 5, noise=0.02, outlier_frac=0.2)
    R = o.eul2rotm(rng.uniform(-1, 1, 3)); t = rng.uniform(-5, 5, 3)
    B = np.arange(n - nb_, n)
    p1[B] = p2[B] @ R + t + rng.normal(0, 2e-3, (nb_, 3))
    E = B[:ne]
    v = rng.normal(size=(ne, 3)); v *= (np.sqrt(th * (1.0 + rng.uniform(-0.03, 0.03, ne))) / np.linalg.norm(v, axis=1))[:, None]
    p1[E] += v
    trng = np.random.default_rng(1)
    table = np.stack([trng.choice(B[ne:], 3, replace=False) + 1 for _ in range(iters)]).astype(np.int32)
    coef = _coef(iters, th=th, ratio=0.01)
    probe = oracle_c.ransac(p1, p2, coef, sample_idx=table, seed=0)
    c2 = np.asarray(probe["inlrNum_refined"])
    near = c2[np.abs(c2 - np.median(c2)) <= 3]
    vals, cnts = np.unique(near, return_counts=True)
    thInlr = int(vals[np.argmax(cnts)])                               # the commonest count next to the median
    coef["thInlrRatio"] = thInlr / n
    ref = oracle_c.ransac(p1, p2, coef, sample_idx=table, seed=0)
    c2 = np.asarray(ref["inlrNum_refined"])
    assert (c2 == thInlr).sum() >= 1 and (np.abs(c2 - thInlr) <= 3).sum() > 10 and 0 < ref["numSuccess"] < (c2 > 0).sum()
    hand, walk, full, c = _run3(p1, p2, coef, debug_set, 0, sample_idx=table)
    _oracle_check(hand, walk, full, ref)
    seeds = _seeds(ref, iters, n, coef["thInlrRatio"], c["exist"])
    assert seeds is not None
    assert c["ho"][0] == c["exist"] - len(seeds), "every refit that is no seed is handed over"
    at_edge = [h for h in np.flatnonzero(c2 == thInlr) if h not in seeds and np.asarray(ref["inlrNum"])[h] >= thInlr]
    print("THINLR %d: %d refits at it, %d of them handed over" % (thInlr, int((c2 == thInlr).sum()), len(at_edge)))
    assert at_edge, "no handed-over refit counts exactly thInlr"


def test_band_rows_behind_the_handover(oracle_c, debug_set):
    """Knife-edge rows (test_gpu_ransac_band.py: squared residual thDist (1 +- delta), delta < 5e-7, inside the screen's band) in a
    scene of 16000 correspondences: 30 % far outliers fill the first kBHand blocks of the bounded pass's order (outliers first), the
    inlier-side knife-edge rows follow them in the next bucket, so the finish meets them -- and re-scores their slots in fp64 on
    the raw rows it finds through `perm`.  70 refits: 64 seeds, six handed over that tie at the maximum."""
    from test_gpu_ransac_band import assert_band_rows, build, coef_of, same
    n = 16000
    pairs = [(100, 9000), (5000, 15999), (4095, 4096), (8191, 12288)]
    s = build(n, 1234, pairs, outer=[200, 7777, 12000])
    ref1 = oracle_c.ransac(s["p1"], s["p2"], coef_of(s, 1, True), sample_idx=s["table"])
    assert not ref1["failed"]
    assert_band_rows(s, ref1["T"], oracle_c)
    d = oracle_c.calcDists(ref1["T"], s["p1"], s["p2"])
    assert int((d > 1.01 * s["th"]).sum()) >= _k() * BLK, "the knife-edge rows must lie behind the handover"
    coef = coef_of(s, 70, True)
    ref = oracle_c.ransac(s["p1"], s["p2"], coef, sample_idx=s["table70"])
    hand, walk, full, c = _run3(s["p1"], s["p2"], coef, debug_set, 0, sample_idx=s["table70"])
    bad = []
    for name, r in (("handover", hand), ("walk", walk), ("full", full)):
        same(r, ref, name, bad)
    assert not bad, "\n".join(bad)
    assert np.isin(s["inner"] + 1, hand["inl"]).all(), "an inlier-side knife-edge row is missing from the list"
    assert c["ho"][0] >= 1, "no refit was handed over"


def test_repeated_calls_and_a_dirty_workspace(oracle_c, debug_set):
    """One workspace, filled with 0xFF bytes before its first call, through scenes with a long list, a short one and a long one
    again: rs_stage1_kernel clears the list's length every call, and only the slots below it are read, so stale indices and
    rows of an earlier call (or 0xFF: NaN rows, index -1) decide nothing."""
    import torch
    from pcreg_amd import _lib
    base1, base2, _ = rigid_case(1500, 77, noise=0.05, outlier_frac=0.1)
    t1 = np.tile(base1, (4, 1)); t2 = np.tile(base2, (4, 1))
    coef_t = _coef(800, th=0.05, ratio=0.1)
    n = _k() * BLK + 2049
    b1, b2, _ = _bench_like(n, 40 + n, outlier_frac=0.2)
    coef_b = _coef(70)
    cap = max(len(t1), n)
    L = _lib.lib()
    nbytes = max(L.pcreg_dev_ransac_workspace(cap, 800), L.pcreg_dev_ransac_workspace(cap, 70))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=torch.device("cuda", 0))
    ref_t = oracle_c.ransac(t1, t2, coef_t, seed=13)
    ref_b = oracle_c.ransac(b1, b2, coef_b, seed=29)
    debug_set("ransac_pass2", 2)
    runs = []
    for p1, p2, coef, seed in ((t1, t2, coef_t, 13), (b1, b2, coef_b, 29), (t1, t2, coef_t, 13), (t1, t2, coef_t, 13), (b1, b2, coef_b, 29)):
        runs.append(_dev_ransac(p1, p2, coef, seed, extra_cap=cap - len(p1), ws=(ws, None)))
    debug_set("ransac_pass2", 1)
    full_t = _dev_ransac(t1, t2, coef_t, 13, extra_cap=cap - len(t1))
    full_b = _dev_ransac(b1, b2, coef_b, 29, extra_cap=cap - len(b1))
    debug_set("ransac_pass2", 0)
    for i, full, ref in ((0, full_t, ref_t), (1, full_b, ref_b), (2, full_t, ref_t), (3, full_t, ref_t), (4, full_b, ref_b)):
        _check(runs[i], full, ref)
