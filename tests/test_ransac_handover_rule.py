"""The bounded second pass's handover rule in numpy (no GPU): DESIGN 4.9.

A refit is walked block by block under the stop rule (out > n - LB and its success decided -> store thInlr or 0); what is still
undecided after K blocks stores its EXACT count instead (the finish's job on the device).  Whatever the counts, the order of the
rows, LB (the exact count of some refit, or 0) and K, the three quantities the selection takes from the stored counts --
numSuccess = #(cnt >= thInlr), the maximum, the first index that reaches it -- are those of exact counts everywhere.
"""
import numpy as np
import pytest

BLK = 512


def _walk(per_block, sizes, n, lb, th_inlr, hand):
    """Stored count of one refit.  per_block: its inliers in each block of the order; hand: blocks walked before the handover
    (0: never)."""
    nb = len(sizes)
    nbw = hand if hand > 0 and nb > hand else nb
    inl = seen = 0
    for b in range(nbw):
        inl += int(per_block[b]); seen += int(sizes[b])
        out = seen - inl
        if out > n - lb and (inl >= th_inlr or out > n - th_inlr):
            return th_inlr if inl >= th_inlr else 0
    return int(per_block.sum())                       # walked to the end, or handed over: the exact count


def _selection(cnt, exist, th_inlr):
    c = np.where(exist, cnt, -1)
    mx = int(c.max())
    return int((c >= th_inlr).sum()), mx, int(np.argmax(c == mx))


def _scene(rng, iters, n, kind):
    sizes = np.full((n + BLK - 1) // BLK, BLK); sizes[-1] = n - BLK * (len(sizes) - 1)
    top = int(rng.integers(n // 4, n + 1))
    if kind == "ties":                                # many refits share the maximum
        cnt = rng.integers(0, top + 1, iters); cnt[rng.random(iters) < 0.3] = top
    elif kind == "all_tie":
        cnt = np.full(iters, top)
    else:
        cnt = rng.integers(0, top + 1, iters)
    th_inlr = int(rng.integers(0, n + 1))
    if kind == "at_thinlr":                           # counts at the success threshold and one to either side of it
        th_inlr = int(rng.integers(1, max(2, top)))
        edge = rng.random(iters) < 0.5
        cnt[edge] = np.clip(th_inlr + rng.integers(-1, 2, int(edge.sum())), 0, n)
    exist = rng.random(iters) < 0.9
    exist[int(rng.integers(iters))] = True
    # each refit's inliers spread over the blocks of a random order: outliers-first, inliers-first or mixed
    per = np.zeros((iters, len(sizes)), dtype=np.int64)
    for h in range(iters):
        left = int(cnt[h])
        order = {0: np.arange(len(sizes)), 1: np.arange(len(sizes))[::-1], 2: rng.permutation(len(sizes))}[int(rng.integers(3))]
        for b in order:
            free = int(sizes[b])
            rest = int(sizes[order[list(order).index(b) + 1:]].sum())
            lo = max(0, left - rest)
            take = int(rng.integers(lo, min(free, left) + 1)) if int(rng.integers(2)) else min(free, left)
            per[h, b] = take; left -= take
        assert left == 0
    return sizes, cnt, exist, per, th_inlr


@pytest.mark.parametrize("kind", ["random", "ties", "all_tie", "at_thinlr"])
def test_stop_rule_until_k_then_exact_counts_selects_like_exact_counts(kind):
    rng = np.random.default_rng({"random": 1, "ties": 2, "all_tie": 3, "at_thinlr": 4}[kind])
    for trial in range(60):
        iters = int(rng.integers(1, 40))
        n = int(rng.integers(1, 20 * BLK))
        sizes, cnt, exist, per, th_inlr = _scene(rng, iters, n, kind)
        want = _selection(cnt, exist, th_inlr)
        lbs = [0, int(cnt[exist].max()), int(rng.choice(cnt[exist]))]
        for lb in lbs:
            for hand in (0, 1, 4, 8, 16, len(sizes), len(sizes) + 1):
                stored = np.array([_walk(per[h], sizes, n, lb, th_inlr, hand) for h in range(iters)])
                assert _selection(stored, exist, th_inlr) == want, (kind, trial, lb, hand)
                # a refit whose count reaches LB is never stopped: it stores its exact count under every K
                keep = exist & (cnt >= lb)
                np.testing.assert_array_equal(stored[keep], cnt[keep])
