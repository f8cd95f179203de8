"""The reference of the trimmed scoring and refits (tests/trim_ref.py), on the CPU: the keep rule on a table, the tie
rule on a hand-made list, and the reason the feature exists stated as a property of the reference -- on partly overlapping
clouds the radius refit stalls and the trimmed one does not."""
import os

import numpy as np

import trim_ref

CORES = min(len(os.sched_getaffinity(0)), 16)


def test_the_keep_rule_on_a_table():
    table = [
        (0.5, 0, 0), (1.0, 0, 0), (1e-6, 0, 0),                            # no pairs: nothing is kept
        (1e-6, 1, 1), (1e-6, 2500, 1), (0.0004, 1000, 1), (0.0001, 4096, 1),  # the max(1, ...) lower bound
        (0.5, 5, 3), (0.7, 5, 4),                                          # exact halves: 2.5 + 0.5 -> 3, 3.5 + 0.5 -> 4
        (0.5, 4, 2), (0.5, 3, 2), (0.5, 1, 1), (0.1, 5, 1), (0.3, 5, 2), (0.25, 2, 1), (0.25, 6, 2),
        (0.6, 2500, 1500), (0.9, 2447, 2202), (0.25, 2447, 612),
        (1.0, 1, 1), (1.0, 5, 5), (1.0, 4194304, 4194304),                 # ratio 1 keeps everything
        (0.999999, 5, 5), (0.89, 5, 4),
    ]
    for ratio, n, want in table:
        assert trim_ref.keep_count(ratio, n) == want, (ratio, n, want)
    for n in range(0, 300):                                                # never more than n, never 0 of some, monotone in the ratio
        last = 0
        for ratio in (1e-6, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0):
            k = trim_ref.keep_count(ratio, n)
            assert (k == 0) == (n == 0) and k <= n and k >= last
            last = k
        assert trim_ref.keep_count(1.0, n) == n


def test_the_tie_rule_on_a_hand_made_list():
    """(d ascending, query ascending): among the pairs at the cut the lowest queries stay"""
    inf = np.inf
    idx = np.array([7, -1, 3, 3, 9, 2, -1, 5, 5, 1], np.int32)
    dist = np.array([2.0, inf, 1.0, 2.0, 0.5, 2.0, inf, 2.0, 3.0, 2.0], np.float32)
    # the order: 4 (0.5), 2 (1.0), then the ties at 2.0 in query order 0, 3, 5, 7, 9, then 8 (3.0)
    order = [4, 2, 0, 3, 5, 7, 9, 8]
    for keep in range(1, 9):
        ratio = (keep - 0.25) / 8
        assert trim_ref.keep_count(ratio, 8) == keep
        i, d, n_within, cut = trim_ref.trim(idx, dist, ratio)
        assert n_within == 8
        assert sorted(np.flatnonzero(i >= 0).tolist()) == sorted(order[:keep]), keep
        assert cut == dist[order[keep - 1]] and cut.dtype == np.float32
        gone = np.setdiff1d(np.arange(10), order[:keep])
        assert (i[gone] == -1).all() and np.isinf(d[gone]).all()
        np.testing.assert_array_equal(i[order[:keep]], idx[order[:keep]])
        np.testing.assert_array_equal(d[order[:keep]], dist[order[:keep]])
    i, d, n_within, cut = trim_ref.trim(np.full(4, -1, np.int32), np.full(4, inf, np.float32), 0.5)      # no pairs
    assert n_within == 0 and np.isinf(cut) and cut > 0 and (i == -1).all()
    i, d, n_within, cut = trim_ref.trim(np.stack([idx, idx]), np.stack([dist, dist]), 0.5)                 # [B, Q]
    assert n_within.tolist() == [8, 8] and cut.tolist() == [2.0, 2.0] and (i[0] == i[1]).all()
    assert sorted(np.flatnonzero(i[0] >= 0).tolist()) == [0, 2, 3, 4]
    i, d, n_within, cut = trim_ref.trim(idx, np.where(idx >= 0, np.float32(inf), dist).astype(np.float32), 0.5)   # every d = +inf: all tie
    assert np.flatnonzero(i >= 0).tolist() == [0, 2, 3, 4] and np.isinf(cut)


def test_trimming_gets_out_of_where_the_radius_stalls():
    """The partial-overlap scene, seed 7, r = 1.5, four steps of the REFERENCE: keeping the closest 0.6 of the pairs ends below 0.01
    RMS from the truth, the radius alone ends above 0.2 (measured when the feature was proposed: 0.0009 and 0.2662, a hundredfold
    margin on each side; properties of the method, not of the library)."""
    sc = trim_ref.overlap_scene(7)
    start = trim_ref.overlap_rms(sc, sc["T0"])
    print(f"start {start:.4f}")
    assert 0.3 < start < 0.4
    out = {}
    for ratio in (None, 0.6):
        ref = trim_ref.overlap_ref(ratio, 4, threads=CORES)
        rms = [trim_ref.overlap_rms(sc, s["T_out"][0]) for s in ref]
        print(f"ratio {ratio}: rms per step {[round(v, 4) for v in rms]}, n_within {[int(s['n_within'][0]) for s in ref]}, "
              f"n_close {[int(s['n_close'][0]) for s in ref]}")
        out[ratio] = rms[-1]
    assert out[0.6] < 0.01
    assert out[None] > 0.2
