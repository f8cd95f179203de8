"""The farthest point sampling reference (tests/fps_ref.c) held to the contract of include/pcreg.h without a GPU: on the integer
lattice, where every distance is exact, against an independent float64 numpy restatement of the loop bit for bit; on every family,
the properties the contract promises (no repeats, live rows only, a non-increasing dist, the cover, min_dist / label against a
brute-force nearest-sample search with ties to the earliest sample, the stop rule as the shortest prefix, K > nf)."""
import numpy as np
import pytest

import fps_ref

M, K = 700, 90


def _live(m):
    return np.isfinite(m).all(axis=1)


def _fmaf(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64; the float64 sum is made ROUND-TO-ODD from its two-sum
    error, after which the rounding to float32 (29 bits fewer) is the single rounding of the fused operation"""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _numpy_fps(m, K, start, stop_d2):
    """the contract's loop in float64 numpy, by its text (exact wherever the fp32 arithmetic is exact)"""
    m = m.astype(np.float64)
    live = np.isfinite(m).all(axis=1)
    D = np.where(live, np.inf, np.nan)
    Lb = np.zeros(len(m), np.int64)
    rows = np.flatnonzero(live)
    s = rows[0] if start < 0 else start
    idx, dist, mx = [], [], np.inf
    while True:
        idx.append(s); dist.append(mx)
        d = ((m[rows] - m[s]) ** 2).sum(axis=1)
        lt = d < D[rows]
        D[rows[lt]] = d[lt]; Lb[rows[lt]] = len(idx)
        mx = D[rows].max()
        r = rows[np.flatnonzero(D[rows] == mx)[0]]                # ties: the lowest original row
        if len(idx) == K or not mx > stop_d2:
            break
        s = r
    return np.array(idx), np.array(dist), mx, D, Lb


@pytest.fixture(scope="module")
def runs():
    return {f: (fps_ref.family(f, M), fps_ref.fps(fps_ref.family(f, M), K)) for f in fps_ref.FAMILIES}


@pytest.mark.parametrize("start,stop_d2", [(-1, 0.0), (5, 0.0), (M - 1, 3.0), (-1, float("inf"))])
def test_lattice_equals_the_float64_restatement_bit_for_bit(start, stop_d2):
    m = fps_ref.family("lattice", M)
    for k in (1, 2, K, M + 5):
        r = fps_ref.fps(m, k, start, stop_d2)
        idx, dist, mx, D, Lb = _numpy_fps(m, k, start, stop_d2)
        assert r["info"] == 0 and r["n_out"] == len(idx)
        assert np.array_equal(r["idx"], idx) and np.array_equal(r["dist"].astype(np.float64), dist)
        assert float(r["cover_d2"]) == mx
        assert np.array_equal(r["min_dist"].astype(np.float64), D) and np.array_equal(r["label"], Lb)


def test_lattice_stops_at_the_number_of_distinct_positions():
    m = fps_ref.family("lattice", M)
    r = fps_ref.fps(m, M + 5)
    assert r["n_out"] == len(np.unique(m, axis=0)) == M // 4 and r["cover_d2"] == 0.0
    assert len(np.unique(m[r["idx"]], axis=0)) == r["n_out"]


@pytest.mark.parametrize("fam", fps_ref.FAMILIES)
def test_properties_on_every_family(fam, runs):
    m, r = runs[fam]
    live = _live(m)
    n = r["n_out"]
    assert 1 <= n <= K and r["info"] == 0
    assert len(set(r["idx"].tolist())) == n and live[r["idx"]].all()
    assert r["idx"][0] == np.flatnonzero(live)[0] and r["dist"][0] == np.inf
    assert (r["dist"][2:] <= r["dist"][1:-1]).all()                # (not a difference: +inf may repeat)
    assert r["cover_d2"] <= r["dist"][n - 1]
    # min_dist / label: the nearest sample by brute force in fp32 with the contract's fmaf, ties to the earliest sample
    s = m[r["idx"]]
    with np.errstate(over="ignore", invalid="ignore"):
        d = (m[:, None, :] - s[None, :, :]).astype(np.float32)
        e = _fmaf(d[:, :, 2], d[:, :, 2], _fmaf(d[:, :, 1], d[:, :, 1], d[:, :, 0] * d[:, :, 0]))
    e = e[live]
    near = e.min(axis=1)
    assert np.array_equal(np.isnan(r["min_dist"]), ~live) and (r["label"][~live] == 0).all()
    assert np.array_equal(r["min_dist"][live], near)
    first = np.where(near < np.inf, (e == near[:, None]).argmax(axis=1) + 1, 0)       # (+inf is never below +inf: no label)
    assert np.array_equal(r["label"][live], first)
    assert r["cover_d2"] == near.max()


@pytest.mark.parametrize("fam", fps_ref.FAMILIES)
def test_stop_is_the_shortest_prefix_whose_cover_is_small_enough(fam, runs):
    m, full = runs[fam]
    # the cover after j + 1 samples of the stop_d2 = 0 run is dist[j + 1] (the D the next sample was chosen with)
    for pick in (2, full["n_out"] // 2, full["n_out"] - 1):
        r2 = float(full["dist"][pick])
        if not np.isfinite(r2):
            continue
        r = fps_ref.fps(m, K, -1, r2)
        covers = np.append(full["dist"][1:], full["cover_d2"])    # cover after 1, 2, ... samples
        want = int(np.flatnonzero(~(covers > np.float32(r2)))[0]) + 1
        assert r["n_out"] == want
        assert np.array_equal(r["idx"], full["idx"][:want]) and np.array_equal(r["dist"], full["dist"][:want])
        assert r["cover_d2"] <= np.float32(r2) and (want == 1 or covers[want - 2] > np.float32(r2))


@pytest.mark.parametrize("fam", fps_ref.FAMILIES)
def test_k_above_the_live_count(fam):
    m = fps_ref.family(fam, 130)
    nf = int(_live(m).sum())
    r = fps_ref.fps(m, 130 + 5)
    assert 1 <= r["n_out"] <= nf and len(set(r["idx"].tolist())) == r["n_out"]
    if fam not in ("lattice", "overflow"):
        assert r["n_out"] == nf and r["cover_d2"] == 0.0          # distinct finite rows: every live row ends up a sample


def test_edge_cases_and_the_dead_start():
    m = fps_ref.family("nonfinite", 200)
    r = fps_ref.fps(m, 0)
    assert r["n_out"] == 0 and np.isnan(r["cover_d2"]) and np.isnan(r["min_dist"]).all() and (r["label"] == 0).all() and r["info"] == 0
    r = fps_ref.fps(np.zeros((0, 3), np.float32), 4)
    assert r["n_out"] == 0 and np.isnan(r["cover_d2"]) and r["info"] == 0
    dead = np.full((5, 3), np.nan, np.float32)
    r = fps_ref.fps(dead, 4)
    assert r["n_out"] == 0 and np.isnan(r["cover_d2"]) and np.isnan(r["min_dist"]).all() and (r["label"] == 0).all() and r["info"] == 0
    r = fps_ref.fps(m, 4, 0)                                      # row 0 of this family is dead
    assert r["info"] == 1 and r["n_out"] == 0 and r["cover_d2"] == np.float32(-7.0) and (r["label"] == -7).all()
    r = fps_ref.fps(m, 4, -1, float("inf"))
    assert r["n_out"] == 1 and r["idx"][0] == np.flatnonzero(_live(m))[0]
