"""pcreg_amd.sweep.promising_clusters' host logic (completeExperimentFast.m:238-248, :266-288) against a float64 restatement
written here; the clustering step is replaced by the CPU reference (tests/cluster_ref.py), so no GPU is needed."""
import numpy as np
import pytest

import cluster_ref


def _sweep_result(seed, n_grid=7, d=5.0, keep=0.5):
    """a synthetic sweep result: sphere centres on a grid of spacing d, a random subset of them tried, random statistics"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    centres = g * d + rng.uniform(-0.01, 0.01, g.shape)
    trial = np.sort(rng.choice(len(centres), int(keep * len(centres)), replace=False))
    n = len(trial)
    putative = rng.integers(120, 400, n)
    inliers = rng.integers(0, 80, n)
    failed = rng.random(n) < 0.1
    transforms = []
    for t in range(n):
        T = np.eye(4)
        T[3, :3] = rng.normal(size=3)
        T[0, 1] = float(t)                                           # (marks which trial a transform came from)
        transforms.append(None if failed[t] else T)
    return dict(centres=centres, trial=trial, statsPutative=putative.astype(np.int64), statsSuccess=rng.integers(0, 5, n).astype(np.int64),
                statsInliers=np.where(failed, 0, inliers).astype(np.int64),
                statsRatio=np.where(failed, 0.0, 100.0 * inliers / putative), transforms=transforms)


def _restated(res, thSucc, thInliers, thRatio, thPutative, r):
    """the script's lines in float64, with a brute-force clustering of the good centres"""
    loc_trial = res["centres"][res["trial"]]
    good = [t for t in range(len(res["trial"])) if res["statsSuccess"][t] >= thSucc and res["statsInliers"][t] >= thInliers and
            res["statsRatio"][t] >= thRatio and res["statsPutative"][t] >= thPutative and res["transforms"][t] is not None]
    loc = loc_trial[good]
    n = len(good)
    label = list(range(n))
    r2 = float(np.float32(r) * np.float32(r))
    changed = True
    while changed:                                                   # label propagation to the smallest row
        changed = False
        for i in range(n):
            for j in range(n):
                if ((loc[i] - loc[j]) ** 2).sum() <= r2 and label[j] < label[i]:
                    label[i] = label[j]
                    changed = True
    out = []
    for c in sorted(set(label)):
        rows = [i for i in range(n) if label[i] == c]
        mean = loc[rows].mean(axis=0)
        # vecnorm(x, 2, 2) as sqrt(x^2 + y^2 + z^2), summed in that order: two centres at (nearly) the same distance from the mean
        # are told apart by the last bit, so the restatement fixes the formula
        dist = [float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) for e in (loc[i] - mean for i in rows)]
        out.append((mean, good[rows[dist.index(min(dist))]]))
    return out


@pytest.fixture
def cpu_clustering(monkeypatch):
    import pcreg_amd.sweep as sw
    calls = []

    def fake(pts, r2):
        calls.append((len(pts), float(r2)))
        return cluster_ref.cluster(pts, r2)
    monkeypatch.setattr(sw, "cluster_points", fake)
    return calls


@pytest.mark.parametrize("seed, th", [(1, (0, 28, 10, 170)), (2, (1, 10, 5, 150)), (3, (0, 40, 12, 200)), (4, (0, 0, 0, 0))])
def test_promising_clusters_equals_the_restatement(cpu_clustering, seed, th):
    from pcreg_amd.sweep import promising_clusters
    res = _sweep_result(seed)
    d = 5.0
    got = promising_clusters(res, *th, d_spheres=d)
    want = _restated(res, *th, 1.6 * d)
    assert len(cpu_clustering) == 1 and cpu_clustering[0][1] == float(np.float32(1.6 * d) * np.float32(1.6 * d))      # ONE clustering call
    assert len(got) == len(want) and len(got) > 1
    for (loc, T), (wloc, wt) in zip(got, want):
        assert loc.dtype == np.float64 and T.shape == (4, 4)
        assert T[0, 1] == float(wt), "the transform of the centre nearest to the mean"
        np.testing.assert_allclose(loc, wloc, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(T, res["transforms"][wt])


def test_an_explicit_radius_and_ties_take_the_first_minimum(cpu_clustering):
    from pcreg_amd.sweep import promising_clusters
    # four centres on a square: all are equally far from the mean, MATLAB's min takes the first
    centres = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0], [100, 0, 0]], np.float64)
    tf = [np.eye(4) * (k + 1) for k in range(5)]
    res = dict(centres=centres, trial=np.arange(5), statsPutative=np.full(5, 200), statsSuccess=np.ones(5), statsInliers=np.full(5, 50),
               statsRatio=np.full(5, 25.0), transforms=tf)
    got = promising_clusters(res, r=4.0)
    assert len(got) == 2
    np.testing.assert_array_equal(got[0][0], [2.0, 2.0, 0.0])
    np.testing.assert_array_equal(got[0][1], tf[0])
    np.testing.assert_array_equal(got[1][0], centres[4])
    np.testing.assert_array_equal(got[1][1], tf[4])
    assert cpu_clustering == [(5, 16.0)]


def test_no_good_sphere_gives_no_cluster(cpu_clustering):
    from pcreg_amd.sweep import promising_clusters
    res = _sweep_result(5)
    assert promising_clusters(res, thInliers=10_000) == []
    empty = dict(centres=np.zeros((0, 3)), trial=np.zeros(0, np.int64), statsPutative=np.zeros(0, np.int64), statsSuccess=np.zeros(0, np.int64),
                 statsInliers=np.zeros(0, np.int64), statsRatio=np.zeros(0), transforms=[])
    assert promising_clusters(empty) == []
    assert cpu_clustering == []                                      # nothing to cluster: no call
