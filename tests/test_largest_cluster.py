"""pcreg_amd.sweep.largest_cluster's host logic (completeExperiment.m:379-389) on synthetic sweep results; the clustering step is
replaced by the CPU reference (tests/cluster_ref.py), as tests/test_promising_clusters.py does, so no GPU is needed."""
import numpy as np
import pytest

import cluster_ref


@pytest.fixture
def cpu_clustering(monkeypatch):
    import pcreg_amd.sweep as sw
    calls = []

    def fake(pts, r2):
        calls.append((len(pts), float(r2)))
        return cluster_ref.cluster(pts, r2)
    monkeypatch.setattr(sw, "cluster_points", fake)
    return calls


def _result(centres, trial, failed=(), weak=()):
    """every trial is good (200 putative, 50 inliers, 25 %) except the ordinals in `failed` (no transform) and `weak` (5 inliers)"""
    n = len(trial)
    tf = [None if t in failed else np.eye(4) * (t + 1) for t in range(n)]
    inl = np.array([0 if t in failed else 5 if t in weak else 50 for t in range(n)], np.int64)
    return dict(centres=np.asarray(centres, np.float64), trial=np.asarray(trial, np.int64), statsPutative=np.full(n, 200, np.int64),
                statsSuccess=np.ones(n, np.int64), statsInliers=inl, statsRatio=100.0 * inl / 200.0, transforms=tf)


def test_of_two_clusters_of_equal_size_the_first_wins(cpu_clustering):
    from pcreg_amd.sweep import largest_cluster
    # spheres 0..7; sphere 1 is never tried.  Trials: spheres [6, 0, 2, 7, 3, 5]; near x = 0: spheres 0, 2, 3; near x = 100: 6, 7, 5
    centres = [[0, 0, 0], [50, 0, 0], [4, 0, 0], [8, 0, 0], [200, 0, 0], [108, 0, 0], [100, 0, 0], [104, 0, 0]]
    res = _result(centres, [6, 0, 2, 7, 3, 5])
    trials, spheres = largest_cluster(res, d_spheres=5.0)
    # both clusters hold three trials; the one with the smallest first row (trial 0: sphere 6) is first
    np.testing.assert_array_equal(trials, [0, 3, 5])
    np.testing.assert_array_equal(spheres, [6, 7, 5])
    assert trials.dtype == np.int64 and spheres.dtype == np.int64
    assert cpu_clustering == [(6, float(np.float32(8.0) * np.float32(8.0)))]                     # ONE clustering call, r = 1.6 d
    # a fourth member makes the other cluster the largest
    res = _result(centres + [[12, 0, 0]], [6, 0, 2, 7, 3, 5, 8])
    trials, spheres = largest_cluster(res, d_spheres=5.0)
    np.testing.assert_array_equal(trials, [1, 2, 4, 6])
    np.testing.assert_array_equal(spheres, [0, 2, 3, 8])


def test_a_failed_or_weak_trial_is_never_a_member(cpu_clustering):
    from pcreg_amd.sweep import largest_cluster, promising_clusters
    centres = [[0, 0, 0], [4, 0, 0], [8, 0, 0], [12, 0, 0], [100, 0, 0], [104, 0, 0]]
    res = _result(centres, [0, 1, 2, 3, 4, 5], failed=(1,), weak=(2,))
    # without trials 1 and 2 the chain 0 - 4 - 8 - 12 falls apart (gaps of 12 > r = 8): {0}, {3}, {4, 5}
    trials, spheres = largest_cluster(res, d_spheres=5.0)
    np.testing.assert_array_equal(trials, [4, 5])
    np.testing.assert_array_equal(spheres, [4, 5])
    # the thresholds and the clustering are those of promising_clusters
    assert len(promising_clusters(res, d_spheres=5.0)) == 3
    assert cpu_clustering[0] == cpu_clustering[1]
    # with the thresholds lowered the weak trial joins and links 0 - 8 - 12: {0, 2, 3} and {4, 5}
    trials, _ = largest_cluster(res, thInliers=5, thRatio=2, d_spheres=5.0)
    np.testing.assert_array_equal(trials, [0, 2, 3])
    # an explicit radius
    trials, _ = largest_cluster(res, r=12.5)
    np.testing.assert_array_equal(trials, [0, 3])


def test_no_good_sphere_gives_empty_lists(cpu_clustering):
    from pcreg_amd.sweep import largest_cluster
    res = _result([[0, 0, 0], [4, 0, 0]], [0, 1])
    trials, spheres = largest_cluster(res, thInliers=10_000)
    assert len(trials) == 0 and len(spheres) == 0 and trials.dtype == np.int64
    empty = dict(centres=np.zeros((0, 3)), trial=np.zeros(0, np.int64), statsPutative=np.zeros(0, np.int64), statsSuccess=np.zeros(0, np.int64),
                 statsInliers=np.zeros(0, np.int64), statsRatio=np.zeros(0), transforms=[])
    trials, spheres = largest_cluster(empty)
    assert len(trials) == 0 and len(spheres) == 0
    assert cpu_clustering == []                                      # nothing to cluster: no call
