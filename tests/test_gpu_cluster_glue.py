"""The link from the sphere sweep to the final stage on the GPU: pcreg_amd.sweep.promising_clusters on a synthetic sweep result
(completeExperimentFast.m:238-288, the clustering through the library's own call) gives the cluster list a hand-built call of
FinalStage.run takes, and the final stage gives the same answer for both."""
import numpy as np
import pytest

from test_gpu_descriptors import OPT, keypoints
from test_gpu_final_stage import PAR, _perturbed, _scene

pytestmark = pytest.mark.gpu


def test_promising_clusters_feed_the_final_stage(oracle_c, oracle_py):
    import torch
    from pcreg_amd.device import soa
    from pcreg_amd.sweep import FinalStage, promising_clusters
    model, surface, kpM, T_true = _scene(5)
    featM, descM = oracle_c.getSpacialHistogramDescriptors(model, kpM, dict(OPT, ALIGN_POINTS=False))
    rng = np.random.default_rng(9)
    d = 5.0
    T_a = [_perturbed(T_true, rng, 0.004, 0.03) for _ in range(3)]
    T_wrong = np.eye(4); T_wrong[:3, :3] = oracle_py.eul2rotm(np.array([1.2, 0.4, -0.7])); T_wrong[3, :3] = [10.0, 5.0, -4.0]
    # sphere centres of the sweep: three neighbours on the grid around the right place (one cluster, its middle centre is nearest
    # to the mean), one good centre far from them (a cluster of its own), one trial with too few inliers, one failed trial,
    # and two centres that were never tried
    centres = np.array([[20.0, 18.0, 12.0], [0.0, 0.0, 0.0], [25.0, 18.0, 12.0], [30.0, 18.0, 12.0], [12.0, 40.0, 11.0], [25.0, 23.0, 12.0],
                        [60.0, 60.0, 60.0], [27.0, 18.0, 14.0]])
    trial = np.array([0, 2, 3, 4, 5, 7])
    result = dict(centres=centres, trial=trial, transforms=[T_a[0], T_a[1], T_a[2], T_wrong, T_true, None],
                  statsPutative=np.array([300, 280, 260, 200, 400, 250]), statsSuccess=np.array([3, 5, 2, 1, 0, 0]),
                  statsInliers=np.array([60, 90, 40, 30, 12, 0]), statsRatio=np.array([20.0, 32.1, 15.4, 15.0, 3.0, 0.0]))
    clusters = promising_clusters(result, d_spheres=d)
    by_hand = [(np.array([25.0, 18.0, 12.0]), T_a[1]), (np.array([12.0, 40.0, 11.0]), T_wrong)]
    assert len(clusters) == 2
    for (loc, T), (wloc, wT) in zip(clusters, by_hand):
        np.testing.assert_allclose(loc, wloc, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(T, wT)
    assert promising_clusters(result, thInliers=1000) == []
    near = kpM[(kpM[:, 0] > 10) & (kpM[:, 0] < 40)]
    kps = []
    for loc, T in by_hand:
        moved = oracle_py.quickTF(surface, oracle_py.invertTF(T))
        kps.append(np.vstack([oracle_py.pcRandomUniformSamples(moved, 3.0, 3.5, rng)[:300], near + rng.normal(0, 0.05, near.shape)]))
    dev = torch.device("cuda", 0)
    fs = FinalStage(soa(torch.from_numpy(surface).to(dev)), featM, descM, device=dev)
    got = fs.run(clusters, kps, OPT, PAR, 14.0, maxDist=1.5)
    want = fs.run(by_hand, kps, OPT, PAR, 14.0, maxDist=1.5)
    assert got["best"] == want["best"] == 0 and got["T_refine"] is not None
    np.testing.assert_array_equal(got["num_close"], want["num_close"])
    np.testing.assert_array_equal(got["num_keypoints"], want["num_keypoints"])
    for a, b in zip(got["matches"], want["matches"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(got["T_refine"], want["T_refine"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got["pts_final"].cpu().numpy(), want["pts_final"].cpu().numpy(), rtol=0, atol=1e-9)
