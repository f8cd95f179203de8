"""SphereSweep.aggregate -- completeExperiment.m:379-458 on the buffers a sweep leaves on the device -- against
tests/unique_rows_ref.aggregated_stage_ref on the same sweep result: the largest cluster of promising spheres, its stacked
matches made unique twice, ONE ransac, estimateTransform over its inliers; one host synchronisation.

The scene is that of tests/test_gpu_sweep.py (seed 0, VM 6000, VS 260, D 96), restated, with descriptor noise poisson(3.0) and
Unique=False, so that a surface keypoint is matched in many spheres (the first unique removes rows) and several surface keypoints
share a model keypoint (the second one does too)."""
import numpy as np
import pytest

from unique_rows_ref import aggregated_stage_ref

pytestmark = pytest.mark.gpu

PAR = dict(UNNORMALIZE=True, norm_factor=2, CHANGE_METRIC=True, metric_factor=0.6, Method="Approximate",
           MatchThreshold=10, MaxRatio=0.99, Metric="SAD", Unique=False, VERBOSE=0)
OPT = dict(minPtNum=3, iterNum=1500, thDist=0.3, thInlrRatio=0.08, REFINE=True, VERBOSE=0)
KW = dict(R_desc=9.0, d_spheres=6.0, min_pts=500, putative_thresh=40, seed=3)
TH = dict(thInliers=28, thRatio=10, thPutative=40)
AGG = dict(minPtNum=3, iterNum=3000, thDist=0.2, thInlrRatio=0.05, REFINE=True, VERBOSE=0)
AGG_SEED = 11


def _scene(seed=0, VM=6000, VS=260, D=96):
    import oracle.pcreg_oracle as o
    rng = np.random.default_rng(seed)
    featM = rng.uniform([0, 0, 0], [40, 30, 20], (VM, 3))
    descM = rng.poisson(3.0, (VM, D)).astype(np.float64)
    centre = np.array([22.0, 14.0, 9.0])
    near = np.argsort(np.linalg.norm(featM - centre, axis=1))[:VS]
    R = o.eul2rotm(np.array([0.3, -0.2, 0.1])); t = np.array([2.0, -1.0, 0.5])
    featS = featM[near] @ R.T + t + rng.normal(0, 0.02, (VS, 3))
    descS = descM[near] + rng.poisson(3.0, (VS, D))
    return featM, descM, featS, descS


@pytest.fixture(scope="module")
def stage(oracle_c):
    """the sweep, its largest cluster, the reference of the aggregated stage on that result: computed once, read by every test"""
    from pcreg_amd.sweep import SphereSweep, largest_cluster
    featM, descM, featS, descS = _scene()
    sw = SphereSweep(featM, descM, featS, descS)
    result = sw.run(PAR, OPT, **KW)
    trials, spheres = largest_cluster(result, d_spheres=KW["d_spheres"], **TH)
    ref = aggregated_stage_ref(result, spheres, featS, featM, AGG, seed=AGG_SEED)
    return dict(sw=sw, result=result, trials=trials, spheres=spheres, ref=ref, featM=featM, descM=descM, featS=featS, descS=descS)


def test_the_scene_exercises_both_uniques(stage):
    ref, res = stage["ref"], stage["result"]
    print("good trials in the largest cluster:", len(stage["trials"]), "counts:", ref["n_total"], ref["n_unique1"], ref["n_unique2"],
          "numSuccess", ref["numSuccess"], "maxInliers", ref["maxInliers"])
    assert len(stage["spheres"]) >= 2
    np.testing.assert_array_equal(stage["spheres"], np.asarray(res["trial"])[stage["trials"]])
    assert (np.diff(stage["trials"]) > 0).all()
    assert ref["n_total"] > ref["n_unique1"] > ref["n_unique2"] >= 3
    assert ref["n_total"] == int(np.asarray(res["num_putative"])[stage["spheres"]].sum())
    assert ref["T"] is not None and ref["T_final"] is not None and ref["maxInliers"] >= 3


def test_aggregate_equals_the_reference_with_one_host_sync(stage, monkeypatch):
    import torch
    sw, ref = stage["sw"], stage["ref"]
    calls = []
    orig_cpu, orig_item, orig_sync = torch.Tensor.cpu, torch.Tensor.item, torch.cuda.synchronize
    orig_ssync, orig_esync = torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu"), orig_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: (calls.append("item"), orig_item(self, *a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("synchronize"), orig_sync(*a, **k))[1])
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append("stream"), orig_ssync(self))[1])
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: (calls.append("event"), orig_esync(self))[1])
    got = sw.aggregate(stage["result"], stage["spheres"], AGG, seed=AGG_SEED)
    monkeypatch.undo()
    assert calls == ["cpu"], calls                                     # the final read and nothing else
    assert got["host_syncs"] == 1
    print("counts:", got["n_total"], got["n_unique1"], got["n_unique2"], "numSuccess", got["numSuccess"], "maxInliers", got["maxInliers"],
          "|T - ref|", np.linalg.norm(got["T"] - ref["T"]) if got["T"] is not None else None,
          "|T_final - ref|", np.linalg.norm(got["T_final"] - ref["T_final"]) if got["T_final"] is not None else None)
    for k in ("n_total", "n_unique1", "n_unique2", "numSuccess", "maxInliers"):
        assert got[k] == ref[k], k
    np.testing.assert_array_equal(got["inlierIdx"], ref["inlierIdx"])
    assert got["T"] is not None and got["T_final"] is not None
    assert np.linalg.norm(got["T"] - ref["T"]) < 1e-9
    assert np.linalg.norm(got["T_final"] - ref["T_final"]) < 1e-9
    assert got["maxInlierRatio"] == 100.0 * ref["maxInliers"] / ref["n_unique2"]
    # the same call again gives the same answer (the workspaces are reused)
    again = sw.aggregate(stage["result"], stage["spheres"], AGG, seed=AGG_SEED)
    np.testing.assert_array_equal(again["inlierIdx"], got["inlierIdx"])
    assert np.array_equal(again["T_final"], got["T_final"])


def test_aggregate_refuses_another_sweeps_result(stage):
    from pcreg_amd.sweep import SphereSweep
    other = SphereSweep(stage["featM"], stage["descM"], stage["featS"], stage["descS"])
    with pytest.raises(ValueError, match="not the result"):
        other.aggregate(stage["result"], stage["spheres"], AGG, seed=AGG_SEED)            # never ran
    res2 = other.run(PAR, OPT, **KW)
    with pytest.raises(ValueError, match="not the result"):
        other.aggregate(stage["result"], stage["spheres"], AGG, seed=AGG_SEED)            # ran, but this is not its dict
    with pytest.raises(ValueError, match="not the result"):
        stage["sw"].aggregate(res2, stage["spheres"], AGG, seed=AGG_SEED)
    with pytest.raises(ValueError, match="not a sphere"):
        other.aggregate(res2, [len(res2["centres"])], AGG)
    # no member: nothing to do, nothing read
    out = other.aggregate(res2, [], AGG)
    assert out["n_total"] == 0 and out["T"] is None and out["T_final"] is None and out["host_syncs"] == 0
    # release() drops the private references
    other.release()
    with pytest.raises(ValueError, match="not the result"):
        other.aggregate(res2, stage["spheres"], AGG, seed=AGG_SEED)
