"""completeExperimentFast.m:280-394 as ONE host-tier call (pcreg_final_stage through pcreg_amd.api.finalStage) against the oracle's CPU
restatement and against the device-tier driver pcreg_amd.sweep.FinalStage on the same inputs; its edges (one cluster, no match
anywhere, too few close matches, clusters without keypoints, the batched-memory path) and its argument checks; the limits call."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_descriptors import OPT, keypoints
from test_gpu_final_stage import PAR, _perturbed, _scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    """test_gpu_final_stage's four-cluster scene: 0 and 3 near the truth, 1 a wrong transform, 2 a sphere without model rows."""
    import oracle.c_oracle as oc
    import oracle.pcreg_oracle as o
    model, surface, kpM, T_true = _scene(5)
    featM, descM = oc.getSpacialHistogramDescriptors(model, kpM, dict(OPT, ALIGN_POINTS=False))
    rng = np.random.default_rng(9)
    T_wrong = np.eye(4); T_wrong[:3, :3] = o.eul2rotm(np.array([1.2, 0.4, -0.7])); T_wrong[3, :3] = [10.0, 5.0, -4.0]
    clusters = [(np.array([25.0, 18.0, 12.0]), _perturbed(T_true, rng, 0.004, 0.03)), (np.array([12.0, 30.0, 11.0]), T_wrong),
                (np.array([500.0, 500.0, 500.0]), _perturbed(T_true, rng)), (np.array([24.0, 19.0, 12.0]), _perturbed(T_true, rng, 0.012, 0.1))]
    near = kpM[(kpM[:, 0] > 10) & (kpM[:, 0] < 40)]
    kps = []
    for loc, T in clusters:
        moved = o.quickTF(surface, o.invertTF(T))
        kps.append(np.vstack([o.pcRandomUniformSamples(moved, 3.0, 3.5, rng)[:300], near + rng.normal(0, 0.05, near.shape)]))
    return dict(model=model, surface=surface, featM=featM, descM=descM, clusters=clusters, kps=kps, R_desc=14.0, T_true=T_true)


@pytest.fixture(scope="module")
def hmodel(case):
    from pcreg_amd.api import DescSet
    h = DescSet(case["descM"])
    yield h
    h.close()


def _device_driver(case, clusters, kps, maxDist=1.5):
    import torch
    from pcreg_amd.device import soa
    from pcreg_amd.sweep import FinalStage
    dev = torch.device("cuda", 0)
    fs = FinalStage(soa(torch.from_numpy(case["surface"]).to(dev)), case["featM"], case["descM"], device=dev)
    return fs.run(clusters, kps, OPT, PAR, case["R_desc"], maxDist=maxDist)


def _host(case, hmodel, clusters, kps, maxDist=1.5):
    from pcreg_amd.api import finalStage
    return finalStage(hmodel, case["featM"], case["surface"], clusters, kps, OPT, PAR, case["R_desc"], maxDist)


def _same_as_driver(got, drv):
    K = len(got["precisions"])
    for key in ("num_keypoints", "num_desc", "num_matches", "num_close"):
        np.testing.assert_array_equal(got[key], drv[key], err_msg=key)
    for i in range(K):
        np.testing.assert_array_equal(got["matches"][i], drv["matches"][i], err_msg=f"cluster {i}")
    np.testing.assert_array_equal(np.isnan(got["precisions"]), np.isnan(drv["precisions"]))
    ok = ~np.isnan(drv["precisions"])
    assert np.array_equal(got["precisions"][ok], drv["precisions"][ok])
    assert got["best"] == drv["best"]
    assert (got["T_refine"] is None) == (drv["T_refine"] is None)
    if drv["T_refine"] is not None:
        assert np.array_equal(got["T_refine"], drv["T_refine"])                            # bit for bit
    np.testing.assert_allclose(got["pts_final"], drv["pts_final"].cpu().numpy().T, rtol=0, atol=1e-12)


def test_host_final_stage_equals_oracle_and_device_driver(case, hmodel):
    import oracle.c_oracle as oc
    import oracle.pcreg_oracle as o
    got = _host(case, hmodel, case["clusters"], case["kps"])
    ref = o.final_stage(case["surface"], case["clusters"], case["kps"], case["featM"], case["descM"], case["R_desc"], OPT, PAR, maxDist=1.5,
                        get_descriptors=oc.getSpacialHistogramDescriptors, get_matches=oc.getMatches)
    assert ref["T_refine"] is not None and np.isnan(ref["precisions"][2])
    for i, c in enumerate(ref["per_cluster"]):
        assert got["num_keypoints"][i] == len(c["feat"]) and got["num_desc"][i] == len(c["featCur"])
        np.testing.assert_array_equal(got["matches"][i], c["matches"], err_msg=f"cluster {i}")
        assert got["num_matches"][i] == len(c["matches"]) and got["num_close"][i] == len(c["inliers"])
    np.testing.assert_array_equal(np.isnan(got["precisions"]), np.isnan(ref["precisions"]))
    ok = ~np.isnan(ref["precisions"])
    np.testing.assert_allclose(got["precisions"][ok], ref["precisions"][ok], rtol=0, atol=1e-12)
    assert got["best"] == ref["best"]
    assert np.linalg.norm(got["T_refine"] - ref["T_refine"]) < 1e-9
    np.testing.assert_allclose(got["pts_final"], ref["pts_final"], rtol=0, atol=1e-9)
    _same_as_driver(got, _device_driver(case, case["clusters"], case["kps"]))


def test_one_cluster(case, hmodel):
    cl, kp = case["clusters"][:1], case["kps"][:1]
    got = _host(case, hmodel, cl, kp)
    assert got["best"] == 0 and got["T_refine"] is not None
    _same_as_driver(got, _device_driver(case, cl, kp))


def test_every_precision_nan(case, hmodel):
    """No model keypoint in any sphere: precisions all NaN, MATLAB's max gives the first cluster, no refinement, its moved surface."""
    import oracle.pcreg_oracle as o
    T0, T1 = case["clusters"][0][1], case["clusters"][3][1]
    cl = [(np.array([900.0, 0, 0]), T0), (np.array([-900.0, 0, 0]), T1)]
    kp = keypoints(40, 3)
    got = _host(case, hmodel, cl, [kp, kp])
    assert np.all(np.isnan(got["precisions"])) and got["best"] == 0 and got["T_refine"] is None
    np.testing.assert_allclose(got["pts_final"], o.quickTF(case["surface"], o.invertTF(T0)), rtol=0, atol=1e-12)
    _same_as_driver(got, _device_driver(case, cl, [kp, kp]))


def test_fewer_than_three_close_matches(case, hmodel):
    got = _host(case, hmodel, case["clusters"], case["kps"], maxDist=0.02)
    assert got["num_close"][got["best"]] < 3 and got["T_refine"] is None
    _same_as_driver(got, _device_driver(case, case["clusters"], case["kps"], maxDist=0.02))


def test_clusters_without_keypoints(case, hmodel):
    """A cluster whose keypoints all lie far from the surface (none survives) and one with no keypoint drawn at all."""
    far = np.full((25, 3), 1.0e4) + np.arange(25)[:, None]
    cl = [case["clusters"][0], case["clusters"][3], case["clusters"][0]]
    kps = [far, case["kps"][3], np.zeros((0, 3))]
    got = _host(case, hmodel, cl, kps)
    assert got["num_keypoints"][0] == 0 and got["num_keypoints"][2] == 0 and got["num_keypoints"][1] > 0
    assert np.isnan(got["precisions"][0]) and np.isnan(got["precisions"][2]) and got["best"] == 1
    assert len(got["matches"][0]) == 0 and len(got["matches"][2]) == 0
    drv = _device_driver(case, cl[:2], kps[:2])                           # the device driver cannot describe zero keypoints
    part = {k: (v[:2] if k in ("num_keypoints", "num_desc", "num_matches", "num_close", "precisions", "matches") else v) for k, v in got.items()}
    _same_as_driver(part, drv)


def test_batched_memory_path_gives_the_same_outputs(case, hmodel):
    from pcreg_amd._lib import lib
    one = _host(case, hmodel, case["clusters"], case["kps"])
    L = lib()
    assert L.pcreg_debug_set(b"final_batch_mb", 1) == 0                  # ~130 keypoints per batch: every cluster runs alone
    try:
        many = _host(case, hmodel, case["clusters"], case["kps"])
        assert L.pcreg_debug_set(b"final_batch_mb", 20) == 0             # two clusters (~8 MB each) per batch
        two = _host(case, hmodel, case["clusters"], case["kps"])
    finally:
        L.pcreg_debug_set(b"final_batch_mb", 0)
    for other in (many, two):
        for key in ("num_keypoints", "num_desc", "num_matches", "num_close", "best"):
            np.testing.assert_array_equal(other[key], one[key], err_msg=key)
        assert np.array_equal(other["precisions"], one["precisions"], equal_nan=True)
        assert np.array_equal(other["T_refine"], one["T_refine"]) and np.array_equal(other["pts_final"], one["pts_final"])
        for a, b in zip(other["matches"], one["matches"]):
            np.testing.assert_array_equal(a, b)


def _raw_call(case, hmodel, K, kp_off, model=None):
    from pcreg_amd import _lib
    from pcreg_amd.api import _desc_opts, _fcol, _match_opts, _ptr
    L = _lib.lib()
    fM, P = _fcol(case["featM"]), _fcol(case["surface"])
    N = P.shape[0]
    Kc = max(K, 1)
    locs = _fcol(np.zeros((Kc, 3))); T = np.tile(np.eye(4).ravel(), (Kc, 1))
    kp_off = np.ascontiguousarray(kp_off, dtype=np.int32)
    kp = _fcol(np.zeros((max(int(kp_off.max()), 1), 3)))
    i32 = lambda: np.zeros(Kc, np.int32)
    nk, nd, nm, nc = i32(), i32(), i32(), i32()
    prec = np.zeros(Kc); best, empty = C.c_int32(-7), C.c_int32(-7); Tr = np.zeros(16); out = np.zeros((N, 3), order="F")
    do, mo = _desc_opts(OPT), _match_opts(PAR)
    h = model if model is not None else hmodel
    rc = L.pcreg_final_stage(h._h, _ptr(fM, C.c_double), fM.shape[0], _ptr(P, C.c_double), N, N, _ptr(locs, C.c_double), _ptr(T, C.c_double), K,
                             _ptr(kp, C.c_double), _ptr(kp_off, C.c_int32), C.byref(do), C.byref(mo), C.c_double(14.0), C.c_double(1.5),
                             _ptr(nk, C.c_int32), _ptr(nd, C.c_int32), _ptr(nm, C.c_int32), _ptr(nc, C.c_int32), _ptr(prec, C.c_double), C.byref(best),
                             _ptr(Tr, C.c_double), C.byref(empty), _ptr(out, C.c_double), None)
    return rc, L.pcreg_last_error().decode(), best.value


def test_bad_arguments_are_refused_before_anything_runs(case, hmodel):
    from pcreg_amd import _lib
    from pcreg_amd.api import DescSet
    for K, off, words in ((2, [1, 3, 5], "kp_off[0]"), (3, [0, 4, 2, 6], "decreases"), (0, [0], "K = 0")):
        rc, msg, best = _raw_call(case, hmodel, K, off)
        assert rc == _lib.PCREG_E_ARG and words in msg, msg
        assert best == -7                                                  # nothing written
    with DescSet(np.ones((case["featM"].shape[0], 979))) as wrong:
        rc, msg, _ = _raw_call(case, hmodel, 1, [0, 3], model=wrong)
        assert rc == _lib.PCREG_E_ARG and "D = 979" in msg, msg
    rc, msg, best = _raw_call(case, hmodel, 1, [0, 0])                    # and a valid call still runs afterwards
    assert rc == 0 and best == 0, msg


def test_limits_are_those_of_the_device_moved_surface(case):
    import torch
    from pcreg_amd.api import finalStageLimits, invertTF
    from pcreg_amd.device import soa
    from pcreg_amd.sweep import quickTF_dev
    Ts = [c[1] for c in case["clusters"]]
    lim = finalStageLimits(case["surface"], Ts)
    pts = soa(torch.from_numpy(case["surface"]).to(torch.device("cuda", 0)))
    for k, T in enumerate(Ts):
        moved = quickTF_dev(pts, invertTF(T)).cpu().numpy()
        want = np.array([moved[0].min(), moved[0].max(), moved[1].min(), moved[1].max(), moved[2].min(), moved[2].max()])
        assert np.array_equal(lim[k], want), k
