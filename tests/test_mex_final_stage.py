"""The 'finalStageLimits' / 'finalStage' commands of mex/pcreg_mex.cpp, built with tests/mexstub/mex.h and a driver of their own
(tests/mexfinal/final_stage_driver.cpp) into a separate library.  CPU: the gateway compiles warning-free, usage and no-device errors
arrive through mexErrMsgIdAndTxt.  GPU: one round trip equals the ctypes path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexfinal") / "libmexfinal.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexfinal", "final_stage_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *inc, srcs[0]])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    return C.CDLL(out)


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _err():
    return C.create_string_buffer(1024)


def test_final_stage_usage_error(drv):
    e = _err()
    assert drv.fs_usage(e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: finalStage:"), e.value
    assert drv.fs_live_arrays() == 0


def test_final_stage_reports_nodevice_through_mexerr(drv):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    pts = np.asfortranarray(np.random.default_rng(0).random((20, 3)))
    T = np.tile(np.eye(4).ravel(order="F"), 2)
    lim = np.zeros(12); e = _err()
    assert drv.fs_limits(_p(pts), 20, _p(T), 2, _p(lim), e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
    assert drv.fs_live_arrays() == 0


@pytest.mark.gpu
def test_final_stage_round_trip_equals_the_ctypes_path(drv):
    import pcreg_amd as pc
    from pcreg_amd.api import DescSet, invertTF
    from test_gpu_descriptors import OPT, keypoints, strips
    from test_gpu_final_stage import PAR, _perturbed
    import oracle.pcreg_oracle as o
    model = strips(20000, 11)
    rng = np.random.default_rng(12)
    T_true = np.eye(4); T_true[:3, :3] = o.eul2rotm(np.array([0.2, -0.1, 0.3])); T_true[3, :3] = [1.0, -2.0, 0.5]
    sel = (model[:, 0] > 10) & (model[:, 0] < 40)
    surface = o.quickTF(model[sel], T_true) + rng.normal(0, 0.01, (sel.sum(), 3))
    kpM = keypoints(800, 13)
    featM, descM = pc.getSpacialHistogramDescriptors(model, kpM, dict(OPT, ALIGN_POINTS=False, VERBOSE=0))
    clusters = [(np.array([25.0, 18.0, 12.0]), _perturbed(T_true, rng, 0.004, 0.03)), (np.array([600.0, 0.0, 0.0]), T_true)]
    near = kpM[(kpM[:, 0] > 12) & (kpM[:, 0] < 38)]
    kps = [near + rng.normal(0, 0.05, near.shape), near[:50]]
    K, N = 2, surface.shape[0]
    moving = np.concatenate([invertTF(T).ravel(order="F") for _, T in clusters])
    e = _err()
    lim = np.zeros(K * 6)
    assert drv.fs_limits(_p(np.asfortranarray(surface)), N, _p(moving), K, _p(lim), e, 1024) == 0, e.value
    assert np.array_equal(lim.reshape(6, K).T, pc.finalStageLimits(surface, [T for _, T in clusters]))
    kp_off = np.array([0, len(kps[0]), len(kps[0]) + len(kps[1])], dtype=np.int32)
    kp = np.asfortranarray(np.vstack(kps))
    locs = np.asfortranarray([c[0] for c in clusters])
    desc6 = np.array([OPT["min_pts"], OPT["max_pts"], OPT["R"], OPT["thVar"][0], OPT["thVar"][1], 1.0 if OPT["k"] == "all" else OPT["k"]], dtype=np.float64)
    par7 = np.array([PAR["MatchThreshold"], PAR["MaxRatio"], PAR["Unique"], PAR["UNNORMALIZE"], PAR["norm_factor"], PAR["CHANGE_METRIC"], PAR["metric_factor"]],
                    dtype=np.float64)
    nk, nd, nm, nc, prec = (np.zeros(K) for _ in range(5))
    best = C.c_double(0); Tr = np.zeros(16); te = C.c_int(-1); pf = np.zeros(N * 3); pairs = np.zeros(int(kp_off[-1]) * 2, dtype=np.uint32); P = C.c_int(-1)
    assert drv.fs_round_trip(_p(np.asfortranarray(descM)), descM.shape[0], descM.shape[1], _p(np.asfortranarray(featM)), _p(np.asfortranarray(surface)), N,
                             _p(locs), K, _p(moving), _p(kp), _p(kp_off, C.c_int32), _p(desc6), _p(par7), C.c_double(14.0), C.c_double(1.5),
                             _p(nk), _p(nd), _p(nm), _p(nc), _p(prec), C.byref(best), _p(Tr), C.byref(te), _p(pf), _p(pairs, C.c_uint32), C.byref(P),
                             e, 1024) == 0, e.value
    assert drv.fs_live_arrays() == 0
    with DescSet(descM) as h:
        ref = pc.finalStage(h, featM, surface, clusters, kps, OPT, PAR, 14.0, 1.5)
    assert ref["T_refine"] is not None and np.isnan(ref["precisions"][1])
    for key, got in (("num_keypoints", nk), ("num_desc", nd), ("num_matches", nm), ("num_close", nc)):
        np.testing.assert_array_equal(got, ref[key], err_msg=key)
    assert np.array_equal(prec, ref["precisions"], equal_nan=True)
    assert best.value == ref["best"] + 1 and te.value == 0 and np.array_equal(Tr.reshape(4, 4, order="F"), ref["T_refine"])
    assert np.array_equal(pf.reshape(3, N).T, ref["pts_final"])
    mats = pairs[:2 * P.value].reshape(2, P.value).T
    np.testing.assert_array_equal(mats, np.vstack(ref["matches"]))
