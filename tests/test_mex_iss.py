"""The ISS keypoints' MEX commands and MATLAB wrappers.  Without a GPU: 'modelIss' and 'pointIss' of mex/pcreg_mex.cpp
(tests/mexiss/iss_driver.cpp on tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array;
matlab/detectISSModel.m and matlab/detectISSFast.m call them the way the gateway checks.  With one: the round trip equals the
ctypes path bit for bit, with 1-based uint32 indices and the eigenvalues as M x 3 columns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD_KINDS, GOOD_VALS = (2, 2, 0, 0, 0), (4.0, 1.0, 0.975, 0.975, 5.0)


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexiss") / "libmexiss.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexiss", "iss_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.di_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, C.c_int]
    L.di_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


def _usage(drv, via_handle, nargs, first_kind, kinds, vals):
    e = _err()
    rc = drv.di_usage(via_handle, nargs, first_kind, (C.c_int * 5)(*kinds), (C.c_double * 5)(*vals), e, 1024)
    return rc, e.value.decode()


def _with(i, kind=None, val=None):
    kinds, vals = list(GOOD_KINDS), list(GOOD_VALS)
    if kind is not None:
        kinds[i] = kind
    if val is not None:
        vals[i] = val
    return kinds, vals


BAD = ([_with(i, kind=0) for i in (0, 1)]                                                             # a double radius
       + [_with(i, val=v) for i in (0, 1) for v in (0.0, -4.0, 1e-40, float("inf"), float("nan"))]
       + [_with(i, kind=2) for i in (2, 3)] + [_with(i, kind=3) for i in (2, 3, 4)]                    # a single or 1 x 2 threshold
       + [_with(i, val=v) for i in (2, 3) for v in (0.0, -0.5, float("inf"), float("nan"))]
       + [_with(4, val=v) for v in (0.0, -1.0, 4.5, float("nan"))] + [_with(4, kind=1)])


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("kinds, vals", BAD)
def test_usage_errors(drv, via_handle, kinds, vals):
    rc, msg = _usage(drv, via_handle, 6, 0, kinds, vals)
    cmd = "modelIss" if via_handle else "pointIss"
    assert rc == 1 and msg.startswith(f"pcreg:usage: {cmd}:"), msg
    assert drv.di_live_arrays() == 0


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs", [5, 7])
def test_a_missing_or_surplus_argument(drv, via_handle, nargs):
    rc, msg = _usage(drv, via_handle, nargs, 0, GOOD_KINDS, GOOD_VALS)
    assert rc == 1 and msg.startswith("pcreg:usage: " + ("modelIss" if via_handle else "pointIss") + ":"), msg
    assert drv.di_live_arrays() == 0


@pytest.mark.parametrize("first_kind", [1, 2])
def test_point_iss_refuses_a_double_or_two_column_cloud(drv, first_kind):
    rc, msg = _usage(drv, 0, 6, first_kind, GOOD_KINDS, GOOD_VALS)
    assert rc == 1 and msg.startswith("pcreg:usage: pointIss:"), msg
    assert drv.di_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    rc, msg = _usage(drv, 1, 6, 0, GOOD_KINDS, GOOD_VALS)
    assert rc == 1 and msg.startswith("pcreg:hip: bad argument"), msg
    assert drv.di_live_arrays() == 0


def _round_trip(drv, via_handle, m, r2s, r2n, g21, g32, mn, nlhs):
    M = len(m)
    kp = np.full(max(M, 1), 0xFFFFFFFF, np.uint32); sal = np.full(max(M, 1), -7.0, np.float64)
    eig = np.full((max(M, 1), 3), -7.0, np.float64, order="F"); nn = np.full(max(M, 1), -7, np.int32)
    e = _err(); n_out = C.c_int(-1); n_kp = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    eb = np.zeros(max(M, 1) * 3, np.float64)
    rc = drv.di_round_trip(via_handle, mf.ctypes.data, M, r2s, r2n, g21, g32, mn, nlhs, kp.ctypes.data, C.byref(n_kp), sal.ctypes.data,
                           eb.ctypes.data, nn.ctypes.data, C.byref(n_out), e, 1024)
    eig = eb[:3 * M].reshape(3, M).T if M else np.zeros((0, 3))
    return rc, e.value.decode(), n_out.value, kp[:max(n_kp.value, 0)], sal[:M], eig, nn[:M]


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, 4.0, 1.0, 0.975, 0.975, 5, 4)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.di_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, rs, rn, mn", [(3000, 3.0, 2.0, 5), (3000, 2.0, 0.7, 8), (2, 3.0, 2.0, 1), (1, 3.0, 2.0, 1), (0, 3.0, 2.0, 5)])
def test_round_trip_equals_the_host_tier(drv, via_handle, M, rs, rn, mn):
    """[keypoints, saliency, eig, nNeighbors] = pcreg_mex('modelIss', h, single(rs^2), single(rn^2), g21, g32, mn) / ('pointIss',
    single(pts), ...) with one to four outputs: the bits of Model.iss_keypoints, the indices 1-based"""
    import pcreg_amd as pc
    from pcreg_amd.api import iss_args
    rng = np.random.default_rng(M + mn)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    with pc.Model(m) as h:
        want = h.iss_keypoints(rs, rn, min_neighbors=mn)
    r2s, r2n, g21, g32, _mn = iss_args(rs, rn, 0.975, 0.975, mn)
    for nlhs in (1, 2, 3, 4):
        rc, msg, n_out, kp, sal, eig, nn = _round_trip(drv, via_handle, m, r2s, r2n, g21, g32, mn, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.di_live_arrays() == 0
        assert kp.dtype == np.uint32 and np.array_equal(kp.astype(np.int64), want["keypoints"].astype(np.int64) + 1)
        if nlhs > 1:
            assert np.array_equal(sal.view(np.uint64), want["saliency"].view(np.uint64))
        if nlhs > 2:
            assert np.array_equal(np.ascontiguousarray(eig).view(np.uint64), np.ascontiguousarray(want["eig"]).view(np.uint64))
        if nlhs > 3:
            assert np.array_equal(nn, want["n_neighbors"])
    if M >= 3000:
        assert 0 < len(want["keypoints"]) < M
    if M <= 2:
        assert len(want["keypoints"]) == 0


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for wrapper, cmd, first in (("detectISSModel", "modelIss", "h"), ("detectISSFast", "pointIss", "single(pts)")):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert f"keypointIndices = pcreg_mex('{cmd}', {first}, r2s, r2n, g21, g32, mn);" in src                      # 7 arguments
        assert f"[keypointIndices, saliency, eigenvalues, numNeighbors] = pcreg_mex('{cmd}', {first}, r2s, r2n, g21, g32, mn);" in src
        # the radii squared in double, the square rounded once to single; the thresholds and the count as doubles
        assert "r2s = single(double(p.Results.SalientRadius) ^ 2);" in src and "r2n = single(double(p.Results.NonMaxRadius) ^ 2);" in src
        assert "g21 = double(p.Results.Threshold21);" in src and "mn = double(p.Results.MinNeighbors);" in src
        for name in ("'SalientRadius'", "'NonMaxRadius'", "'Threshold21', 0.975", "'Threshold32', 0.975", "'MinNeighbors', 5"):
            assert f"addParameter(p, {name}" in src, name
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 7\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 3
        assert "iss_on_handle(" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
    fast = open(os.path.join(ROOT, "matlab", "detectISSFast.m")).read()
    assert fast.startswith("function [keypoints, keypointIndices, saliency, eigenvalues, numNeighbors] = detectISSFast(pts, varargin)")
    assert "keypoints = pts(keypointIndices, :);" in fast
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "detectISSModel" in integ and "pcreg_model_iss_f32" in integ and "detectISSFeatures" in integ
