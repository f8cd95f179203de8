"""The denoising's MEX commands and MATLAB wrappers.  Without a GPU: 'modelDenoise' and 'pointDenoise' of mex/pcreg_mex.cpp
(tests/mexdenoise/denoise_driver.cpp on tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array;
matlab/pcdenoiseModel.m and matlab/pcdenoiseFast.m call them the way the gateway checks.  With one: the round trip equals the
ctypes path bit for bit, with 1-based uint32 indices."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexdenoise") / "libmexdenoise.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexdenoise", "denoise_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.dd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.dd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, k_kind, k, t_kind, t", [
    (2, 0, 4.0, 0, 1.0), (4, 0, 4.0, 0, 1.0), (3, 0, 0.0, 0, 1.0), (3, 0, 32.0, 0, 1.0), (3, 0, 4.5, 0, 1.0), (3, 0, float("nan"), 0, 1.0),
    (3, 1, 4.0, 0, 1.0), (3, 0, 4.0, 0, -0.5), (3, 0, 4.0, 0, float("nan")), (3, 0, 4.0, 0, float("inf")), (3, 0, 4.0, 2, 1.0), (3, 0, 4.0, 3, 1.0)])
def test_usage_errors(drv, via_handle, nargs, k_kind, k, t_kind, t):
    """a missing or surplus argument; k below 1, above 31, fractional, NaN or int32; a threshold negative, NaN, infinite, single or 1 x 2"""
    e = _err()
    assert drv.dd_usage(via_handle, nargs, 0, k_kind, k, t_kind, t, e, 1024) == 1
    cmd = "modelDenoise" if via_handle else "pointDenoise"
    assert e.value.decode().startswith(f"pcreg:usage: {cmd}:"), e.value
    assert drv.dd_live_arrays() == 0


@pytest.mark.parametrize("first_kind", [1, 2])
def test_point_denoise_refuses_a_double_or_two_column_cloud(drv, first_kind):
    e = _err()
    assert drv.dd_usage(0, 3, first_kind, 0, 4.0, 0, 1.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: pointDenoise:"), e.value
    assert drv.dd_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.dd_usage(1, 3, 0, 0, 4.0, 0, 1.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.dd_live_arrays() == 0


def _round_trip(drv, via_handle, m, k, t, nlhs):
    M = len(m)
    inl = np.full(max(M, 1), 0xFFFFFFFF, np.uint32); md = np.full(max(M, 1), -7.0, np.float64)
    e = _err(); n_out = C.c_int(-1); n_inl = C.c_int(-1); thr = C.c_double(-7.0)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    rc = drv.dd_round_trip(via_handle, mf.ctypes.data, M, k, t, nlhs, inl.ctypes.data, C.byref(n_inl), md.ctypes.data, C.byref(thr),
                           C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, inl[:max(n_inl.value, 0)], md[:M], thr.value


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, 4, 1.0, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.dd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, k, t", [(3000, 4, 1.0), (3000, 17, 0.0), (2, 3, 1.0), (1, 4, 1.0), (0, 4, 1.0)])
def test_round_trip_equals_the_host_tier(drv, via_handle, M, k, t):
    """[inlierIndices, meanDist, thr] = pcreg_mex('modelDenoise', h, k, threshold) / ('pointDenoise', single(pts), k, threshold) with
    one, two and three outputs: the bits of Model.denoise, the indices 1-based"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + k)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    with pc.Model(m) as h:
        want = h.denoise(k, t)
    for nlhs in (1, 2, 3):
        rc, msg, n_out, inl, md, thr = _round_trip(drv, via_handle, m, k, t, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.dd_live_arrays() == 0
        assert inl.dtype == np.uint32 and np.array_equal(inl.astype(np.int64), want["inliers"].astype(np.int64) + 1)
        if nlhs > 1:
            assert np.array_equal(md.view(np.uint64), want["mean_dist"].view(np.uint64))
        if nlhs > 2:
            assert np.array_equal(np.float64(thr).view(np.uint64), np.float64(want["thr"]).view(np.uint64))
    if M >= 3000:
        assert 0 < len(want["inliers"]) < M and want["inliers"].min() >= 0
    if M == 2:
        assert np.array_equal(want["inliers"], [0, 1])
    if M <= 1:
        assert len(want["inliers"]) == 0 and np.isnan(want["thr"])


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for wrapper, cmd, first in (("pcdenoiseModel", "modelDenoise", "h"), ("pcdenoiseFast", "pointDenoise", "single(pts)")):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert f"inlierIndices = pcreg_mex('{cmd}', {first}, double(k), double(threshold));" in src          # 4 arguments
        assert f"[inlierIndices, meanDist] = pcreg_mex('{cmd}', {first}, double(k), double(threshold));" in src
        assert "if nargin < 2, k = 4; end" in src and "if nargin < 3, threshold = 1.0; end" in src
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 4\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
        assert "denoise_on_handle(" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
    model = open(os.path.join(ROOT, "matlab", "pcdenoiseModel.m")).read()
    assert model.startswith("function [inlierIndices, meanDist, thr] = pcdenoiseModel(h, k, threshold)")
    assert "[inlierIndices, meanDist, thr] = pcreg_mex('modelDenoise', h, double(k), double(threshold));" in model
    fast = open(os.path.join(ROOT, "matlab", "pcdenoiseFast.m")).read()
    assert fast.startswith("function [ptsOut, inlierIndices, outlierIndices, meanDist] = pcdenoiseFast(pts, k, threshold)")
    assert "ptsOut = pts(inlierIndices, :);" in fast and "outlierIndices = uint32(find(~keep));" in fast
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pcdenoiseModel" in integ and "pcreg_model_denoise_f32" in integ and "pcdenoise" in integ
