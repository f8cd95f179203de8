"""The farthest point sampling's MEX commands and MATLAB wrappers.  Without a GPU: 'modelFps' and 'pointFps' of mex/pcreg_mex.cpp
(tests/mexfps/fps_driver.cpp on tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array;
matlab/farthestPointsModel.m and matlab/farthestPointsFast.m call them the way the gateway checks.  With one: the round trip equals
the ctypes path bit for bit, with 1-based uint32 rows and single distances."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexfps") / "libmexfps.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexfps", "fps_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.fd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.fd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, k_kind, K, s_kind, start, r_kind, stop", [
    (3, 0, 4.0, 0, 0.0, 2, 0.0), (5, 0, 4.0, 0, 0.0, 2, 0.0), (4, 0, -1.0, 0, 0.0, 2, 0.0), (4, 0, 4.5, 0, 0.0, 2, 0.0),
    (4, 0, float("nan"), 0, 0.0, 2, 0.0), (4, 1, 4.0, 0, 0.0, 2, 0.0), (4, 0, 4.0, 0, -1.0, 2, 0.0), (4, 0, 4.0, 0, 1.5, 2, 0.0),
    (4, 0, 4.0, 2, 1.0, 2, 0.0), (4, 0, 4.0, 0, 0.0, 0, 0.0), (4, 0, 4.0, 0, 0.0, 2, -1.0), (4, 0, 4.0, 0, 0.0, 2, float("nan")),
    (4, 0, 4.0, 0, 0.0, 3, 0.0)])
def test_usage_errors(drv, via_handle, nargs, k_kind, K, s_kind, start, r_kind, stop):
    """a missing or surplus argument; K negative, fractional, NaN or int32; a start negative, fractional or single; a stop that is
    double, negative, NaN or 1 x 2"""
    e = _err()
    assert drv.fd_usage(via_handle, nargs, 0, k_kind, K, s_kind, start, r_kind, stop, e, 1024) == 1
    cmd = "modelFps" if via_handle else "pointFps"
    assert e.value.decode().startswith(f"pcreg:usage: {cmd}:"), e.value
    assert drv.fd_live_arrays() == 0


@pytest.mark.parametrize("first_kind", [1, 2])
def test_point_fps_refuses_a_double_or_two_column_cloud(drv, first_kind):
    e = _err()
    assert drv.fd_usage(0, 4, first_kind, 0, 4.0, 0, 0.0, 2, 0.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: pointFps:"), e.value
    assert drv.fd_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.fd_usage(1, 4, 0, 0, 4.0, 0, 0.0, 2, 0.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.fd_live_arrays() == 0


def _round_trip(drv, via_handle, m, K, start1, stop_d2, nlhs):
    M = len(m)
    idx = np.full(max(K, 1), 0xFFFFFFFF, np.uint32); d2 = np.full(max(K, 1), -7.0, np.float32)
    lab = np.full(max(M, 1), 0xFFFFFFFF, np.uint32); md = np.full(max(M, 1), -7.0, np.float32)
    e = _err(); n_out = C.c_int(-1); n = C.c_int(-1); cover = C.c_float(-7.0)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    rc = drv.fd_round_trip(via_handle, mf.ctypes.data, M, K, start1, stop_d2, nlhs, idx.ctypes.data, d2.ctypes.data, C.byref(n), lab.ctypes.data,
                           md.ctypes.data, C.byref(cover), C.byref(n_out), e, 1024)
    k = max(n.value, 0)
    return rc, e.value.decode(), n_out.value, idx[:k], d2[:k], lab[:M], md[:M], np.float32(cover.value)


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, 4, 0, 0.0, 5)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.fd_live_arrays() == 0


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, K, start1, stop_d2", [(3000, 100, 0, 0.0), (3000, 100, 3000, 40.0), (700, 705, 1, 0.0), (2, 3, 2, 0.0), (1, 4, 0, INF),
                                                  (0, 4, 0, 0.0), (50, 0, 0, 0.0)])
def test_round_trip_equals_the_host_tier(drv, via_handle, M, K, start1, stop_d2):
    """[idx, d2, label, minD2, coverD2] = pcreg_mex('modelFps', h, K, start, stopD2) / ('pointFps', single(pts), ...) with one to five
    outputs: the bits of Model.farthest_points, the rows 1-based, single distances"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + K)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    if M >= 700:
        m[5, 1] = np.nan                                          # a dead row: label 0, minD2 NaN
    with pc.Model(m) as h:
        want = h.farthest_points(K, start1 - 1, stop_d2)
    for nlhs in (1, 2, 3, 4, 5):
        rc, msg, n_out, idx, d2, lab, md, cover = _round_trip(drv, via_handle, m, K, start1, stop_d2, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.fd_live_arrays() == 0
        assert idx.dtype == np.uint32 and np.array_equal(idx.astype(np.int64), want["idx"].astype(np.int64) + 1)
        if nlhs > 1:
            assert d2.dtype == np.float32 and np.array_equal(_u32(d2), _u32(want["dist"]))
        if nlhs > 2:
            assert np.array_equal(lab.astype(np.int64), want["label"].astype(np.int64))
        if nlhs > 3:
            nan = np.isnan(want["min_dist"])
            assert np.array_equal(np.isnan(md), nan) and np.array_equal(_u32(md[~nan]), _u32(want["min_dist"][~nan]))
        if nlhs > 4:
            assert (np.isnan(cover) and np.isnan(want["cover_d2"])) or _u32(cover) == _u32(want["cover_d2"])
    if M == 3000:
        assert (want["n_out"] == K if stop_d2 == 0.0 else 2 < want["n_out"] < K) and want["label"][5] == 0 and want["label"].max() == want["n_out"]
        assert want["idx"][0] == (0 if start1 == 0 else start1 - 1)
    if M == 700:
        assert want["n_out"] == 699                               # every finite row, and the sampling stops by itself
    if M == 0 or K == 0:
        assert want["n_out"] == 0 and np.isnan(want["cover_d2"])


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
def test_a_dead_start_row_is_refused(drv, via_handle):
    m = np.random.default_rng(1).random((100, 3)).astype(np.float32)
    m[41, 2] = np.inf
    rc, msg, *_ = _round_trip(drv, via_handle, m, 5, 42, 0.0, 5)
    assert rc == 1 and msg.startswith("pcreg:hip: bad argument") and "start" in msg
    assert drv.fd_live_arrays() == 0


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for wrapper, cmd, first, nout in (("farthestPointsModel", "modelFps", "h", 5), ("farthestPointsFast", "pointFps", "single(pts)", 4)):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert f"idx = pcreg_mex('{cmd}', {first}, double(K), double(s), r2);" in src                        # 5 arguments
        assert f"[idx, d2, label, minD2] = pcreg_mex('{cmd}', {first}, double(K), double(s), r2);" in src
        assert "r2 = single(r) * single(r);" in src and "s = 0; r = 0;" in src                             # squared in single; the defaults
        assert "case 'start'," in src and "case 'stopdistance'," in src
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 5\b", block) and "fps_on_handle(" in block and "fps_args_ok(prhs + 2)" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
        assert src.startswith(f"function [idx, d2, label, minD2{', coverD2' if nout == 5 else ''}] = {wrapper}(")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "farthestPointsModel" in integ and "farthestPointsFast" in integ and "pcreg_model_fps_f32" in integ
