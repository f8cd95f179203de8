"""The downsampling's MEX command and MATLAB wrapper.  Without a GPU: 'downsampleGrid' of mex/pcreg_mex.cpp
(tests/mexdownsample/downsample_driver.cpp on tests/mexstub/mex.h) refuses bad usage through mexErrMsgIdAndTxt and leaks no array;
matlab/pcdownsampleFast.m calls it the way the gateway checks.  With one: the round trip equals the ctypes path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexdownsample") / "libmexdownsample.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexdownsample", "downsample_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.dd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.dd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, first_kind, step_kind, step", [
    (1, 0, 0, 0.5), (3, 0, 0, 0.5), (2, 2, 0, 0.5), (2, 0, 0, 0.0), (2, 0, 0, -1.0), (2, 0, 0, float("nan")), (2, 0, 0, float("inf")),
    (2, 0, 1, 2.0), (2, 0, 2, 0.5)])
def test_usage_errors(drv, nargs, first_kind, step_kind, step):
    """a missing or surplus argument, a two-column cloud, a step of 0, below 0, NaN, Inf, in int32 or of two numbers"""
    e = _err()
    assert drv.dd_usage(nargs, first_kind, step_kind, step, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: downsampleGrid:"), e.value
    assert drv.dd_live_arrays() == 0


def test_a_double_cloud_is_refused_with_the_remedy(drv):
    e = _err()
    assert drv.dd_usage(2, 1, 0, 0.5, e, 1024) == 1
    msg = e.value.decode()
    assert msg.startswith("pcreg:usage: downsampleGrid:") and "single(pts)" in msg
    assert drv.dd_live_arrays() == 0


def _round_trip(drv, p, step, nlhs):
    n = len(p)
    out = np.full(3 * max(n, 1), -7.0, np.float32); cnt = np.full(max(n, 1), -7, np.int32); lab = np.full(max(n, 1), -7, np.int32)
    e = _err(); u = C.c_int(-1); nl = C.c_int(-1)
    pf = np.asfortranarray(p, dtype=np.float32) if n else np.zeros((1, 3), np.float32, order="F")
    rc = drv.dd_round_trip(pf.ctypes.data, n, step, nlhs, out.ctypes.data, cnt.ctypes.data, lab.ctypes.data, C.byref(u), C.byref(nl), e, 1024)
    uu = max(u.value, 0)
    return rc, e.value.decode(), u.value, nl.value, out[:3 * uu].reshape(3, uu).T, cnt[:uu], lab[:n]


def test_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    p = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, p, 0.25, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.dd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n, step", [(5000, 1.5), (3, 0.5), (0, 1.0)])
def test_round_trip_equals_the_host_tier(drv, n, step):
    """[ptsOut, counts, labels] = pcreg_mex('downsampleGrid', single(pts), gridStep) with one, two and three outputs: the bits of
    pcreg_amd.pcdownsample (labels 1-based here)"""
    import pcreg_amd as pc
    p = (np.random.default_rng(n).random((n, 3)) * 20).astype(np.float32)
    if n > 100:
        p[17, 1] = np.nan
    want_o, want_c, want_l = pc.pcdownsample(p, step)
    for nlhs in (1, 2, 3):
        rc, msg, u, nl, out, cnt, lab = _round_trip(drv, p, step, nlhs)
        assert rc == 0, msg
        assert nl == nlhs and u == len(want_o) and drv.dd_live_arrays() == 0
        np.testing.assert_array_equal(np.ascontiguousarray(out).view(np.uint32), want_o.view(np.uint32))
        if nlhs > 1:
            np.testing.assert_array_equal(cnt, want_c)
        if nlhs > 2:
            np.testing.assert_array_equal(lab, want_l + 1)
    if n > 100:
        assert 0 < len(want_o) < n and want_l[17] == -1


@pytest.mark.gpu
def test_the_cell_limit_is_a_library_error(drv):
    p = np.array([[0, 0, 0], [2.0 ** 21, 0, 0]], np.float32)
    rc, msg, *_ = _round_trip(drv, p, 1.0, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "2^21" in msg
    assert drv.dd_live_arrays() == 0


def test_the_wrapper_calls_the_command_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    src = open(os.path.join(ROOT, "matlab", "pcdownsampleFast.m")).read()
    assert src.startswith("function [ptsOut, counts, labels] = pcdownsampleFast(pts, gridStep)")
    assert "[ptsOut, counts, labels] = pcreg_mex('downsampleGrid', single(pts), double(gridStep));" in src      # 3 arguments, 3 outputs
    assert "ptsOut = pcreg_mex('downsampleGrid', single(pts), double(gridStep));" in src
    block = gw.split('strcmp(cmd, "downsampleGrid")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 3\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
    assert "pcreg_downsample_grid_f32(" in block and "single(pts)" in block
    assert "'downsampleGrid'" in head and "pcdownsampleFast.m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pcdownsampleFast" in integ and "pcreg_downsample_grid_f32" in integ and "pcdownsample" in integ
