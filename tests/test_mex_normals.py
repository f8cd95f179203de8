"""The normals' MEX commands and MATLAB wrappers.  Without a GPU: 'modelNormals' and 'pointNormals' of mex/pcreg_mex.cpp
(tests/mexnormals/normals_driver.cpp on tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array;
matlab/pcnormalsModel.m and matlab/pcnormalsFast.m call them the way the gateway checks.  With one: the round trip equals the
ctypes path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexnormals") / "libmexnormals.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexnormals", "normals_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.nd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_int]
    L.nd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, first_kind, k_kind, k, v_kind", [
    (2, 0, 0, 6.0, 0), (4, 0, 0, 6.0, 0), (3, 0, 0, 2.0, 0), (3, 0, 0, 33.0, 0), (3, 0, 0, 6.5, 0), (3, 0, 0, float("nan"), 0), (3, 0, 1, 6.0, 0),
    (3, 0, 0, 6.0, 2), (3, 0, 0, 6.0, 3)])
def test_usage_errors(drv, via_handle, nargs, first_kind, k_kind, k, v_kind):
    """a missing or surplus argument, k below 3, above 32, fractional, NaN or int32, a viewpoint of two numbers or in single"""
    e = _err()
    assert drv.nd_usage(via_handle, nargs, first_kind, k_kind, k, v_kind, e, 1024) == 1
    cmd = "modelNormals" if via_handle else "pointNormals"
    assert e.value.decode().startswith(f"pcreg:usage: {cmd}:"), e.value
    assert drv.nd_live_arrays() == 0


@pytest.mark.parametrize("first_kind", [1, 2])
def test_point_normals_refuses_a_double_or_two_column_cloud(drv, first_kind):
    e = _err()
    assert drv.nd_usage(0, 3, first_kind, 0, 6.0, 1, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: pointNormals:"), e.value
    assert drv.nd_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.nd_usage(1, 3, 0, 0, 6.0, 1, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.nd_live_arrays() == 0


def _round_trip(drv, via_handle, m, k, vp, nlhs):
    M = len(m)
    nrm = np.full((3, max(M, 1)), -7.0, np.float32); var = np.full(max(M, 1), -7.0, np.float32)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    v = None if vp is None else np.asarray(vp, np.float64)
    rc = drv.nd_round_trip(via_handle, mf.ctypes.data, M, k, None if v is None else v.ctypes.data, nlhs, nrm.ctypes.data, var.ctypes.data,
                           C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, nrm[:, :M].T, var[:M]


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, 6, None, 2)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.nd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, k, vp", [(3000, 6, None), (3000, 17, (10.0, 10.0, 500.0)), (2, 3, None), (0, 4, None)])
def test_round_trip_equals_the_host_tier(drv, via_handle, M, k, vp):
    """[normals, variation] = pcreg_mex('modelNormals', h, k, viewpoint) / ('pointNormals', single(pts), k, viewpoint) with one and
    with two outputs: the bits of Model.normals"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + k)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    with pc.Model(m) as h:
        want_n, want_v = h.normals(k, viewpoint=vp, variation=True)
    for nlhs in (1, 2):
        rc, msg, n_out, nrm, var = _round_trip(drv, via_handle, m, k, vp, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.nd_live_arrays() == 0
        np.testing.assert_array_equal(np.ascontiguousarray(nrm).view(np.uint32), np.ascontiguousarray(want_n).view(np.uint32))
        if nlhs == 2:
            np.testing.assert_array_equal(var.view(np.uint32), want_v.view(np.uint32))
    if M >= 3000:
        assert not np.isnan(want_n).any()
    else:
        assert np.isnan(want_n).all()


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for wrapper, cmd, first in (("pcnormalsModel", "modelNormals", "h"), ("pcnormalsFast", "pointNormals", "single(pts)")):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert src.startswith(f"function [normals, variation] = {wrapper}(")
        assert f"[normals, variation] = pcreg_mex('{cmd}', {first}, double(k), double(viewpoint));" in src       # 4 arguments, 2 outputs
        assert f"normals = pcreg_mex('{cmd}', {first}, double(k), double(viewpoint));" in src
        assert "if nargin < 3, viewpoint = []; end" in src
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 4\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 1
        assert "normals_on_handle(" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pcnormalsModel" in integ and "pcreg_model_normals_f32" in integ and "pcnormals" in integ
