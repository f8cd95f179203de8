"""The radius FPFH's MEX commands and MATLAB wrappers.  Without a GPU: 'modelFpfhRadius' and 'pointFpfhRadius' of mex/pcreg_mex.cpp
(tests/mexfpfhradius/fpfh_radius_driver.cpp on tests/mexstub/mex.h, built with -Wall -Wextra -Werror) refuse bad usage through
mexErrMsgIdAndTxt and leak no array; matlab/extractFPFHRadiusModel.m and matlab/extractFPFHRadiusFast.m call them the way the
gateway checks.  With one: the round trip equals the ctypes path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexfpfhradius") / "libmexfpfhradius.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexfpfhradius", "fpfh_radius_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.frd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_int]
    L.frd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, r_kind, r2, n_kind, n, nrm_kind, kn, v_kind", [
    (5, 0, 4.0, 0, 0.0, 0, 6.0, 0), (7, 0, 4.0, 0, 0.0, 0, 6.0, 0), (6, 0, -1.0, 0, 0.0, 0, 6.0, 0), (6, 0, float("nan"), 0, 0.0, 0, 6.0, 0),
    (6, 1, 4.0, 0, 0.0, 0, 6.0, 0), (6, 0, 4.0, 0, -1.0, 0, 6.0, 0), (6, 0, 4.0, 0, 2.5, 0, 6.0, 0), (6, 0, 4.0, 0, float("nan"), 0, 6.0, 0),
    (6, 0, 4.0, 0, 3e9, 0, 6.0, 0), (6, 0, 4.0, 1, 50.0, 0, 6.0, 0), (6, 0, 4.0, 0, 50.0, 2, 6.0, 0), (6, 0, 4.0, 0, 50.0, 3, 6.0, 0),
    (6, 0, 4.0, 0, 50.0, 0, 2.0, 0), (6, 0, 4.0, 0, 50.0, 0, 33.0, 0), (6, 0, 4.0, 0, 50.0, 0, 6.0, 2), (6, 0, 4.0, 0, 50.0, 0, 6.0, 3)])
def test_usage_errors(drv, via_handle, nargs, r_kind, r2, n_kind, n, nrm_kind, kn, v_kind):
    """a missing or surplus argument; r2 negative, NaN or in double; maxNeighbors negative, fractional, NaN, above int32 or an int32;
    normals in double or of two columns; kNormals outside 3 .. 32; a viewpoint of two numbers or in single"""
    e = _err()
    assert drv.frd_usage(via_handle, nargs, 0, r_kind, r2, n_kind, n, nrm_kind, kn, v_kind, e, 1024) == 1
    cmd = "modelFpfhRadius" if via_handle else "pointFpfhRadius"
    assert e.value.decode().startswith(f"pcreg:usage: {cmd}:"), e.value
    assert drv.frd_live_arrays() == 0


@pytest.mark.parametrize("first_kind, nrm_kind", [(1, 1), (2, 1), (0, 4)])
def test_point_command_refuses_a_double_or_two_column_cloud_and_normals_of_another_height(drv, first_kind, nrm_kind):
    e = _err()
    assert drv.frd_usage(0, 6, first_kind, 0, 4.0, 0, 50.0, nrm_kind, 6.0, 1, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: pointFpfhRadius:"), e.value
    assert drv.frd_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.frd_usage(1, 6, 0, 0, 4.0, 0, 50.0, 0, 6.0, 1, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.frd_live_arrays() == 0


def _round_trip(drv, via_handle, m, r2, n, nrm, kn, vp, nlhs):
    M = len(m)
    out = np.full((33, max(M, 1)), -7.0, np.float64)
    cnt = np.full((33, max(M, 1)), 77, np.uint32)
    nn = np.full(max(M, 1), -3, np.int32)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    nf = None if nrm is None else (np.asfortranarray(nrm, np.float32) if M else np.zeros((1, 3), np.float32, order="F"))
    v = None if vp is None else np.asarray(vp, np.float64)
    rc = drv.frd_round_trip(via_handle, mf.ctypes.data, M, float(r2), n, None if nf is None else nf.ctypes.data, kn, None if v is None else v.ctypes.data,
                            nlhs, out.ctypes.data, cnt.ctypes.data, nn.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, out[:, :M].T, cnt[:, :M].T, nn[:M]


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, 0.25, 0, None, 6, None, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.frd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("M, radius, n, given, kn, vp", [(3000, 2.5, 0, False, 9, (10.0, 10.0, 500.0)), (3000, 4.0, 50, True, 6, None),
                                                         (2, 1.0, 0, False, 3, None), (0, 1.0, 0, False, 4, None)])
def test_round_trip_equals_the_host_tier(drv, via_handle, M, radius, n, given, kn, vp):
    """[features, spfh, nNeighbors] = pcreg_mex('modelFpfhRadius', h, r2, maxNeighbors, normals, kNormals, viewpoint) /
    ('pointFpfhRadius', single(pts), ...) with one, two and three outputs, normals given or computed in the call: the bits of
    Model.fpfh_radius"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + n)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    with pc.Model(m) as h:
        nrm = h.normals(9, viewpoint=(10.0, 10.0, 500.0)) if given else None
        want, wcnt, wnn = h.fpfh_radius(radius, normals=nrm, max_neighbors=n, k_normals=kn, viewpoint=vp, counts=True, n_neighbors=True)
    r2 = np.float32(radius * radius)
    for nlhs in (1, 2, 3):
        rc, msg, n_out, out, cnt, nn = _round_trip(drv, via_handle, m, r2, n, nrm, kn, vp, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.frd_live_arrays() == 0
        np.testing.assert_array_equal(np.ascontiguousarray(out).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
        if nlhs >= 2:
            np.testing.assert_array_equal(cnt, wcnt)
        if nlhs >= 3:
            np.testing.assert_array_equal(nn, wnn)
    if M >= 3000:
        assert not np.isnan(want).any() and wnn.max() > 31 and (n == 0 or wnn.max() == n)
    else:
        assert (want == 0).all()


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for wrapper, cmd, first in (("extractFPFHRadiusModel", "modelFpfhRadius", "h"), ("extractFPFHRadiusFast", "pointFpfhRadius", "single(pts)")):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert src.startswith(f"function [features, spfh, nNeighbors] = {wrapper}(")
        tail = f"pcreg_mex('{cmd}', {first}, r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));"      # 7 arguments
        assert "[features, spfh, nNeighbors] = " + tail in src and "[features, spfh] = " + tail in src and "    features = " + tail in src
        assert "r2 = single(double(radius)^2);" in src
        assert "50" in src and "wide enough" in src                       # how MATLAB's default of 50 neighbours is reached
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 7\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
        assert "fpfh_radius_on_handle(" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
    fast = open(os.path.join(ROOT, "matlab", "extractFPFHRadiusFast.m")).read()
    for name in ("'Radius'", "'NumNeighbors'", "'NumNeighborsNormals'", "'Viewpoint'"):
        assert name in fast
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "extractFPFHRadiusModel" in integ and "pcreg_model_fpfh_radius_f32" in integ
