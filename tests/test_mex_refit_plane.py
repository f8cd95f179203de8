"""The point-to-plane refit's MEX command and MATLAB wrapper, in the manner of tests/test_mex_refit.py.  Without a GPU: the
'modelRefitPlane' command of mex/pcreg_mex.cpp (tests/mexrefitplane/refit_plane_driver.cpp on tests/mexstub/mex.h) refuses bad
usage through mexErrMsgIdAndTxt and leaks no array; matlab/refitPlaneModel.m calls it the way the gateway checks.  With one: the
round trip -- 4 x 4 x B in and out, a zero page for an empty result, normals given and [] -- equals the ctypes path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexrefitplane") / "libmexrefitplane.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexrefitplane", "refit_plane_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.pd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_int]
    L.pd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, pts_double, t_kind, n_kind, r, steps, k", [
    (6, 0, 0, 0, 1.0, 1.0, 6.0), (8, 0, 0, 0, 1.0, 1.0, 6.0), (7, 1, 0, 0, 1.0, 1.0, 6.0), (7, 0, 1, 0, 1.0, 1.0, 6.0), (7, 0, 0, 0, -1.0, 1.0, 6.0),
    (7, 0, 0, 0, float("nan"), 1.0, 6.0), (7, 0, 0, 0, 1.0, 0.0, 6.0), (7, 0, 0, 0, 1.0, 1.5, 6.0), (7, 0, 0, 0, 1.0, float("nan"), 6.0),
    (7, 0, 0, 1, 1.0, 1.0, 6.0), (7, 0, 0, 2, 1.0, 1.0, 6.0), (7, 0, 0, 0, 1.0, 1.0, 2.0), (7, 0, 0, 0, 1.0, 1.0, 33.0), (7, 0, 0, 0, 1.0, 1.0, 6.5)])
def test_model_refit_plane_usage_errors(drv, nargs, pts_double, t_kind, n_kind, r, steps, k):
    """wrong argument counts, a double cloud, a 3 x 4 T, a negative / NaN radius, steps 0, fractional or NaN, double or two-column
    normals, k 2, 33 or fractional"""
    e = _err()
    assert drv.pd_usage(nargs, pts_double, t_kind, n_kind, r, steps, k, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelRefitPlane:"), e.value
    assert drv.pd_live_arrays() == 0


def test_model_refit_plane_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.pd_usage(7, 0, 0, 0, 1.5, 2.0, 6.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.pd_live_arrays() == 0


def _round_trip(drv, m, pts, T16, r, steps, normals, k, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    To = np.full((max(B, 1), 16), -7.0)
    n, npl = (np.full(max(B, 1), -7, np.int32) for _ in range(2))
    s, res = (np.full(max(B, 1), -7.0, np.float64) for _ in range(2))
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts) if Q else np.zeros((1, 3), np.float32, order="F")
    nf = None if normals is None else np.asfortranarray(normals, np.float32) if len(normals) else np.zeros((1, 3), np.float32, order="F")
    rc = drv.pd_round_trip(mf.ctypes.data, M, pf.ctypes.data, Q, T16.ctypes.data, B, float(r), steps, None if nf is None else nf.ctypes.data,
                           0 if normals is None else len(normals), k, nlhs, To.ctypes.data, n.ctypes.data, s.ctypes.data, npl.ctypes.data,
                           res.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, To[:B], n[:B], s[:B], npl[:B], res[:B]


def test_model_refit_plane_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, m[:5], T16, 0.5, 1, None, 6, 5)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.pd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, steps", [(4096, 777, 5, 1), (4096, 777, 5, 3), (0, 9, 3, 1), (500, 0, 2, 1), (500, 20, 0, 1)])
def test_model_refit_plane_round_trip_equals_the_host_tier(drv, M, Q, B, steps):
    """[Tout, nClose, sumD2, nPlane, sumRes2] = pcreg_mex('modelRefitPlane', h, single(pts), T, maxDist, steps, normals, k) with 1 and
    with 5 outputs, with given normals and with []: maxDist squared once in single, a zero page for an empty result; the same bits
    as Model.refit_plane"""
    import pcreg_amd as pc
    import plane_ref
    sc = plane_ref.scene()
    m = sc["model"][:M]
    pts = sc["cloud"][:Q].astype(np.float32)                  # the surface in its true place: the identity is nearly right
    T = np.tile(np.eye(4), (B, 1, 1))
    rng = np.random.default_rng(M + Q)
    for b in range(1, B):
        T[b, 3, :3] = rng.normal(size=3) * 0.05 * b
    if B > 2:
        T[2] = 0.0
    T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)
    r = 1.5
    with pc.Model(m) as h:
        given = h.normals(8)
        wants = {"given": h.refit_plane(pts, T, np.float32(r) * np.float32(r), steps=steps, normals=given),
                 "computed": h.refit_plane(pts, T, np.float32(r) * np.float32(r), steps=steps, k=8)}
    for how, want in wants.items():
        for nlhs in (1, 5):
            rc, msg, n_out, To, n, s, npl, res = _round_trip(drv, m, pts, T16, r, steps, given if how == "given" else None, 8, nlhs)
            assert rc == 0, msg
            assert n_out == nlhs and drv.pd_live_arrays() == 0
            got = np.ascontiguousarray(To.reshape(B, 4, 4).transpose(0, 2, 1))              # page b, column-major
            np.testing.assert_array_equal(got.view(np.uint64), want["T"].view(np.uint64))
            for b in range(B):
                assert want["empty"][b] == (not got[b].any())                               # a zero page for an empty result
            if nlhs == 5:
                np.testing.assert_array_equal(n, want["n_close"])
                np.testing.assert_array_equal(s.view(np.uint64), want["sum_d2"].view(np.uint64))
                np.testing.assert_array_equal(npl, want["n_plane"])
                np.testing.assert_array_equal(res.view(np.uint64), want["sum_res2"].view(np.uint64))
        if M >= 4096 and Q >= 777 and B:
            assert not want["empty"][0] and want["n_plane"][0] >= 700 and want["empty"][2]
        if M == 0 or Q == 0:
            assert want["empty"].all()


def test_refit_plane_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "refitPlaneModel.m")).read()
    assert src.startswith("function [Tout, nClose, sumD2, nPlane, sumRes2] = refitPlaneModel(h, pts, T, maxDist, steps, normals, k)")
    assert "[Tout, nClose, sumD2, nPlane, sumRes2] = pcreg_mex('modelRefitPlane', h, single(pts), double(T), maxDist, double(steps), single(normals), " \
           "double(k));" in src                                                                          # 8 arguments, 5 outputs
    assert "if nargin < 5, steps = 1; end" in src and "if nargin < 6, normals = []; end" in src and "if nargin < 7, k = 6; end" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelRefitPlane")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 8\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 4
    assert "r * r" in block and "pcreg_model_refit_plane_f32(" in block
    head = gw[:gw.index("#if __has_include")]
    assert "'modelRefitPlane'" in head and "refitPlaneModel.m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "refitPlaneModel" in integ and "pcreg_model_refit_plane_f32" in integ
