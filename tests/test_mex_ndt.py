"""The NDT's MEX commands and MATLAB wrappers, in the manner of tests/test_mex_refit_plane.py.  Without a GPU: the 'ndtCreate',
'ndtRefit' and 'ndtDestroy' commands of mex/pcreg_mex.cpp (tests/mexndt/ndt_driver.cpp on tests/mexstub/mex.h) refuse bad usage
through mexErrMsgIdAndTxt and leak no array; matlab/ndtModel.m, refitNdtModel.m and refitNdtFast.m call them the way the gateway
checks.  With one: the round trip -- 4 x 4 x B in and out, a zero page for an empty result -- equals the ctypes path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexndt") / "libmexndt.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexndt", "ndt_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.nd_create_usage.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_char_p, C.c_int]
    L.nd_refit_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_int]
    L.nd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, pts_double, step, min_points", [
    (2, 0, 1.0, 6.0), (4, 0, 1.0, 6.0), (3, 1, 1.0, 6.0), (3, 0, 0.0, 6.0), (3, 0, -1.0, 6.0), (3, 0, float("nan"), 6.0), (3, 0, float("inf"), 6.0),
    (3, 0, 1.0, 2.0), (3, 0, 1.0, 6.5), (3, 0, 1.0, float("nan"))])
def test_ndt_create_usage_errors(drv, nargs, pts_double, step, min_points):
    """wrong argument counts, a double cloud, a step that is zero, negative, NaN or infinite, minPoints 2, fractional or NaN"""
    e = _err()
    assert drv.nd_create_usage(nargs, pts_double, step, min_points, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: ndtCreate:"), e.value
    assert drv.nd_live_arrays() == 0


@pytest.mark.parametrize("nargs, pts_double, t_kind, neighbors, ratio, steps", [
    (5, 0, 0, 1.0, 0.55, 1.0), (7, 0, 0, 1.0, 0.55, 1.0), (6, 1, 0, 1.0, 0.55, 1.0), (6, 0, 1, 1.0, 0.55, 1.0), (6, 0, 0, 0.0, 0.55, 1.0),
    (6, 0, 0, 3.0, 0.55, 1.0), (6, 0, 0, 27.0, 0.55, 1.0), (6, 0, 0, float("nan"), 0.55, 1.0), (6, 0, 0, 7.0, 1.0, 1.0), (6, 0, 0, 7.0, -0.1, 1.0),
    (6, 0, 0, 7.0, float("nan"), 1.0), (6, 0, 0, 1.0, 0.55, 0.0), (6, 0, 0, 1.0, 0.55, 1.5), (6, 0, 0, 1.0, 0.55, float("nan"))])
def test_ndt_refit_usage_errors(drv, nargs, pts_double, t_kind, neighbors, ratio, steps):
    """wrong argument counts, a double cloud, a 3 x 4 T, neighbors 0, 3, 27 or NaN, a ratio of 1, negative or NaN, steps 0, fractional or NaN"""
    e = _err()
    assert drv.nd_refit_usage(nargs, pts_double, t_kind, neighbors, ratio, steps, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: ndtRefit:"), e.value
    assert drv.nd_live_arrays() == 0


def test_ndt_null_handle_is_a_library_error_and_destroy_wants_a_handle(drv):
    e = _err()
    assert drv.nd_refit_usage(6, 0, 0, 7.0, 0.3, 2.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.nd_live_arrays() == 0
    assert drv.nd_refit_usage(-1, 0, 0, 1.0, 0.5, 1.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: ndtDestroy:"), e.value
    assert drv.nd_live_arrays() == 0


def _round_trip(drv, m, step, min_points, pts, T16, neighbors, ratio, steps, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    To = np.full((max(B, 1), 16), -7.0)
    n = np.full(max(B, 1), -7, np.int32)
    s = np.full(max(B, 1), -7.0, np.float64)
    sizes = np.full(2, -7, np.int32)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m, np.float32) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts, np.float32) if Q else np.zeros((1, 3), np.float32, order="F")
    rc = drv.nd_round_trip(mf.ctypes.data, M, float(step), min_points, pf.ctypes.data, Q, T16.ctypes.data, B, neighbors, float(ratio), steps, nlhs,
                           sizes.ctypes.data, To.ctypes.data, n.ctypes.data, s.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, sizes.tolist(), To[:B], n[:B], s[:B]


def test_ndt_create_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, 0.5, 6, m[:5], T16, 1, 0.55, 1, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.nd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, neighbors, steps", [(4096, 777, 5, 1, 1), (4096, 777, 5, 7, 3), (0, 9, 3, 1, 1), (500, 0, 2, 7, 1), (500, 20, 0, 1, 1)])
def test_ndt_round_trip_equals_the_host_tier(drv, M, Q, B, neighbors, steps):
    """[h, nVoxels, nGaussians] = pcreg_mex('ndtCreate', ...) and [Tout, nPairs, sumE] = pcreg_mex('ndtRefit', ...) with 1 and with 3
    outputs: a zero page for an empty result; the same bits as NdtModel.refit"""
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
    with pc.NdtModel(m, 4.0) as h:
        sizes = [h.n_voxels, h.n_gaussians]
        want = h.refit(pts, T, neighbors=neighbors, outlier_ratio=0.3, steps=steps)
    for nlhs in (1, 3):
        rc, msg, n_out, got_sizes, To, n, s = _round_trip(drv, m, 4.0, 6, pts, T16, neighbors, 0.3, steps, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and got_sizes == sizes and drv.nd_live_arrays() == 0
        got = np.ascontiguousarray(To.reshape(B, 4, 4).transpose(0, 2, 1))              # page b, column-major
        np.testing.assert_array_equal(got.view(np.uint64), want["T"].view(np.uint64))
        for b in range(B):
            assert want["empty"][b] == (not got[b].any())                               # a zero page for an empty result
        if nlhs == 3:
            np.testing.assert_array_equal(n, want["n_pairs"])
            np.testing.assert_array_equal(s.view(np.uint64), want["sum_e"].view(np.uint64))
    if M >= 4096 and Q >= 777 and B:
        assert not want["empty"][0] and want["n_pairs"][0] >= 700 and want["empty"][2] and sizes[1] > 100
    if M == 0 or Q == 0:
        assert want["empty"].all()


def test_the_wrappers_call_the_commands_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "refitNdtModel.m")).read()
    assert src.startswith("function [Tout, nPairs, sumE] = refitNdtModel(h, pts, T, neighbors, outlierRatio, steps)")
    call = "[Tout, nPairs, sumE] = pcreg_mex('ndtRefit', h, single(pts), double(T), double(neighbors), double(outlierRatio), double(steps));"
    assert call in src                                                                                   # 7 arguments, 3 outputs
    assert "if nargin < 4, neighbors = 1; end" in src and "if nargin < 5, outlierRatio = 0.55; end" in src and "if nargin < 6, steps = 1; end" in src
    mk = open(os.path.join(ROOT, "matlab", "ndtModel.m")).read()
    assert mk.startswith("function [h, nVoxels, nGaussians] = ndtModel(pts, step, minPoints)") and "if nargin < 3, minPoints = 6; end" in mk
    assert "[h, nVoxels, nGaussians] = pcreg_mex('ndtCreate', single(pts), double(step), double(minPoints));" in mk
    fast = open(os.path.join(ROOT, "matlab", "refitNdtFast.m")).read()
    assert fast.startswith("function [Tout, nPairs, sumE] = refitNdtFast(model, step, pts, T, neighbors, outlierRatio, steps, minPoints)")
    assert "pcreg_mex('ndtCreate', single(model), double(step), double(minPoints));" in fast and call in fast
    assert "onCleanup(@() pcreg_mex('ndtDestroy', h))" in fast
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "ndtRefit")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 7\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2 and "pcreg_ndt_refit_f32(" in block
    block = gw.split('strcmp(cmd, "ndtCreate")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 4\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2 and "pcreg_ndt_create(" in block
    assert "pcreg_ndt_destroy(" in gw.split('strcmp(cmd, "ndtDestroy")')[1].split("strcmp(cmd,")[0]
    head = gw[:gw.index("#if __has_include")]
    assert all(s in head for s in ("'ndtCreate'", "'ndtRefit'", "'ndtDestroy'", "ndtModel.m", "refitNdtModel.m", "refitNdtFast.m"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in integ for s in ("ndtModel", "refitNdtModel", "refitNdtFast", "pcreg_ndt_refit_f32", "pcreg_dev_ndt_refit_f32"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "NdtModel" in readme and "pcreg_ndt_refit_f32" in readme
