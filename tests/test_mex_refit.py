"""The transform refit's MEX command and MATLAB wrapper.  Without a GPU: the 'modelRefit' command of mex/pcreg_mex.cpp
(tests/mexrefit/refit_driver.cpp on tests/mexstub/mex.h) refuses bad usage through mexErrMsgIdAndTxt and leaks no array;
matlab/refitTransformsModel.m calls it the way the gateway checks.  With one: the round trip -- 4 x 4 x B in and out, a zero page
for an empty result -- equals the ctypes path."""
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
    out = str(tmp_path_factory.mktemp("mexrefit") / "libmexrefit.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexrefit", "refit_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.rd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_char_p, C.c_int]
    L.rd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, pts_double, t_kind, s_kind, r, steps", [
    (4, 0, 0, 0, 1.0, 1.0), (6, 0, 0, 0, 1.0, 1.0), (5, 1, 0, 0, 1.0, 1.0), (5, 0, 1, 0, 1.0, 1.0), (5, 0, 2, 0, 1.0, 1.0), (5, 0, 0, 0, -1.0, 1.0),
    (5, 0, 0, 0, float("nan"), 1.0), (5, 0, 0, 0, 1.0, 0.0), (5, 0, 0, 0, 1.0, -2.0), (5, 0, 0, 0, 1.0, 1.5), (5, 0, 0, 0, 1.0, float("nan")),
    (5, 0, 0, 1, 1.0, 2.0)])
def test_model_refit_usage_errors(drv, nargs, pts_double, t_kind, s_kind, r, steps):
    """wrong argument counts, a double cloud, a 3 x 4 T, a single T, a negative / NaN radius, steps 0, negative, fractional, NaN or int32"""
    e = _err()
    assert drv.rd_usage(nargs, pts_double, t_kind, s_kind, r, steps, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelRefit:"), e.value
    assert drv.rd_live_arrays() == 0


def test_model_refit_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.rd_usage(5, 0, 0, 0, 1.5, 2.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.rd_live_arrays() == 0


def _round_trip(drv, m, pts, T16, r, steps, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    To = np.full((max(B, 1), 16), -7.0); n = np.full(max(B, 1), -7, np.int32); s = np.full(max(B, 1), -7.0, np.float64)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts) if Q else np.zeros((1, 3), np.float32, order="F")
    rc = drv.rd_round_trip(mf.ctypes.data, M, pf.ctypes.data, Q, T16.ctypes.data, B, float(r), steps, nlhs, To.ctypes.data, n.ctypes.data,
                           s.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, To[:B], n[:B], s[:B]


def test_model_refit_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, m[:5], T16, 0.5, 1, 3)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.rd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, r, steps", [(3000, 777, 5, 1.5, 1), (3000, 777, 5, 1.5, 3), (0, 9, 3, 1.0, 1), (3000, 300, 4, 0.0, 2), (500, 0, 2, 1.0, 1),
                                               (500, 20, 0, 1.0, 1)])
def test_model_refit_round_trip_equals_the_host_tier(drv, M, Q, B, r, steps):
    """[Tout, nClose, sumD2] = pcreg_mex('modelRefit', h, single(pts), T, maxDist, steps) with 1 and with 3 outputs: 4 x 4 x B in and
    out, maxDist squared once in single, a zero page for an empty result; the same bits as Model.refit_transforms"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + Q)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    k = min(M, Q, 200)
    pts = np.vstack([(rng.random((Q - k, 3)) * 22 - 1).astype(np.float32), m[:k] + rng.normal(0, 0.01, (k, 3)).astype(np.float32)]) if Q else \
        np.zeros((0, 3), np.float32)
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(1, B):
        T[b, 3, :3] = rng.normal(size=3) * 0.05 * b
    if B > 2:
        T[2] = 0.0
    T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)
    with pc.Model(m) as h:
        want = h.refit_transforms(pts, T, np.float32(r) * np.float32(r), steps=steps)
    for nlhs in (1, 3):
        rc, msg, n_out, To, n, s = _round_trip(drv, m, pts, T16, r, steps, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.rd_live_arrays() == 0
        got = np.ascontiguousarray(To.reshape(B, 4, 4).transpose(0, 2, 1))              # page b, column-major
        np.testing.assert_array_equal(got.view(np.uint64), want["T"].view(np.uint64))
        for b in range(B):
            assert want["empty"][b] == (not got[b].any())                               # a zero page for an empty result
        if nlhs == 3:
            np.testing.assert_array_equal(n, want["n_close"])
            np.testing.assert_array_equal(s.view(np.uint64), want["sum_d2"].view(np.uint64))
    if M >= 3000 and Q >= 777 and B:
        assert not want["empty"][0] and want["n_close"][0] >= 200 and want["empty"][2]
    if M == 0 or Q == 0 or r == 0.0:
        assert want["empty"].all()


def test_refit_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "refitTransformsModel.m")).read()
    assert src.startswith("function [Tout, nClose, sumD2] = refitTransformsModel(h, pts, T, maxDist, steps)")
    assert "[Tout, nClose, sumD2] = pcreg_mex('modelRefit', h, single(pts), double(T), maxDist, double(steps));" in src    # 6 arguments, 3 outputs
    assert "if nargin < 5, steps = 1; end" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelRefit")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 6\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
    assert "r * r" in block and "pcreg_model_refit_f32(" in block
    head = gw[:gw.index("#if __has_include")]
    assert "'modelRefit'" in head and "refitTransformsModel.m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "refitTransformsModel" in integ and "pcreg_model_refit_f32" in integ
