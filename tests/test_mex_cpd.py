"""The coherent-point-drift refit's MEX command and MATLAB wrapper, in the manner of tests/test_mex_refit_gicp.py.  Without a GPU:
the 'modelRefitCpd' command of mex/pcreg_mex.cpp (tests/mexrefitcpd/refit_cpd_driver.cpp on tests/mexstub/mex.h) refuses bad
usage through mexErrMsgIdAndTxt and leaks no array; matlab/refitCpdModel.m calls it the way the gateway checks.  With one: the
round trip -- 4 x 4 x B in and out, a zero page for an empty result, a variance for all pages or one per page -- equals the ctypes
path bit for bit (two handles of the same model: the sums run in the rows' original order, whatever the preparation)."""
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
    out = str(tmp_path_factory.mktemp("mexrefitcpd") / "libmexrefitcpd.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexrefitcpd", "refit_cpd_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.cd_usage.argtypes = [C.c_int] * 5 + [C.c_double] * 3 + [C.c_char_p, C.c_int]
    L.cd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


OK = dict(nargs=6, pts_double=0, t_kind=0, n_sigma=1, sigma_single=0, sigma2=0.0, outlier=0.1, steps=1.0)


@pytest.mark.parametrize("kw", [
    dict(nargs=5), dict(nargs=7), dict(pts_double=1), dict(t_kind=1), dict(n_sigma=3), dict(n_sigma=0), dict(sigma_single=1), dict(outlier=-0.1),
    dict(outlier=1.0), dict(outlier=float("nan")), dict(outlier=float("inf")), dict(steps=0.0), dict(steps=1.5), dict(steps=float("nan"))],
    ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_model_refit_cpd_usage_errors(drv, kw):
    """wrong argument counts, a double cloud, a 3 x 4 T, three or no variances for two pages, a single variance, an outlier weight
    below 0, at 1, NaN or inf, steps 0, fractional or NaN"""
    a = dict(OK, **kw)
    e = _err()
    assert drv.cd_usage(a["nargs"], a["pts_double"], a["t_kind"], a["n_sigma"], a["sigma_single"], a["sigma2"], a["outlier"], a["steps"], e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelRefitCpd:"), e.value
    assert drv.cd_live_arrays() == 0


@pytest.mark.parametrize("n_sigma, sigma2, outlier", [(1, 0.0, 0.1), (2, 1.5, 0.0), (1, -1.0, 0.999)])
def test_model_refit_cpd_null_handle_is_a_library_error(drv, n_sigma, sigma2, outlier):
    e = _err()
    assert drv.cd_usage(6, 0, 0, n_sigma, 0, sigma2, outlier, 2.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.cd_live_arrays() == 0


def _round_trip(drv, m, pts, T16, sigma2, outlier, steps, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    To = np.full((max(B, 1), 16), -7.0)
    dbl = np.full((4, max(B, 1)), -7.0)
    n = np.full(max(B, 1), -7, np.int32)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts) if Q else np.zeros((1, 3), np.float32, order="F")
    sg = np.ascontiguousarray(np.asarray(sigma2, np.float64).reshape(-1))
    dflat = np.full(4 * max(B, 1), -7.0)
    rc = drv.cd_round_trip(mf.ctypes.data, M, pf.ctypes.data, Q, T16.ctypes.data, B, sg.ctypes.data, len(sg), float(outlier), steps, nlhs,
                           To.ctypes.data, dflat.ctypes.data, n.ctypes.data, C.byref(n_out), e, 1024)
    dbl = dflat[:4 * B].reshape(4, B) if B else np.zeros((4, 0))
    return rc, e.value.decode(), n_out.value, To[:B], dbl, n[:B]


def test_model_refit_cpd_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, m[:5], T16, 0.0, 0.1, 1, 6)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.cd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, steps", [(4096, 777, 5, 1), (4096, 777, 5, 3), (0, 9, 3, 1), (500, 0, 2, 1), (500, 20, 0, 1)])
def test_model_refit_cpd_round_trip_equals_the_host_tier(drv, M, Q, B, steps):
    """[Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = pcreg_mex('modelRefitCpd', h, single(pts), T, sigma2, outlier, steps) with 1 and
    with 6 outputs, a variance for all pages and one per page: a zero page for an empty result; the same bits as Model.refit_cpd"""
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
    per = np.linspace(0.0, 2.0, B) if B else np.zeros(1)      # the first page asks for the initial variance
    for sigma2 in (0.0, per):
        with pc.Model(m) as h:
            want = h.refit_cpd(pts, T, sigma2=sigma2 if B else 0.0, outlier=0.2, steps=steps)
        for nlhs in (1, 6):
            rc, msg, n_out, To, dbl, n = _round_trip(drv, m, pts, T16, sigma2, 0.2, steps, nlhs)
            assert rc == 0, msg
            assert n_out == nlhs and drv.cd_live_arrays() == 0
            got = np.ascontiguousarray(To.reshape(B, 4, 4).transpose(0, 2, 1))              # page b, column-major
            np.testing.assert_array_equal(got.view(np.uint64), want["T"].view(np.uint64))
            for b in range(B):
                assert want["empty"][b] == (not got[b].any())                               # a zero page for an empty result
            if nlhs == 6:
                for row, key in zip(dbl, ("sigma2", "Np", "sum_res2", "sum_d2")):
                    np.testing.assert_array_equal(row.view(np.uint64), want[key].view(np.uint64))
                np.testing.assert_array_equal(n, want["n_live"])
        if M >= 4096 and Q >= 777 and B:
            assert not want["empty"][0] and want["Np"][0] > 1 and want["empty"][2] and want["n_live"].tolist() == [Q, Q, 0, Q, Q]
        if M == 0 or Q == 0:
            assert want["empty"].all()


def test_refit_cpd_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "refitCpdModel.m")).read()
    assert src.startswith("function [Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = refitCpdModel(h, pts, T, sigma2, outlier, steps)")
    assert "[Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = pcreg_mex('modelRefitCpd', h, single(pts), double(T), double(sigma2), double(outlier), " \
           "double(steps));" in src                                                                      # 7 arguments, 6 outputs
    assert "if nargin < 4, sigma2 = 0; end" in src and "if nargin < 5, outlier = 0.1; end" in src and "if nargin < 6, steps = 1; end" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelRefitCpd")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 7\b", block) and "plhs[5]" in block and "pcreg_model_refit_cpd_f32(" in block
    head = gw[:gw.index("#if __has_include")]
    assert "'modelRefitCpd'" in head and "refitCpdModel.m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "refitCpdModel" in integ and "pcreg_model_refit_cpd_f32" in integ
