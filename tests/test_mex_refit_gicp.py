"""The plane-to-plane refit's MEX command and MATLAB wrapper, in the manner of tests/test_mex_refit_plane.py.  Without a GPU: the
'modelRefitGicp' command of mex/pcreg_mex.cpp (tests/mexrefitgicp/refit_gicp_driver.cpp on tests/mexstub/mex.h) refuses bad
usage through mexErrMsgIdAndTxt and leaks no array; matlab/refitGicpModel.m calls it the way the gateway checks.  With one: the
round trip -- 4 x 4 x B in and out, a zero page for an empty result, either set of normals given and [] -- equals the ctypes
path bit for bit."""
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
    out = str(tmp_path_factory.mktemp("mexrefitgicp") / "libmexrefitgicp.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexrefitgicp", "refit_gicp_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.gd_usage.argtypes = [C.c_int] * 5 + [C.c_double] * 4 + [C.c_char_p, C.c_int]
    L.gd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


OK = dict(nargs=9, pts_double=0, t_kind=0, n_kind=0, q_kind=0, r=1.0, steps=1.0, k=6.0, epsilon=1e-3)


@pytest.mark.parametrize("kw", [
    dict(nargs=8), dict(nargs=10), dict(pts_double=1), dict(t_kind=1), dict(r=-1.0), dict(r=float("nan")), dict(steps=0.0), dict(steps=1.5),
    dict(steps=float("nan")), dict(n_kind=1), dict(n_kind=2), dict(q_kind=1), dict(q_kind=2), dict(k=2.0), dict(k=33.0), dict(k=6.5),
    dict(epsilon=0.0), dict(epsilon=-1e-3), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(epsilon=float("inf"))],
    ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_model_refit_gicp_usage_errors(drv, kw):
    """wrong argument counts, a double cloud, a 3 x 4 T, a negative / NaN radius, steps 0, fractional or NaN, double or two-column
    normals on either side, k 2, 33 or fractional, epsilon 0, negative, above 1, NaN or inf"""
    a = dict(OK, **kw)
    e = _err()
    assert drv.gd_usage(a["nargs"], a["pts_double"], a["t_kind"], a["n_kind"], a["q_kind"], a["r"], a["steps"], a["k"], a["epsilon"], e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelRefitGicp:"), e.value
    assert drv.gd_live_arrays() == 0


@pytest.mark.parametrize("epsilon, q_kind", [(1e-3, 0), (1.0, 3), (5e-324, 0)])
def test_model_refit_gicp_null_handle_is_a_library_error(drv, epsilon, q_kind):
    e = _err()
    assert drv.gd_usage(9, 0, 0, 0, q_kind, 1.5, 2.0, 6.0, epsilon, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.gd_live_arrays() == 0


def _round_trip(drv, m, pts, T16, r, steps, normals, qnormals, k, epsilon, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    To = np.full((max(B, 1), 16), -7.0)
    n, npr = (np.full(max(B, 1), -7, np.int32) for _ in range(2))
    s, res = (np.full(max(B, 1), -7.0, np.float64) for _ in range(2))
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts) if Q else np.zeros((1, 3), np.float32, order="F")
    col = lambda a: None if a is None else np.asfortranarray(a, np.float32) if len(a) else np.zeros((1, 3), np.float32, order="F")
    nf, qf = col(normals), col(qnormals)
    rc = drv.gd_round_trip(mf.ctypes.data, M, pf.ctypes.data, Q, T16.ctypes.data, B, float(r), steps, None if nf is None else nf.ctypes.data,
                           0 if normals is None else len(normals), None if qf is None else qf.ctypes.data, 0 if qnormals is None else len(qnormals),
                           k, float(epsilon), nlhs, To.ctypes.data, n.ctypes.data, s.ctypes.data, npr.ctypes.data, res.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, To[:B], n[:B], s[:B], npr[:B], res[:B]


def test_model_refit_gicp_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, m[:5], T16, 0.5, 1, None, None, 6, 1e-3, 5)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.gd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, steps", [(4096, 777, 5, 1), (4096, 777, 5, 3), (0, 9, 3, 1), (500, 0, 2, 1), (500, 20, 0, 1)])
def test_model_refit_gicp_round_trip_equals_the_host_tier(drv, M, Q, B, steps):
    """[Tout, nClose, sumD2, nPairs, sumRes2] = pcreg_mex('modelRefitGicp', h, single(pts), T, maxDist, steps, normals, ptsNormals, k,
    epsilon) with 1 and with 5 outputs, with given normals and with [] on either side: maxDist squared once in single, a zero page
    for an empty result; the same bits as Model.refit_gicp"""
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
    r, eps = 1.5, 1e-2
    r2 = np.float32(r) * np.float32(r)
    with pc.Model(m) as h, pc.Model(pts) as hq:
        given, given_q = h.normals(8), hq.normals(8)
        wants = {"given": (given, given_q, h.refit_gicp(pts, T, r2, steps=steps, normals=given, query_normals=given_q, epsilon=eps)),
                 "computed": (None, None, h.refit_gicp(pts, T, r2, steps=steps, k=8, epsilon=eps)),
                 "mixed": (given, None, h.refit_gicp(pts, T, r2, steps=steps, normals=given, k=8, epsilon=eps))}
    for how, (nr, nq, want) in wants.items():
        for nlhs in (1, 5):
            rc, msg, n_out, To, n, s, npr, res = _round_trip(drv, m, pts, T16, r, steps, nr, nq, 8, eps, nlhs)
            assert rc == 0, msg
            assert n_out == nlhs and drv.gd_live_arrays() == 0
            got = np.ascontiguousarray(To.reshape(B, 4, 4).transpose(0, 2, 1))              # page b, column-major
            np.testing.assert_array_equal(got.view(np.uint64), want["T"].view(np.uint64))
            for b in range(B):
                assert want["empty"][b] == (not got[b].any())                               # a zero page for an empty result
            if nlhs == 5:
                np.testing.assert_array_equal(n, want["n_close"])
                np.testing.assert_array_equal(s.view(np.uint64), want["sum_d2"].view(np.uint64))
                np.testing.assert_array_equal(npr, want["n_pairs"])
                np.testing.assert_array_equal(res.view(np.uint64), want["sum_res2"].view(np.uint64))
        if M >= 4096 and Q >= 777 and B:
            assert not want["empty"][0] and want["n_pairs"][0] >= 700 and want["empty"][2]
        if M == 0 or Q == 0:
            assert want["empty"].all()


def test_refit_gicp_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "refitGicpModel.m")).read()
    assert src.startswith("function [Tout, nClose, sumD2, nPairs, sumRes2] = refitGicpModel(h, pts, T, maxDist, steps, normals, ptsNormals, k, epsilon)")
    assert "[Tout, nClose, sumD2, nPairs, sumRes2] = pcreg_mex('modelRefitGicp', h, single(pts), double(T), maxDist, double(steps), single(normals), " \
           "single(ptsNormals), double(k), double(epsilon));" in src                                     # 10 arguments, 5 outputs
    assert "if nargin < 5, steps = 1; end" in src and "if nargin < 6, normals = []; end" in src and "if nargin < 7, ptsNormals = []; end" in src
    assert "if nargin < 8, k = 6; end" in src and "if nargin < 9, epsilon = 1e-3; end" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelRefitGicp")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 10\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 4
    assert "r * r" in block and "pcreg_model_refit_gicp_f32(" in block
    head = gw[:gw.index("#if __has_include")]
    assert "'modelRefitGicp'" in head and "refitGicpModel.m" in head
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "refitGicpModel" in integ and "pcreg_model_refit_gicp_f32" in integ
