"""The transform scoring's C ABI, MEX command and MATLAB wrapper.  Without a GPU: the three entry points are exported, declared and
listed; argument errors (a negative or NaN r2, null pointers, bad sizes, a workspace one byte short) are PCREG_E_ARG before anything
runs; a valid call without a device is PCREG_E_NODEVICE; "score_batch_slots" is a debug key; the 'modelScore' command of
mex/pcreg_mex.cpp (tests/mexscore/score_driver.cpp on tests/mexstub/mex.h) refuses bad usage through mexErrMsgIdAndTxt and leaks no
array; matlab/scoreTransformsModel.m calls it the way the gateway checks.  With one: the round trip equals the ctypes path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_score_workspace", "pcreg_dev_model_score_f32", "pcreg_model_score_f32")
MAXQ = 4 << 20


def _lib():
    from pcreg_amd import _lib
    return _lib, _lib.lib()


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def test_new_symbols_are_declared_exported_and_listed():
    _l, L = _lib()
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in head, name
        assert name in _l.SYMBOLS, name
    assert '"score_batch_slots"' in head
    assert L.pcreg_debug_set(b"score_batch_slots", 1000) == _l.PCREG_OK
    assert L.pcreg_debug_set(b"score_batch_slots", 0) == _l.PCREG_OK
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    from pcreg_amd.sweep import score_trials
    assert callable(pc.Model.score_transforms) and callable(PreparedModel.score_transforms) and callable(score_trials)


def test_workspace_follows_the_header_and_is_bounded():
    _, L = _lib()
    f = L.pcreg_dev_model_score_workspace
    up = lambda x: (x + 255) // 256 * 256
    for Q, B in ((0, 0), (1, 1), (3000, 8), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        nb = max(1, min(B, MAXQ // max(Q, 1)))
        S, P = max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)
        assert f(Q, B, 0) == f(Q, B, 1 << 20) == 131_328 + up(12 * S) + 2 * up(4 * S) + up(8 * P) + up(4 * P), (Q, B)
    assert f(50_000, 107, 0) == f(50_000, 83, 0) == f(50_000, 1 << 20, 0)         # 83 transforms fill the 4 Mi slots
    assert f(1, 1 << 30, 0) <= 131_328 + 40 * MAXQ
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "131 328 + roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256)" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    T = np.zeros(3 * 16, np.float64)
    n = np.zeros(3, np.int32)
    s = np.zeros(3, np.float64)
    p = lambda a: a.ctypes.data
    fake, big, E = 16, 1 << 40, _l.PCREG_E_ARG               # (the handle is never dereferenced: the checks refuse first)
    dev = lambda h=fake, q=p(buf), Q=4, ldq=4, t=p(T), B=3, r2=1.0, nc=p(n), sd=p(s), ws=p(buf), wsb=big: \
        L.pcreg_dev_model_score_f32(h, q, Q, ldq, t, B, r2, nc, sd, None, None, ws, wsb, None)
    host = lambda h=fake, q=p(buf), Q=4, ldq=4, t=p(T), B=3, r2=1.0, nc=p(n), sd=p(s): L.pcreg_model_score_f32(h, q, Q, ldq, t, B, r2, nc, sd, None, None)
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert dev(r2=r2) == E and host(r2=r2) == E, r2
    assert b"bad argument" in L.pcreg_last_error()
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(nc=None), dict(sd=None), dict(Q=-1), dict(B=-1), dict(ldq=3),
               dict(Q=MAXQ + 1, ldq=MAXQ + 1)):
        assert dev(**kw) == E and host(**kw) == E, kw
    assert dev(ws=None) == E
    need = L.pcreg_dev_model_score_workspace(4, 3, 0)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    from pcreg_amd.api import _transforms16
    with pytest.raises(ValueError):
        _transforms16([np.eye(3)])


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    T = np.zeros(3 * 16, np.float64)
    n = np.zeros(3, np.int32)
    s = np.zeros(3, np.float64)
    p = lambda a: a.ctypes.data
    need = L.pcreg_dev_model_score_workspace(4, 3, 0)
    assert L.pcreg_dev_model_score_f32(16, p(buf), 4, 4, p(T), 3, 1.0, p(n), p(s), None, None, p(buf), need, None) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_dev_model_score_f32(16, p(buf), 4, 4, p(T), 3, float("inf"), p(n), p(s), None, None, p(buf), need, None) == _l.PCREG_E_NODEVICE


# ---- the MEX command ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexscore") / "libmexscore.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexscore", "score_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.sd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.sd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, pts_double, t_kind, r_kind, r", [(3, 0, 0, 0, 1.0), (5, 0, 0, 0, 1.0), (4, 1, 0, 0, 1.0), (4, 0, 1, 0, 1.0),
                                                                  (4, 0, 2, 0, 1.0), (4, 0, 0, 0, -1.0), (4, 0, 0, 0, float("nan")), (4, 0, 0, 1, 2.0)])
def test_model_score_usage_errors(drv, nargs, pts_double, t_kind, r_kind, r):
    """wrong argument counts, a double cloud, a 3 x 4 T, a single T, a negative / NaN radius, an int32 radius"""
    e = _err()
    assert drv.sd_usage(nargs, pts_double, t_kind, r_kind, r, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelScore:"), e.value
    assert drv.sd_live_arrays() == 0


def test_model_score_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.sd_usage(4, 0, 0, 0, 1.5, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.sd_live_arrays() == 0


def _round_trip(drv, m, pts, T16, r, nlhs):
    M, Q, B = len(m), len(pts), len(T16)
    n = np.full(max(B, 1), -7, np.int32); s = np.full(max(B, 1), -7.0, np.float64)
    idx = np.full((max(B, 1), max(Q, 1)), -7, np.int32); d2 = np.full((max(B, 1), max(Q, 1)), -7.0, np.float32)
    e = _err(); n_out = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    pf = np.asfortranarray(pts) if Q else np.zeros((1, 3), np.float32, order="F")
    rc = drv.sd_round_trip(mf.ctypes.data, M, pf.ctypes.data, Q, T16.ctypes.data, B, float(r), nlhs, n.ctypes.data, s.ctypes.data,
                           idx.ctypes.data, d2.ctypes.data, C.byref(n_out), e, 1024)
    return rc, e.value.decode(), n_out.value, n[:B], s[:B], idx, d2


def test_model_score_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    rc, msg, *_ = _round_trip(drv, m, m[:5], T16, 0.5, 4)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.sd_live_arrays() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M, Q, B, r", [(3000, 777, 5, 1.5), (5, 40, 2, 40.0), (0, 9, 3, 1.0), (3000, 300, 4, 0.0), (500, 0, 2, 1.0), (500, 20, 0, 1.0)])
def test_model_score_round_trip_equals_the_host_tier(drv, M, Q, B, r):
    """[nClose, sumD2, idx, D2] = pcreg_mex('modelScore', h, single(pts), T, maxDist) with 2 and with 4 outputs: 1-based rows, 0
    for none, maxDist squared once in single; the same bits as Model.score_transforms"""
    import pcreg_amd as pc
    rng = np.random.default_rng(M + Q)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    pts = np.vstack([(rng.random((Q - min(M, Q, 50), 3)) * 22 - 1).astype(np.float32), m[:min(M, Q, 50)]]) if Q else np.zeros((0, 3), np.float32)
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(1, B):
        T[b, 3, :3] = rng.normal(size=3) * 0.2 * b
    if B > 2:
        T[2] = 0.0
    T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)
    with pc.Model(m) as h:
        want = h.score_transforms(pts, T, np.float32(r) * np.float32(r), rows=True)
    for nlhs in (2, 4):
        rc, msg, n_out, n, s, idx, d2 = _round_trip(drv, m, pts, T16, r, nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.sd_live_arrays() == 0
        np.testing.assert_array_equal(n, want["n_close"])
        np.testing.assert_array_equal(s.view(np.uint64), want["sum_d2"].view(np.uint64))
        if nlhs == 4 and B * Q:
            got_i = idx.reshape(-1)[:B * Q].reshape(B, Q)                 # Q x B column-major = [B][Q]
            got_d = d2.reshape(-1)[:B * Q].reshape(B, Q)
            np.testing.assert_array_equal(got_i, want["idx"] + 1)
            np.testing.assert_array_equal(got_d.view(np.uint32), want["dist"].view(np.uint32))
            assert (got_i >= 0).all() and ((got_i == 0) == np.isposinf(got_d)).all()
        elif nlhs == 2:
            assert (idx == -7).all() and (d2 == -7.0).all()                # the last two outputs were not built
    if M >= 500 and Q and B:
        assert want["n_close"][0] >= min(Q, 50) and (B < 3 or want["n_close"][2] == 0)


def test_score_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "scoreTransformsModel.m")).read()
    assert src.startswith("function [fitness, rmse, nClose, idx, D2] = scoreTransformsModel(h, pts, T, maxDist, invert)")
    assert "[nClose, sumD2, idx, D2] = pcreg_mex('modelScore', h, single(pts), A, maxDist);" in src      # 5 arguments, 4 outputs
    assert "[nClose, sumD2] = pcreg_mex('modelScore', h, single(pts), A, maxDist);" in src                # ... or 2
    assert "iscell(T)" in src and "isempty(T{b})" in src and "invertTF(" in src                          # the cell and the array form
    assert "fitness = double(nClose) / size(pts, 1);" in src and "rmse = sqrt(sumD2 ./ double(nClose));" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelScore")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 5\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 3
    assert "nlhs > 2" in block and "r * r" in block
    head = gw[:gw.index("#if __has_include")]
    assert "'modelScore'" in head and "scoreTransformsModel.m" in head
