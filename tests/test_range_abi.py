"""The radius search's C ABI and MEX command without a GPU: the five entry points are exported, declared and listed; argument
errors (a negative or NaN r2, null pointers, bad sizes, a negative capacity) are PCREG_E_ARG before anything runs; a valid call
without a device is PCREG_E_NODEVICE; the workspace is O(Q) and independent of M; "range_sort_cap" is a debug key; the
'modelRange' command of mex/pcreg_mex.cpp (tests/mexrange/range_driver.cpp on tests/mexstub/mex.h) refuses bad usage through
mexErrMsgIdAndTxt and leaks no array; matlab/rangesearchModel.m calls it the way the gateway checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_range_workspace", "pcreg_dev_model_range_count_f32", "pcreg_dev_model_range_fill_f32", "pcreg_model_range_f32",
       "pcreg_range_points_f32")
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
    assert '"range_sort_cap"' in head
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    assert callable(pc.rangesearch_points) and callable(pc.Model.rangesearch)
    assert callable(PreparedModel.rangesearch) and callable(PreparedModel.rangesearch_count)


def test_range_sort_cap_is_a_debug_key():
    _l, L = _lib()
    assert L.pcreg_debug_set(b"range_sort_cap", 16) == _l.PCREG_OK
    assert L.pcreg_debug_set(b"range_sort_cap", 0) == _l.PCREG_OK


def test_workspace_is_linear_in_Q_and_independent_of_M():
    """include/pcreg.h: 147 712 + 3 * roundup(4 * max(Q, 1), 256) bytes, 12 bytes per query."""
    _, L = _lib()
    f = L.pcreg_dev_model_range_workspace
    assert f(0, 0) > 0 and f(0, 0) == f(1, 0)
    for Q in (0, 1, 513, 50_000):
        assert f(Q, 0) == f(Q, 100) == f(Q, 1 << 20) == 147_712 + 3 * ((4 * max(Q, 1) + 255) // 256 * 256)
    assert 0 < f(4_000_000, 1 << 20) - f(2_000_000, 1 << 20) <= 12 * 2_000_000 + 3 * 256
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "147 712 + 3 * roundup(4 * max(Q, 1), 256)" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    fb = np.zeros(256, np.float32)
    so = np.zeros(65, np.int64)
    p = lambda a: a.ctypes.data
    fake = 16                                          # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    big = 1 << 40
    # the valid shapes of the calls below: host(fake, q, 4, 4, r2, cap, so, idx, dist) etc.
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, r2, 256, p(so), p(ib), p(fb)) == E, r2
        assert L.pcreg_model_range_f32(fake, p(buf), 4, 4, r2, 256, p(so), p(ib), p(fb)) == E
        assert L.pcreg_dev_model_range_count_f32(fake, p(buf), 4, 4, r2, p(ib), p(so), p(buf), big, None) == E
        assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, r2, 0, p(so), 256, p(ib), p(fb), p(buf), big, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    # null pointers
    assert L.pcreg_range_points_f32(None, 4, 4, p(buf), 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, None, 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 1.0, 256, None, p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 1.0, 256, p(so), None, p(fb)) == E       # capacity > 0 needs idx
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 1.0, 256, p(so), p(ib), None) == E
    assert L.pcreg_model_range_f32(None, p(buf), 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, None, 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, p(buf), 4, 4, 1.0, 256, None, p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, p(buf), 4, 4, 1.0, 256, p(so), None, p(fb)) == E
    assert L.pcreg_dev_model_range_count_f32(None, p(buf), 4, 4, 1.0, p(ib), p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, None, 4, 4, 1.0, p(ib), p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), 4, 4, 1.0, None, p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), 4, 4, 1.0, p(ib), None, p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), 4, 4, 1.0, p(ib), p(so), None, big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(None, p(buf), 4, 4, 1.0, 0, p(so), 256, p(ib), p(fb), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, 1.0, 0, None, 256, p(ib), p(fb), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, 1.0, 0, p(so), 256, None, p(fb), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, 1.0, 0, p(so), 256, p(ib), None, p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, 1.0, 0, p(so), 256, p(ib), p(fb), None, big, None) == E
    # bad sizes: negative counts, ld < n, Q above 4 Mi, a negative capacity
    assert L.pcreg_range_points_f32(p(buf), -1, 4, p(buf), 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 3, p(buf), 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), -1, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 3, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 1.0, -1, p(so), p(ib), p(fb)) == E
    assert L.pcreg_range_points_f32(p(buf), MAXQ + 1, MAXQ + 1, p(buf), 4, 4, 1.0, 0, p(so), None, None) == E
    assert L.pcreg_model_range_f32(fake, p(buf), -1, 4, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, p(buf), 4, 3, 1.0, 256, p(so), p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, p(buf), 4, 4, 1.0, -1, p(so), p(ib), p(fb)) == E
    assert L.pcreg_model_range_f32(fake, p(buf), MAXQ + 1, MAXQ + 1, 1.0, 0, p(so), None, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), -1, 4, 1.0, p(ib), p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), 4, 3, 1.0, p(ib), p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_count_f32(fake, p(buf), MAXQ + 1, MAXQ + 1, 1.0, p(ib), p(so), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 3, 1.0, 0, p(so), 256, p(ib), p(fb), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), 4, 4, 1.0, 0, p(so), -1, p(ib), p(fb), p(buf), big, None) == E
    assert L.pcreg_dev_model_range_fill_f32(fake, p(buf), MAXQ + 1, MAXQ + 1, 1.0, 0, p(so), 256, p(ib), p(fb), p(buf), big, None) == E
    # the Python tiers refuse a bad radius themselves
    import pcreg_amd as pc
    for r2 in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pc.rangesearch_points(np.zeros((5, 3)), np.ones((7, 3)), r2)


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    fb = np.zeros(256, np.float32)
    so = np.zeros(65, np.int64)
    p = lambda a: a.ctypes.data
    N = _l.PCREG_E_NODEVICE
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 1.0, 256, p(so), p(ib), p(fb)) == N
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, 0.0, 0, p(so), None, None) == N            # capacity 0: idx / dist may be null
    assert L.pcreg_range_points_f32(p(buf), 4, 4, p(buf), 4, 4, float("inf"), 0, p(so), None, None) == N
    assert L.pcreg_dev_model_range_count_f32(16, p(buf), 4, 4, 1.0, p(ib), p(so), p(buf), 1 << 20, None) == N
    assert L.pcreg_dev_model_range_fill_f32(16, p(buf), 4, 4, 1.0, 0, p(so), 0, None, None, p(buf), 1 << 20, None) == N
    with pytest.raises(PcregError) as e:
        pc.rangesearch_points(np.zeros((5, 3)), np.ones((7, 3)), 4.0)
    assert e.value.code == N


# ---- the MEX command ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexrange") / "libmexrange.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexrange", "range_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.rd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.rd_round_trip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_longlong), C.c_longlong,
                                C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, q_double, r_kind, r", [(2, 0, 0, 1.0), (4, 0, 0, 1.0), (3, 1, 0, 1.0), (3, 0, 0, -1.0), (3, 0, 0, float("nan")),
                                                        (3, 0, 1, 2.0), (3, 0, 2, 1.0)])
def test_model_range_usage_errors(drv, nargs, q_double, r_kind, r):
    """wrong argument counts, a double query, a negative / NaN radius, an int32 radius, a 1 x 2 radius"""
    e = _err()
    assert drv.rd_usage(nargs, q_double, r_kind, r, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelRange:"), e.value
    assert drv.rd_live_arrays() == 0


def test_model_range_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.rd_usage(3, 0, 0, 1.5, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.rd_live_arrays() == 0


def test_model_range_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.asfortranarray(np.random.default_rng(0).random((20, 3)).astype(np.float32))
    y = np.asfortranarray(m[:5])
    counts = np.zeros(5, np.int32); idx = np.zeros(64, np.int32); d2 = np.zeros(64, np.float32); e = _err(); total = C.c_longlong(-1)
    assert drv.rd_round_trip(m.ctypes.data, 20, y.ctypes.data, 5, 0.5, counts.ctypes.data, C.byref(total), 64, idx.ctypes.data, d2.ctypes.data,
                             e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
    assert drv.rd_live_arrays() == 0


def test_rangesearch_wrapper_calls_the_command_as_the_gateway_checks():
    src = open(os.path.join(ROOT, "matlab", "rangesearchModel.m")).read()
    assert "[counts, idx, D2] = pcreg_mex('modelRange', h, single(Y), r);" in src                 # 4 arguments, 3 outputs
    assert "mat2cell" in src and "sqrt(double(D2" in src
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    block = gw.split('strcmp(cmd, "modelRange")')[1].split("strcmp(cmd,")[0]
    assert re.search(r"nrhs != 4\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
    head = gw[:gw.index("#if __has_include")]
    assert "'modelRange'" in head and "rangesearchModel.m" in head
    assert not os.path.exists(os.path.join(ROOT, "matlab", "clusterPoints.m"))
