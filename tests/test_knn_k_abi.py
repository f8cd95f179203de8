"""The k-nearest search's C ABI and MEX command without a GPU: the five entry points are exported and declared, argument
errors (k outside [1, 32], null pointers, bad sizes) are PCREG_E_ARG before anything runs, a valid call without a device is
PCREG_E_NODEVICE; the 'modelKnn' command of mex/pcreg_mex.cpp (tests/mexknn/knn_driver.cpp on tests/mexstub/mex.h) refuses
bad usage through mexErrMsgIdAndTxt and leaks no array.  GPU: one MEX round trip equals the ctypes path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_knn_workspace", "pcreg_dev_model_knn_f32", "pcreg_dev_merge_topk_f32", "pcreg_model_knn_f32", "pcreg_knn_points_f32")


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
    assert "#define PCREG_KNN_MAX_K 32" in head
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in head, name
        assert name in _l.SYMBOLS, name
    assert _l.KNN_MAX_K == 32


def test_workspace_is_linear_in_Q_and_independent_of_k():
    _, L = _lib()
    f = L.pcreg_dev_model_knn_workspace
    assert f(0, 0, 1) > 0
    assert f(50_000, 1 << 20, 32) == f(50_000, 1 << 20, 1) == f(50_000, 100, 8)
    assert f(4_000_000, 1 << 20, 32) - f(2_000_000, 1 << 20, 32) <= 2 * 4 * 2_000_000 + 512


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(64 * 33, np.int32)
    fb = np.zeros(64 * 33, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    for k in (0, 33, -1):
        assert L.pcreg_knn_points_f32(p(buf), 4, 4, p(buf), 4, 4, k, p(ib), p(fb)) == E
        assert L.pcreg_model_knn_f32(fake, p(buf), 4, 4, k, p(ib), p(fb)) == E
        assert L.pcreg_dev_model_knn_f32(fake, p(buf), 4, 4, k, 0, p(ib), p(fb), p(buf), C.c_size_t(1 << 20), None) == E
        assert L.pcreg_dev_merge_topk_f32(p(ib), p(fb), 2, 4, k, C.c_size_t(0), p(ib), p(fb), None) == E
    assert b"bad argument" in L.pcreg_last_error()
    # null pointers
    assert L.pcreg_knn_points_f32(None, 4, 4, p(buf), 4, 4, 2, p(ib), p(fb)) == E
    assert L.pcreg_knn_points_f32(p(buf), 4, 4, None, 4, 4, 2, p(ib), p(fb)) == E
    assert L.pcreg_knn_points_f32(p(buf), 4, 4, p(buf), 4, 4, 2, None, p(fb)) == E
    assert L.pcreg_knn_points_f32(p(buf), 4, 4, p(buf), 4, 4, 2, p(ib), None) == E
    assert L.pcreg_model_knn_f32(None, p(buf), 4, 4, 2, p(ib), p(fb)) == E
    assert L.pcreg_dev_model_knn_f32(None, p(buf), 4, 4, 2, 0, p(ib), p(fb), p(buf), C.c_size_t(1 << 20), None) == E
    assert L.pcreg_dev_model_knn_f32(fake, p(buf), 4, 4, 2, 0, p(ib), p(fb), None, C.c_size_t(1 << 20), None) == E
    assert L.pcreg_dev_merge_topk_f32(None, p(fb), 2, 4, 2, C.c_size_t(0), p(ib), p(fb), None) == E
    # bad sizes: negative counts, ld < n, Q above 4 Mi, R < 1, a rank stride shorter than Q * k
    assert L.pcreg_knn_points_f32(p(buf), -1, 4, p(buf), 4, 4, 2, p(ib), p(fb)) == E
    assert L.pcreg_knn_points_f32(p(buf), 4, 3, p(buf), 4, 4, 2, p(ib), p(fb)) == E
    assert L.pcreg_knn_points_f32(p(buf), 4, 4, p(buf), 4, 3, 2, p(ib), p(fb)) == E
    assert L.pcreg_dev_model_knn_f32(fake, p(buf), (4 << 20) + 1, (4 << 20) + 1, 2, 0, p(ib), p(fb), p(buf), C.c_size_t(1 << 40), None) == E
    assert L.pcreg_dev_merge_topk_f32(p(ib), p(fb), 0, 4, 2, C.c_size_t(0), p(ib), p(fb), None) == E
    assert L.pcreg_dev_merge_topk_f32(p(ib), p(fb), 2, 4, 2, C.c_size_t(7), p(ib), p(fb), None) == E


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(64 * 32, np.int32)
    fb = np.zeros(64 * 32, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_knn_points_f32(p(buf), 4, 4, p(buf), 4, 4, 3, p(ib), p(fb)) == _l.PCREG_E_NODEVICE
    assert L.pcreg_dev_merge_topk_f32(p(ib), p(fb), 2, 4, 3, C.c_size_t(0), p(ib), p(fb), None) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    with pytest.raises(PcregError) as e:
        pc.knn_points(np.zeros((5, 3)), np.ones((7, 3)), 4)
    assert e.value.code == _l.PCREG_E_NODEVICE
    with pytest.raises(ValueError):
        pc.knn_points(np.zeros((5, 3)), np.ones((7, 3)), 33)


# ---- the MEX command ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexknn") / "libmexknn.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexknn", "knn_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    return C.CDLL(out)


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("nargs, as_double, k", [(2, 0, 3.0), (3, 1, 3.0), (3, 0, 0.0), (3, 0, 33.0), (3, 0, 2.5)])
def test_model_knn_usage_errors(drv, nargs, as_double, k):
    e = _err()
    assert drv.kd_usage(nargs, as_double, C.c_double(k), e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: modelKnn:"), e.value
    assert drv.kd_live_arrays() == 0


def test_model_knn_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.kd_usage(3, 0, C.c_double(3.0), e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.kd_live_arrays() == 0


def test_model_knn_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    idx = np.zeros(5 * 4, np.int32); d2 = np.zeros(5 * 4, np.float32); e = _err()
    assert drv.kd_round_trip(np.asfortranarray(m).ctypes.data_as(C.c_void_p), 20, np.asfortranarray(m[:5]).ctypes.data_as(C.c_void_p), 5, 4,
                             idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
    assert drv.kd_live_arrays() == 0


def test_knnsearch_wrapper_keeps_min_k_m_columns():
    src = open(os.path.join(ROOT, "matlab", "knnsearchModel.m")).read()
    assert "pcreg_mex('modelKnn', h, single(Y), K)" in src and "sqrt(double(D2" in src and "idx(1, :) > 0" in src


@pytest.mark.gpu
@pytest.mark.parametrize("M, k", [(3000, 8), (5, 8), (0, 2)])
def test_model_knn_round_trip_equals_the_ctypes_path(drv, M, k):
    import pcreg_amd as pc
    rng = np.random.default_rng(M + k)
    m = (rng.random((M, 3)) * 20).astype(np.float32)
    Y = (rng.random((777, 3)) * 22 - 1).astype(np.float32)
    Q = len(Y)
    idx = np.zeros(Q * k, np.int32); d2 = np.zeros(Q * k, np.float32); e = _err()
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    assert drv.kd_round_trip(mf.ctypes.data_as(C.c_void_p), M, np.asfortranarray(Y).ctypes.data_as(C.c_void_p), Q, k,
                             idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), e, 1024) == 0, e.value
    assert drv.kd_live_arrays() == 0
    with pc.Model(m) as h:
        ri, rd = h.knn(Y, k)
    assert np.array_equal(idx.reshape(k, Q).T, ri + 1)                     # 1-based, 0 past M
    assert np.array_equal(d2.reshape(k, Q).T.view(np.uint32), rd.view(np.uint32))
