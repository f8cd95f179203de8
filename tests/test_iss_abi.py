"""The ISS keypoints' C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (a radius that
is zero, negative, subnormal, infinite or NaN, a threshold that is not finite or not > 0, min_neighbors < 1, 2^26 rows or more,
null pointers, bad sizes, keypoints without their count, a short workspace) are PCREG_E_ARG before anything runs; a valid call
without a device is PCREG_E_NODEVICE; the workspace is the one formula the header states."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_iss_workspace", "pcreg_dev_model_iss_f32", "pcreg_model_iss_f32", "pcreg_point_iss_f32")


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
    import pcreg_amd as pc
    assert "point_iss" in pc.__all__ and hasattr(pc, "point_iss") and hasattr(pc.Model, "iss_keypoints")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "iss_keypoints")


def _stated(M):
    """iss_ws_layout as include/pcreg.h states it"""
    r256 = lambda b: -(-b // 256) * 256
    R, Cn = max(M, 1), max(-(-M // 2048), 1)
    return r256(R) + r256(4 * Cn)


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_iss_workspace
    for M in (0, 1, 256, 257, 2048, 2049, 65536, 1000000, (1 << 26) - 1):
        assert f(M) == _stated(M), M
    assert _stated(0) == _stated(1) == 512 and _stated(2049) == 2304 + 256
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "roundup(R, 256) + roundup(4 C, 256) bytes" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    nn = np.zeros(64, np.int32)
    eig = np.zeros(64 * 3, np.float64)
    sal = np.zeros(64, np.float64)
    kp = np.zeros(64, np.int32)
    n = C.c_int32(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 20)
    E = _l.PCREG_E_ARG
    outs = (p(nn), p(eig), p(sal), p(kp), C.byref(n))

    def all_three(rs, rn, g21, g32, mn):
        assert L.pcreg_point_iss_f32(p(pts), 8, 8, rs, rn, g21, g32, mn, *outs) == E
        assert L.pcreg_model_iss_f32(fake, rs, rn, g21, g32, mn, *outs) == E
        assert L.pcreg_dev_model_iss_f32(fake, rs, rn, g21, g32, mn, *outs, p(pts), big, None) == E

    for bad in (0.0, -1.0, 1e-40, float("inf"), float("nan"), -float("inf")):
        all_three(bad, 4.0, 0.975, 0.975, 5)
        all_three(4.0, bad, 0.975, 0.975, 5)
    assert b"bad argument" in L.pcreg_last_error()
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        all_three(4.0, 4.0, bad, 0.975, 5)
        all_three(4.0, 4.0, 0.975, bad, 5)
    for bad in (0, -1):
        all_three(4.0, 4.0, 0.975, 0.975, bad)
    ok = (4.0, 4.0, 0.975, 0.975, 5)
    # ldm < M, a negative M, 2^26 rows, null pointers, keypoints without their count
    assert L.pcreg_point_iss_f32(p(pts), 8, 7, *ok, *outs) == E
    assert L.pcreg_point_iss_f32(p(pts), -1, 8, *ok, *outs) == E
    assert L.pcreg_point_iss_f32(p(pts), 1 << 26, 1 << 26, *ok, *outs) == E
    assert L.pcreg_point_iss_f32(None, 8, 8, *ok, *outs) == E
    assert L.pcreg_point_iss_f32(p(pts), 8, 8, *ok, None, p(eig), p(sal), p(kp), C.byref(n)) == E
    assert L.pcreg_point_iss_f32(p(pts), 8, 8, *ok, p(nn), p(eig), None, p(kp), C.byref(n)) == E
    assert L.pcreg_point_iss_f32(p(pts), 8, 8, *ok, p(nn), p(eig), p(sal), p(kp), None) == E
    assert L.pcreg_model_iss_f32(None, *ok, *outs) == E
    assert L.pcreg_model_iss_f32(fake, *ok, p(nn), p(eig), p(sal), p(kp), None) == E
    assert L.pcreg_dev_model_iss_f32(None, *ok, *outs, p(pts), big, None) == E
    assert L.pcreg_dev_model_iss_f32(fake, *ok, *outs, None, big, None) == E
    assert L.pcreg_dev_model_iss_f32(fake, *ok, p(nn), p(eig), p(sal), p(kp), None, p(pts), big, None) == E
    # a workspace one byte short of what the smallest model needs (a given model's own size is checked with the handle in hand)
    short = C.c_size_t(L.pcreg_dev_model_iss_workspace(0) - 1)
    assert L.pcreg_dev_model_iss_f32(fake, *ok, *outs, p(pts), short, None) == E
    assert n.value == -5 and not nn.any() and not sal.any() and not eig.any()          # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    nn = np.zeros(64, np.int32)
    sal = np.zeros(64, np.float64)
    kp = np.zeros(64, np.int32)
    n = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_point_iss_f32(p(pts), 8, 9, 4.0, 1.0, 0.975, 0.975, 5, p(nn), None, p(sal), p(kp), C.byref(n)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_iss_f32(p(pts), 8, 8, 2.0 ** -126, 3e38, 1e-300, 1e300, 1, p(nn), None, p(sal), None, None) == _l.PCREG_E_NODEVICE
    assert L.pcreg_point_iss_f32(None, 0, 0, 4.0, 1.0, 0.975, 0.975, 5, None, None, None, None, C.byref(n)) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_iss(np.ones((7, 3)), 2.0, 1.0)
    assert e.value.code == _l.PCREG_E_NODEVICE


def test_point_iss_rejects_bad_arguments_and_squares_in_double():
    import pcreg_amd as pc
    from pcreg_amd.api import iss_args
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        with pytest.raises(ValueError):
            pc.point_iss(np.ones((7, 3)), bad, 1.0)
        with pytest.raises(ValueError):
            pc.point_iss(np.ones((7, 3)), 1.0, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.point_iss(np.ones((7, 3)), 1.0, 1.0, bad, 0.9)
        with pytest.raises(ValueError):
            pc.point_iss(np.ones((7, 3)), 1.0, 1.0, 0.9, bad)
    with pytest.raises(ValueError):
        pc.point_iss(np.ones((7, 3)), 1.0, 1.0, 0.9, 0.9, 0)
    for shape in ((7, 2), (7, 4), (7,), (2, 7, 3)):
        with pytest.raises(ValueError):
            pc.point_iss(np.ones(shape), 1.0, 1.0)
    # 0.1 as a double squared and rounded once, not float32(0.1) squared in single
    r2s, r2n, g21, g32, mn = iss_args(0.1, 1.7, 0.975, 0.5, 5)
    assert r2s == float(np.float32(0.1 * 0.1)) and r2n == float(np.float32(1.7 * 1.7)) and (g21, g32, mn) == (0.975, 0.5, 5)
    assert np.float32(0.1) * np.float32(0.1) != np.float32(0.1 * 0.1)
