"""The denoising's C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (k outside
[1, 31], a negative or non-finite threshold, null pointers, bad sizes, a short workspace) are PCREG_E_ARG before anything runs; a
valid call without a device is PCREG_E_NODEVICE; the workspace is the one formula the header states."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_denoise_workspace", "pcreg_dev_model_denoise_f32", "pcreg_model_denoise_f32", "pcreg_point_denoise_f32")


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
    assert "point_denoise" in pc.__all__ and hasattr(pc, "point_denoise") and hasattr(pc.Model, "denoise")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "denoise")


def _stated(M):
    """denoise_ws_layout as include/pcreg.h states it"""
    r256 = lambda b: -(-b // 256) * 256
    R, Cn = max(M, 1), max(-(-M // 2048), 1)
    return r256(4 * R) + r256(8 * R) + 2 * r256(8 * Cn) + 2 * r256(4 * Cn) + 256


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_denoise_workspace
    for M in (0, 1, 2048, 2049, 65536, 1000000, (1 << 31) - 1):
        assert f(M, 1) == f(M, 31) == _stated(M), M
    assert _stated(0) == _stated(1) == 1792 and _stated(2048) == 8192 + 16384 + 4 * 256 + 256
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "roundup(4 R, 256) + roundup(8 R, 256) + 2 roundup(8 C, 256) + 2 roundup(4 C, 256) + 256 bytes" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    md = np.zeros(64, np.float64)
    inl = np.zeros(64, np.int32)
    n = C.c_int32(-5)
    st = np.zeros(4, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 20)
    E = _l.PCREG_E_ARG
    for k in (0, 32, -1, 33):
        assert L.pcreg_point_denoise_f32(p(pts), 8, 8, k, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
        assert L.pcreg_model_denoise_f32(fake, k, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
        assert L.pcreg_dev_model_denoise_f32(fake, k, 1.0, p(md), p(inl), C.byref(n), p(st), p(pts), big, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    for t in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        assert L.pcreg_point_denoise_f32(p(pts), 8, 8, 4, t, p(md), p(inl), C.byref(n), p(st)) == E
        assert L.pcreg_model_denoise_f32(fake, 4, t, p(md), p(inl), C.byref(n), p(st)) == E
        assert L.pcreg_dev_model_denoise_f32(fake, 4, t, p(md), p(inl), C.byref(n), p(st), p(pts), big, None) == E
    # ldm < M, a negative M, null pointers, inliers without their count
    assert L.pcreg_point_denoise_f32(p(pts), 8, 7, 4, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
    assert L.pcreg_point_denoise_f32(p(pts), -1, 8, 4, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
    assert L.pcreg_point_denoise_f32(None, 8, 8, 4, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
    assert L.pcreg_point_denoise_f32(p(pts), 8, 8, 4, 1.0, p(md), p(inl), None, p(st)) == E
    assert L.pcreg_model_denoise_f32(None, 4, 1.0, p(md), p(inl), C.byref(n), p(st)) == E
    assert L.pcreg_model_denoise_f32(fake, 4, 1.0, p(md), p(inl), None, p(st)) == E
    assert L.pcreg_dev_model_denoise_f32(None, 4, 1.0, p(md), p(inl), C.byref(n), p(st), p(pts), big, None) == E
    assert L.pcreg_dev_model_denoise_f32(fake, 4, 1.0, p(md), p(inl), C.byref(n), p(st), None, big, None) == E
    assert L.pcreg_dev_model_denoise_f32(fake, 4, 1.0, p(md), p(inl), None, p(st), p(pts), big, None) == E
    # a workspace one byte short of what the smallest model needs (a given model's own size is checked with the handle in hand)
    short = C.c_size_t(L.pcreg_dev_model_denoise_workspace(0, 4) - 1)
    assert L.pcreg_dev_model_denoise_f32(fake, 4, 1.0, p(md), p(inl), C.byref(n), p(st), p(pts), short, None) == E
    assert n.value == -5 and not md.any() and not st.any()          # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    md = np.zeros(64, np.float64)
    inl = np.zeros(64, np.int32)
    n = C.c_int32(0)
    st = np.zeros(4, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_point_denoise_f32(p(pts), 8, 9, 4, 1.0, p(md), p(inl), C.byref(n), p(st)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_denoise_f32(p(pts), 8, 8, 31, 0.0, None, None, None, None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_denoise(np.ones((7, 3)))
    assert e.value.code == _l.PCREG_E_NODEVICE


def test_point_denoise_rejects_bad_arguments():
    import pcreg_amd as pc
    for bad in (0, 32):
        with pytest.raises(ValueError):
            pc.point_denoise(np.ones((7, 3)), bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.point_denoise(np.ones((7, 3)), 4, bad)
    for shape in ((7, 2), (7, 4), (7,), (2, 7, 3)):
        with pytest.raises(ValueError):
            pc.point_denoise(np.ones(shape))
