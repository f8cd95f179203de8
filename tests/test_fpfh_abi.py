"""The FPFH's C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (k outside [3, 32],
ldn < M, ldf < M, k_normals outside its range without normals, null pointers, bad sizes) are PCREG_E_ARG before anything runs; a
valid call without a device is PCREG_E_NODEVICE; the workspace is the one formula the header states."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fpfh_workspace", "pcreg_dev_model_fpfh_f32", "pcreg_model_fpfh_f32", "pcreg_point_fpfh_f32")


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
    assert "point_fpfh" in pc.__all__ and hasattr(pc, "point_fpfh") and hasattr(pc.Model, "fpfh")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "fpfh")


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_fpfh_workspace
    up = lambda x: -(-x // 256) * 256
    for M in (0, 1, 63, 64, 65, 512, 1 << 20, (1 << 31) - 1):
        R = max(M, 1)
        for k in (3, 8, 17, 32):
            assert f(M, k) == up(4 * R) + 2 * up(4 * R * k) + up(33 * R), (M, k)


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 33, np.float64)
    cnt = np.zeros(64 * 33, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    big = C.c_size_t(1 << 20)
    for k in (2, 33, 0, -1):
        assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, k, p(nrm), 8, 0, None, p(out), 8, p(cnt)) == E
        assert L.pcreg_model_fpfh_f32(fake, k, p(nrm), 8, 0, None, p(out), 8, None) == E
        assert L.pcreg_dev_model_fpfh_f32(fake, k, p(nrm), 8, p(out), None, p(pts), big, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    # ldn < M, ldf < M, ldm < M, a negative M, null pointers
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, p(nrm), 7, 0, None, p(out), 8, None) == E
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, p(nrm), 8, 0, None, p(out), 7, None) == E
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 7, 6, p(nrm), 8, 0, None, p(out), 8, None) == E
    assert L.pcreg_point_fpfh_f32(p(pts), -1, 8, 6, p(nrm), 8, 0, None, p(out), 8, None) == E
    assert L.pcreg_point_fpfh_f32(None, 8, 8, 6, p(nrm), 8, 0, None, p(out), 8, None) == E
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, p(nrm), 8, 0, None, None, 8, None) == E
    # no normals: k_normals has the normals' range
    for kn in (2, 33, 0, -1):
        assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, None, 0, kn, None, p(out), 8, None) == E
    assert L.pcreg_model_fpfh_f32(None, 6, p(nrm), 8, 0, None, p(out), 8, None) == E
    assert L.pcreg_dev_model_fpfh_f32(None, 6, p(nrm), 8, p(out), None, p(pts), big, None) == E
    assert L.pcreg_dev_model_fpfh_f32(fake, 6, p(nrm), 8, p(out), None, None, big, None) == E


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 33, np.float64)
    cnt = np.zeros(64 * 33, np.uint8)
    vp = (C.c_double * 3)(0.0, 0.0, 9.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, p(nrm), 9, 0, None, p(out), 9, p(cnt)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_fpfh_f32(p(pts), 8, 8, 6, None, 0, 5, vp, p(out), 8, None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fpfh(np.ones((7, 3)), 4)
    assert e.value.code == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fpfh(np.ones((7, 3)), 4, normals=np.ones((7, 3)))
    assert e.value.code == _l.PCREG_E_NODEVICE
    for bad in (2, 33):
        with pytest.raises(ValueError):
            pc.point_fpfh(np.ones((7, 3)), bad)
        with pytest.raises(ValueError):
            pc.point_fpfh(np.ones((7, 3)), 4, k_normals=bad)
    with pytest.raises(ValueError):
        pc.point_fpfh(np.ones((7, 3)), 4, normals=np.ones((6, 3)))
    with pytest.raises(ValueError):
        pc.point_fpfh(np.ones((7, 3)), 4, viewpoint=(1.0, 2.0))
