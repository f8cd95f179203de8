"""The normals' C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (k outside
[3, 32], ldn < M, null pointers, bad sizes) are PCREG_E_ARG before anything runs; a valid call without a device is
PCREG_E_NODEVICE; the workspace is the one formula the header states."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_normals_workspace", "pcreg_dev_model_normals_f32", "pcreg_model_normals_f32", "pcreg_point_normals_f32")


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
    assert "point_normals" in pc.__all__ and hasattr(pc.Model, "normals")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "normals")


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_normals_workspace
    for M in (0, 1, 63, 64, 65, 512, 1 << 20, (1 << 31) - 1):
        want = -(-4 * max(M, 1) // 256) * 256
        assert f(M, 3) == f(M, 32) == want, M


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    for k in (2, 33, 0, -1):
        assert L.pcreg_point_normals_f32(p(pts), 8, 8, k, None, p(out), 8, None) == E
        assert L.pcreg_model_normals_f32(fake, k, None, p(out), 8, None) == E
        assert L.pcreg_dev_model_normals_f32(fake, k, None, p(out), 8, None, p(pts), C.c_size_t(1 << 20), None) == E
    assert b"bad argument" in L.pcreg_last_error()
    # ldn < M, ldm < M, a negative M, null pointers
    assert L.pcreg_point_normals_f32(p(pts), 8, 8, 6, None, p(out), 7, None) == E
    assert L.pcreg_point_normals_f32(p(pts), 8, 7, 6, None, p(out), 8, None) == E
    assert L.pcreg_point_normals_f32(p(pts), -1, 8, 6, None, p(out), 8, None) == E
    assert L.pcreg_point_normals_f32(None, 8, 8, 6, None, p(out), 8, None) == E
    assert L.pcreg_point_normals_f32(p(pts), 8, 8, 6, None, None, 8, None) == E
    assert L.pcreg_model_normals_f32(None, 6, None, p(out), 8, None) == E
    assert L.pcreg_dev_model_normals_f32(None, 6, None, p(out), 8, None, p(pts), C.c_size_t(1 << 20), None) == E
    assert L.pcreg_dev_model_normals_f32(fake, 6, None, p(out), 8, None, None, C.c_size_t(1 << 20), None) == E


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 3, np.float32)
    var = np.zeros(64, np.float32)
    vp = (C.c_double * 3)(0.0, 0.0, 9.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_point_normals_f32(p(pts), 8, 8, 6, vp, p(out), 9, p(var)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    with pytest.raises(PcregError) as e:
        pc.point_normals(np.ones((7, 3)), 4)
    assert e.value.code == _l.PCREG_E_NODEVICE
    for bad in (2, 33):
        with pytest.raises(ValueError):
            pc.point_normals(np.ones((7, 3)), bad)
    with pytest.raises(ValueError):
        pc.point_normals(np.ones((7, 3)), 4, viewpoint=(1.0, 2.0))
