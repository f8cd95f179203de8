"""The radius FPFH's C ABI without a GPU: the five entry points are exported, declared and listed; argument errors (a NaN or negative
r2, max_neighbors < 0, M above 4 Mi, ldn < M, ldf < M, k_normals outside its range without normals, null pointers, bad sizes, a
workspace one byte short) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE; the workspace is
the one formula the header states."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fpfh_radius_workspace", "pcreg_dev_model_fpfh_radius_count_f32", "pcreg_dev_model_fpfh_radius_f32",
       "pcreg_model_fpfh_radius_f32", "pcreg_point_fpfh_radius_f32")


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
        assert getattr(L, name).argtypes is not None, name
    assert L.pcreg_dev_model_fpfh_radius_workspace.restype is C.c_size_t
    assert len(L.pcreg_dev_model_fpfh_radius_count_f32.argtypes) == 7 and len(L.pcreg_dev_model_fpfh_radius_f32.argtypes) == 13
    assert len(L.pcreg_model_fpfh_radius_f32.argtypes) == 11 and len(L.pcreg_point_fpfh_radius_f32.argtypes) == 13
    import pcreg_amd as pc
    assert "point_fpfh_radius" in pc.__all__ and hasattr(pc, "point_fpfh_radius") and hasattr(pc.Model, "fpfh_radius")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "fpfh_radius") and hasattr(PreparedModel, "fpfh_radius_count")
    assert '"fpfh_radius_lanes"' in head
    assert L.pcreg_debug_set(b"fpfh_radius_lanes", 16) == _l.PCREG_OK and L.pcreg_debug_set(b"fpfh_radius_lanes", 0) == _l.PCREG_OK


def test_workspace_is_the_stated_formula():
    """the radius search's own workspace for M queries, the lists (4 + 4 bytes an entry), m_j and the uint32 counts"""
    _, L = _lib()
    f = L.pcreg_dev_model_fpfh_radius_workspace
    up = lambda x: -(-x // 256) * 256
    for M in (0, 1, 63, 64, 65, 512, 1 << 20, 4 << 20):
        R = max(M, 1)
        for cap in (0, 1, 64, 65, 12345, 50 << 20, 1 << 33):
            want = L.pcreg_dev_model_range_workspace(M, M) + 2 * up(4 * cap) + up(4 * R) + up(132 * R)
            assert f(M, cap) == want, (M, cap)
    assert f(100, -5) == f(100, 0)


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 33, np.float64)
    cnt = np.zeros(64 * 33, np.uint32)
    nn = np.zeros(64, np.int32)
    seg = np.zeros(65, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    E = _l.PCREG_E_ARG
    big = C.c_size_t(1 << 30)
    point = lambda **kw: L.pcreg_point_fpfh_radius_f32(*[kw.get(k, d) for k, d in (
        ("m", p(pts)), ("M", 8), ("ldm", 8), ("r2", 4.0), ("n", 0), ("nrm", p(nrm)), ("ldn", 8), ("kn", 0), ("vp", None), ("out", p(out)),
        ("ldf", 8), ("cnt", p(cnt)), ("nn", p(nn)))])
    # a radius the radius search refuses, a negative max_neighbors
    for r2 in (float("nan"), -1.0, -float("inf")):
        assert point(r2=r2) == E
        assert L.pcreg_model_fpfh_radius_f32(None, r2, 0, p(nrm), 8, 0, None, p(out), 8, None, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    assert point(n=-1) == E
    # ldn < M, ldf < M, ldm < M, a negative M, M above 4 Mi, null pointers
    assert point(ldn=7) == E
    assert point(ldf=7) == E
    assert point(ldm=7) == E
    assert point(M=-1) == E
    too_many = (4 << 20) + 1
    assert point(M=too_many, ldm=too_many, ldn=too_many, ldf=too_many) == E
    assert point(m=None) == E
    assert point(out=None) == E
    # no normals: k_normals has the normals' range
    for kn in (2, 33, 0, -1):
        assert point(nrm=None, ldn=0, kn=kn) == E
    assert L.pcreg_model_fpfh_radius_f32(None, 4.0, 0, p(nrm), 8, 0, None, p(out), 8, None, None) == E
    # the device tier: a null model, workspace or seg_off
    assert L.pcreg_dev_model_fpfh_radius_count_f32(None, 4.0, p(nn), p(seg), p(pts), big, None) == E
    assert L.pcreg_dev_model_fpfh_radius_f32(None, 4.0, 0, p(nrm), 8, p(seg), 0, p(out), None, None, p(pts), big, None) == E


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 33, np.float64)
    cnt = np.zeros(64 * 33, np.uint32)
    nn = np.zeros(64, np.int32)
    vp = (C.c_double * 3)(0.0, 0.0, 9.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_point_fpfh_radius_f32(p(pts), 8, 8, 4.0, 50, p(nrm), 9, 0, None, p(out), 9, p(cnt), p(nn)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_fpfh_radius_f32(p(pts), 8, 8, float("inf"), 0, None, 0, 5, vp, p(out), 8, None, None) == _l.PCREG_E_NODEVICE
    assert L.pcreg_point_fpfh_radius_f32(p(pts), 8, 8, 0.0, 0, None, 0, 5, None, p(out), 8, None, None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fpfh_radius(np.ones((7, 3)), 2.0)
    assert e.value.code == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fpfh_radius(np.ones((7, 3)), 2.0, normals=np.ones((7, 3)), max_neighbors=50, counts=True, n_neighbors=True)
    assert e.value.code == _l.PCREG_E_NODEVICE
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pc.point_fpfh_radius(np.ones((7, 3)), bad)
    with pytest.raises(ValueError):
        pc.point_fpfh_radius(np.ones((7, 3)), 2.0, max_neighbors=-1)
    for bad in (2, 33):
        with pytest.raises(ValueError):
            pc.point_fpfh_radius(np.ones((7, 3)), 2.0, k_normals=bad)
    with pytest.raises(ValueError):
        pc.point_fpfh_radius(np.ones((7, 3)), 2.0, normals=np.ones((6, 3)))
    with pytest.raises(ValueError):
        pc.point_fpfh_radius(np.ones((7, 3)), 2.0, viewpoint=(1.0, 2.0))
