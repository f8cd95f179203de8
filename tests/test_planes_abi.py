"""The plane extraction's C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (a
max_distance that is zero, negative, subnormal, infinite or NaN or whose fp32 square is not a normal number, max_planes, n_trials or
min_inliers out of range, a reference vector that is not finite or zero, its angle out of range, 2^26 rows or more, null pointers,
bad sizes, a short workspace) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE; the
workspace is the one formula the header states."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fit_planes_workspace", "pcreg_dev_model_fit_planes_f32", "pcreg_model_fit_planes_f32", "pcreg_point_fit_planes_f32")


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
    assert "point_fit_planes" in pc.__all__ and hasattr(pc, "point_fit_planes") and hasattr(pc.Model, "fit_planes")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "fit_planes")


def _stated(M, B):
    """planes_ws_layout as include/pcreg.h states it"""
    r256 = lambda b: -(-b // 256) * 256
    R, Cn, T = max(M, 1), max(-(-M // 2048), 1), B
    return 6400 + r256(R) + r256(4 * Cn) + 4 * r256(4 * R) + 2 * r256(12 * T) + r256(T) + r256(8 * T) + r256(4 * T)


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_fit_planes_workspace
    for M in (0, 1, 256, 257, 2048, 2049, 65536, 1000000, (1 << 26) - 1):
        for B in (1, 64, 1000, 1 << 20):
            assert f(M, B) == _stated(M, B), (M, B)
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "6400 + roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + 2 roundup(12 T, 256) + roundup(T, 256) + roundup(8 T, 256) +" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    pl, ce = np.zeros(64 * 4), np.zeros(64 * 3)
    cnt, rm = np.zeros(64, np.int32), np.zeros(64)
    n = C.c_int32(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 24)
    E = _l.PCREG_E_ARG
    outs = (p(lab), p(pl), p(ce), p(cnt), p(rm), C.byref(n), None, None, None)
    ref = np.array([0.0, 0.0, 1.0])

    def all_three(t, rv, ang, P, B, mi):
        r = None if rv is None else p(rv)
        assert L.pcreg_point_fit_planes_f32(p(pts), 8, 8, t, r, ang, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_model_fit_planes_f32(fake, t, r, ang, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_dev_model_fit_planes_f32(fake, t, r, ang, P, B, mi, 0, None, 0, *outs, p(pts), big, None) == E

    for bad in (0.0, -1.0, 1e-40, float("inf"), float("nan"), -float("inf"), 1e-20, 1e20):      # (the last two: the square leaves the normals)
        all_three(bad, None, 0.0, 1, 16, 3)
    assert b"bad argument" in L.pcreg_last_error()
    for P in (0, -1, 65):
        all_three(0.1, None, 0.0, P, 16, 3)
    for B in (0, -1, (1 << 20) + 1):
        all_three(0.1, None, 0.0, 1, B, 3)
    for mi in (2, 0, -1):
        all_three(0.1, None, 0.0, 1, 16, mi)
    for rv in (np.zeros(3), np.array([np.nan, 0, 1.0]), np.array([np.inf, 0, 1.0]), np.array([1e200, 1e200, 0.0])):
        all_three(0.1, rv, 0.5, 1, 16, 3)
    for ang in (0.0, -0.5, 1.5707963267948968, float("nan"), float("inf")):
        all_three(0.1, ref, ang, 1, 16, 3)
    ok = (0.1, None, 0.0, 2, 16, 3, 0, None)
    # ldm < M, a negative M, 2^26 rows, null pointers
    assert L.pcreg_point_fit_planes_f32(p(pts), 8, 7, *ok, *outs) == E
    assert L.pcreg_point_fit_planes_f32(p(pts), -1, 8, *ok, *outs) == E
    assert L.pcreg_point_fit_planes_f32(p(pts), 1 << 26, 1 << 26, *ok, *outs) == E
    assert L.pcreg_point_fit_planes_f32(None, 8, 8, *ok, *outs) == E
    for k in range(6):
        o = list(outs)
        o[k] = None
        assert L.pcreg_point_fit_planes_f32(p(pts), 8, 8, *ok, *o) == E, k
    assert L.pcreg_model_fit_planes_f32(None, *ok, *outs) == E
    o = list(outs)
    o[5] = None
    assert L.pcreg_model_fit_planes_f32(fake, *ok, *o) == E
    assert L.pcreg_dev_model_fit_planes_f32(None, *ok, 0, *outs, p(pts), big, None) == E
    assert L.pcreg_dev_model_fit_planes_f32(fake, *ok, 0, *outs, None, big, None) == E
    assert L.pcreg_dev_model_fit_planes_f32(fake, *ok, 0, *o, p(pts), big, None) == E
    # a workspace one byte short of what the smallest model needs (a given model's own size is checked with the handle in hand)
    short = C.c_size_t(L.pcreg_dev_model_fit_planes_workspace(0, 16) - 1)
    assert L.pcreg_dev_model_fit_planes_f32(fake, *ok, 0, *outs, p(pts), short, None) == E
    assert n.value == -5 and not lab.any() and not pl.any() and not cnt.any()          # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    pl, ce = np.zeros(64 * 4), np.zeros(64 * 3)
    cnt, rm = np.zeros(64, np.int32), np.zeros(64)
    n = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = (p(lab), p(pl), p(ce), p(cnt), p(rm), C.byref(n), None, None, None)
    ref = np.array([0.0, 0.0, -2.0])
    assert L.pcreg_point_fit_planes_f32(p(pts), 8, 9, 0.1, None, 0.0, 64, 1 << 20, 3, 2 ** 64 - 1, None, *outs) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_fit_planes_f32(p(pts), 8, 8, 0.1, p(ref), math.pi / 2, 1, 1, 3, 0, None, *outs) == _l.PCREG_E_NODEVICE
    assert L.pcreg_point_fit_planes_f32(None, 0, 0, 0.1, None, 0.0, 1, 1, 3, 0, None, None, None, None, None, None, C.byref(n), None, None,
                                        None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fit_planes(np.ones((7, 3)), 0.5)
    assert e.value.code == _l.PCREG_E_NODEVICE


def test_point_fit_planes_rejects_bad_arguments():
    import pcreg_amd as pc
    from pcreg_amd.api import planes_args
    pts = np.ones((7, 3))
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        with pytest.raises(ValueError):
            pc.point_fit_planes(pts, bad)
    for kw in (dict(max_planes=0), dict(max_planes=65), dict(n_trials=0), dict(n_trials=(1 << 20) + 1), dict(min_inliers=2),
               dict(ref_vec=[0, 0, 0]), dict(ref_vec=[1, 2]), dict(ref_vec=[1, np.nan, 0]), dict(ref_vec=[0, 0, 1], max_angle=0.0),
               dict(ref_vec=[0, 0, 1], max_angle=2.0), dict(samples=np.zeros((1, 5, 3), np.int32), n_trials=4)):
        with pytest.raises(ValueError):
            pc.point_fit_planes(pts, 0.5, **kw)
    for shape in ((7, 2), (7, 4), (7,), (2, 7, 3)):
        with pytest.raises(ValueError):
            pc.point_fit_planes(np.ones(shape), 0.5)
    t, rv, ang, P, B, mi, sd = planes_args(0.1, [0, 0, 2], 0.25, 3, 100, 5, -1)
    assert t == float(np.float32(0.1)) and list(rv) == [0.0, 0.0, 2.0] and (ang, P, B, mi) == (0.25, 3, 100, 5) and sd == 2 ** 64 - 1
