"""The sphere extraction's C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (a
max_distance that is zero, negative, subnormal, infinite or NaN or whose fp32 square is not a normal number, radius bounds that are
negative, NaN or out of order, max_spheres, n_trials or min_inliers out of range, 2^26 rows or more, null pointers, bad sizes, a
short workspace) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE; the workspace is the one
formula the header states."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fit_spheres_workspace", "pcreg_dev_model_fit_spheres_f32", "pcreg_model_fit_spheres_f32", "pcreg_point_fit_spheres_f32")
INF = float("inf")


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
    assert "point_fit_spheres" in pc.__all__ and hasattr(pc, "point_fit_spheres") and hasattr(pc.Model, "fit_spheres")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "fit_spheres")


def test_prototypes_match_the_header():
    """the ctypes argument lists have the header's number of parameters, floats where the header has floats"""
    _l, L = _lib()
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    for name in NEW[1:]:
        decl = head.split("int " + name + "(")[1].split(");")[0]
        params = [p for p in decl.replace("\n", " ").split(",")]
        at = getattr(L, name).argtypes
        assert len(at) == len(params), name
        for a, p in zip(at, params):
            p = " ".join(w for w in p.split() if not w.startswith("/*") and not w.endswith("*/"))
            if p.startswith("float "):
                assert a is C.c_float, (name, p)
            elif p.startswith("uint64_t "):
                assert a is C.c_uint64, (name, p)
            elif "*" in p:
                assert a is C.c_void_p, (name, p)
            elif p.startswith("size_t "):
                assert a is C.c_size_t, (name, p)
            else:
                assert a is C.c_int, (name, p)
    assert L.pcreg_dev_model_fit_spheres_workspace.restype is C.c_size_t


def _stated(M, B):
    """fit_spheres_ws_layout as include/pcreg.h states it"""
    r256 = lambda b: -(-b // 256) * 256
    R, Cn, T = max(M, 1), max(-(-M // 2048), 1), B
    return 9984 + r256(R) + r256(4 * Cn) + 4 * r256(4 * R) + r256(12 * T) + r256(16 * T) + r256(T) + r256(8 * T) + r256(4 * T)


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_fit_spheres_workspace
    for M in (0, 1, 256, 257, 2048, 2049, 65536, 1000000, (1 << 26) - 1):
        for B in (1, 64, 1000, 1 << 20):
            assert f(M, B) == _stated(M, B), (M, B)
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "9984 + roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + roundup(12 T, 256) + roundup(16 T, 256) + roundup(T, 256) +" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    sp = np.zeros(64 * 4)
    cnt, rm, used = np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32)
    n = C.c_int32(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 24)
    E = _l.PCREG_E_ARG
    outs = (p(lab), p(sp), p(cnt), p(rm), p(used), C.byref(n), None, None, None)

    def all_three(t, r0, r1, P, B, mi):
        assert L.pcreg_point_fit_spheres_f32(p(pts), 8, 8, t, r0, r1, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_model_fit_spheres_f32(fake, t, r0, r1, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_dev_model_fit_spheres_f32(fake, t, r0, r1, P, B, mi, 0, None, 0, *outs, p(pts), big, None) == E

    for bad in (0.0, -1.0, 1e-40, INF, float("nan"), -INF, 1e-20, 1e20):      # (the last two: the square leaves the normals)
        all_three(bad, 0.0, INF, 1, 16, 4)
    assert b"bad argument" in L.pcreg_last_error()
    for r0, r1 in ((-1.0, 5.0), (-0.5, INF), (float("nan"), 5.0), (0.0, float("nan")), (3.0, 2.0), (INF, 5.0), (0.0, -INF)):
        all_three(0.1, r0, r1, 1, 16, 4)
    for P in (0, -1, 65):
        all_three(0.1, 0.0, INF, P, 16, 4)
    for B in (0, -1, (1 << 20) + 1):
        all_three(0.1, 0.0, INF, 1, B, 4)
    for mi in (3, 0, -1):
        all_three(0.1, 0.0, INF, 1, 16, mi)
    ok = (0.1, 0.0, INF, 2, 16, 4, 0, None)
    # ldm < M, a negative M, 2^26 rows, null pointers
    assert L.pcreg_point_fit_spheres_f32(p(pts), 8, 7, *ok, *outs) == E
    assert L.pcreg_point_fit_spheres_f32(p(pts), -1, 8, *ok, *outs) == E
    assert L.pcreg_point_fit_spheres_f32(p(pts), 1 << 26, 1 << 26, *ok, *outs) == E
    assert L.pcreg_point_fit_spheres_f32(None, 8, 8, *ok, *outs) == E
    for k in range(6):
        o = list(outs)
        o[k] = None
        assert L.pcreg_point_fit_spheres_f32(p(pts), 8, 8, *ok, *o) == E, k
    assert L.pcreg_model_fit_spheres_f32(None, *ok, *outs) == E
    o = list(outs)
    o[5] = None
    assert L.pcreg_model_fit_spheres_f32(fake, *ok, *o) == E
    assert L.pcreg_dev_model_fit_spheres_f32(None, *ok, 0, *outs, p(pts), big, None) == E
    assert L.pcreg_dev_model_fit_spheres_f32(fake, *ok, 0, *outs, None, big, None) == E
    assert L.pcreg_dev_model_fit_spheres_f32(fake, *ok, 0, *o, p(pts), big, None) == E
    # a workspace one byte short of what the smallest model needs (a given model's own size is checked with the handle in hand)
    short = C.c_size_t(L.pcreg_dev_model_fit_spheres_workspace(0, 16) - 1)
    assert L.pcreg_dev_model_fit_spheres_f32(fake, *ok, 0, *outs, p(pts), short, None) == E
    assert n.value == -5 and not lab.any() and not sp.any() and not cnt.any() and not used.any()          # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    sp = np.zeros(64 * 4)
    cnt, rm, used = np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32)
    n = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = (p(lab), p(sp), p(cnt), p(rm), p(used), C.byref(n), None, None, None)
    assert L.pcreg_point_fit_spheres_f32(p(pts), 8, 9, 0.1, 0.0, INF, 64, 1 << 20, 4, 2 ** 64 - 1, None, *outs) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_fit_spheres_f32(p(pts), 8, 8, 0.1, 2.0, 2.0, 1, 1, 4, 0, None, *outs) == _l.PCREG_E_NODEVICE
    assert L.pcreg_point_fit_spheres_f32(None, 0, 0, 0.1, 0.0, INF, 1, 1, 4, 0, None, None, None, None, None, None, C.byref(n), None, None,
                                         None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.point_fit_spheres(np.ones((7, 3)), 0.5)
    assert e.value.code == _l.PCREG_E_NODEVICE


def test_point_fit_spheres_rejects_bad_arguments():
    import pcreg_amd as pc
    from pcreg_amd.api import fit_spheres_args
    pts = np.ones((7, 3))
    for bad in (0.0, -1.0, float("nan"), INF, 1e-30, 1e30):
        with pytest.raises(ValueError):
            pc.point_fit_spheres(pts, bad)
    for kw in (dict(max_spheres=0), dict(max_spheres=65), dict(n_trials=0), dict(n_trials=(1 << 20) + 1), dict(min_inliers=3),
               dict(min_radius=-1.0), dict(min_radius=float("nan")), dict(max_radius=float("nan")), dict(min_radius=3.0, max_radius=2.0),
               dict(samples=np.zeros((1, 4, 3), np.int32), n_trials=4), dict(samples=np.zeros((1, 5, 4), np.int32), n_trials=4)):
        with pytest.raises(ValueError):
            pc.point_fit_spheres(pts, 0.5, **kw)
    for shape in ((7, 2), (7, 4), (7,), (2, 7, 3)):
        with pytest.raises(ValueError):
            pc.point_fit_spheres(np.ones(shape), 0.5)
    t, r0, r1, P, B, mi, sd = fit_spheres_args(0.1, 0.3, math.inf, 3, 100, 5, -1)
    assert t == float(np.float32(0.1)) and r0 == float(np.float32(0.3)) and r1 == math.inf and (P, B, mi) == (3, 100, 5) and sd == 2 ** 64 - 1
