"""The cylinder extraction's C ABI without a GPU: the four entry points are exported, declared and listed; argument errors (a
max_distance that is zero, negative, subnormal, infinite or NaN or whose fp32 square is not a normal number, radius bounds that are
negative, NaN or out of order, a reference vector that is not finite or zero, a max_angle outside (0, pi / 2] with one, max_cylinders,
n_trials, min_inliers or k_normals out of range, 2^26 rows or more, null pointers, bad sizes, a short workspace) are PCREG_E_ARG
before anything runs; a valid call without a device is PCREG_E_NODEVICE; the workspace is the one formula the header states."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fit_cylinders_workspace", "pcreg_dev_model_fit_cylinders_f32", "pcreg_model_fit_cylinders_f32",
       "pcreg_point_fit_cylinders_f32")
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
    assert "point_fit_cylinders" in pc.__all__ and hasattr(pc, "point_fit_cylinders") and hasattr(pc.Model, "fit_cylinders")
    from pcreg_amd.device import PreparedModel
    assert hasattr(PreparedModel, "fit_cylinders")


def test_prototypes_match_the_header():
    """the ctypes argument lists have the header's number of parameters, floats where the header has floats, doubles where it has
    doubles"""
    _l, L = _lib()
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    for name in NEW[1:]:
        decl = head.split("int " + name + "(")[1].split(");")[0]
        while "/*" in decl:                            # (the comments of a parameter hold no comma, but words)
            decl = decl[:decl.index("/*")] + decl[decl.index("*/") + 2:]
        params = [" ".join(p.split()) for p in decl.replace("\n", " ").split(",")]
        at = getattr(L, name).argtypes
        assert len(at) == len(params), name
        for a, p in zip(at, params):
            if p.startswith("float "):
                assert a is C.c_float, (name, p)
            elif p.startswith("double "):
                assert a is C.c_double, (name, p)
            elif p.startswith("uint64_t "):
                assert a is C.c_uint64, (name, p)
            elif "*" in p:
                assert a is C.c_void_p, (name, p)
            elif p.startswith("size_t "):
                assert a is C.c_size_t, (name, p)
            else:
                assert a is C.c_int, (name, p)
    assert L.pcreg_dev_model_fit_cylinders_workspace.restype is C.c_size_t


def _stated(M, B):
    """fit_cylinders_ws_layout as include/pcreg.h states it"""
    r256 = lambda b: -(-b // 256) * 256
    R, Cn, T = max(M, 1), max(-(-M // 2048), 1), B
    return 11008 + 2 * r256(R) + r256(4 * Cn) + 4 * r256(4 * R) + r256(12 * T) + r256(28 * T) + r256(T) + r256(8 * T) + r256(4 * T)


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_fit_cylinders_workspace
    for M in (0, 1, 256, 257, 2048, 2049, 65536, 1000000, (1 << 26) - 1):
        for B in (1, 64, 1000, 1 << 20):
            assert f(M, B) == _stated(M, B), (M, B)
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "11008 + 2 roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + roundup(12 T, 256) + roundup(28 T, 256) + roundup(T, 256) +" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    cy, ex = np.zeros(64 * 7), np.zeros(64 * 2)
    cnt, rm, used = np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32)
    n = C.c_int32(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 24)
    E = _l.PCREG_E_ARG
    outs = (p(lab), p(cy), p(ex), p(cnt), p(rm), p(used), C.byref(n), None, None, None)
    rv = (C.c_double * 3)(0.0, 0.0, 1.0)

    def all_three(t, r0, r1, ref, ang, P, B, mi):
        assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 8, t, r0, r1, ref, ang, p(nrm), 8, 12, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_model_fit_cylinders_f32(fake, t, r0, r1, ref, ang, p(nrm), 8, 12, P, B, mi, 0, None, *outs) == E
        assert L.pcreg_dev_model_fit_cylinders_f32(fake, t, r0, r1, ref, ang, fake, 8, P, B, mi, 0, None, 0, *outs, p(pts), big, None) == E

    for bad in (0.0, -1.0, 1e-40, INF, float("nan"), -INF, 1e-20, 1e20):      # (the last two: the square leaves the normals)
        all_three(bad, 0.0, INF, None, 0.0, 1, 16, 4)
    assert b"bad argument" in L.pcreg_last_error()
    for r0, r1 in ((-1.0, 5.0), (-0.5, INF), (float("nan"), 5.0), (0.0, float("nan")), (3.0, 2.0), (INF, 5.0), (0.0, -INF)):
        all_three(0.1, r0, r1, None, 0.0, 1, 16, 4)
    for ang in (0.0, -0.1, 1.6, float("nan"), INF):                            # max_angle is read with a reference vector alone
        all_three(0.1, 0.0, INF, rv, ang, 1, 16, 4)
    for bad in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (INF, 0.0, 1.0), (1e200, 1e200, 1e200)):
        all_three(0.1, 0.0, INF, (C.c_double * 3)(*bad), 0.5, 1, 16, 4)
    for P in (0, -1, 65):
        all_three(0.1, 0.0, INF, None, 0.0, P, 16, 4)
    for B in (0, -1, (1 << 20) + 1):
        all_three(0.1, 0.0, INF, None, 0.0, 1, B, 4)
    for mi in (3, 0, -1):
        all_three(0.1, 0.0, INF, None, 0.0, 1, 16, mi)
    geo = (0.1, 0.0, INF, None, 0.0)
    ok = (2, 16, 4, 0, None)
    # ldm < M, a negative M, 2^26 rows, null pointers, ldn < M, k_normals out of range without normals
    assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 7, *geo, p(nrm), 8, 12, *ok, *outs) == E
    assert L.pcreg_point_fit_cylinders_f32(p(pts), -1, 8, *geo, p(nrm), 8, 12, *ok, *outs) == E
    assert L.pcreg_point_fit_cylinders_f32(p(pts), 1 << 26, 1 << 26, *geo, p(nrm), 1 << 26, 12, *ok, *outs) == E
    assert L.pcreg_point_fit_cylinders_f32(None, 8, 8, *geo, p(nrm), 8, 12, *ok, *outs) == E
    assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 8, *geo, p(nrm), 7, 12, *ok, *outs) == E
    for kn in (2, 33, 0, -1):
        assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 8, *geo, None, 8, kn, *ok, *outs) == E, kn
        assert L.pcreg_model_fit_cylinders_f32(fake, *geo, None, 8, kn, *ok, *outs) == E, kn
    for k in range(7):
        o = list(outs)
        o[k] = None
        assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 8, *geo, p(nrm), 8, 12, *ok, *o) == E, k
    assert L.pcreg_model_fit_cylinders_f32(None, *geo, p(nrm), 8, 12, *ok, *outs) == E
    o = list(outs)
    o[6] = None
    assert L.pcreg_model_fit_cylinders_f32(fake, *geo, p(nrm), 8, 12, *ok, *o) == E
    assert L.pcreg_dev_model_fit_cylinders_f32(None, *geo, fake, 8, *ok, 0, *outs, p(pts), big, None) == E
    assert L.pcreg_dev_model_fit_cylinders_f32(fake, *geo, fake, 8, *ok, 0, *outs, None, big, None) == E
    assert L.pcreg_dev_model_fit_cylinders_f32(fake, *geo, fake, 8, *ok, 0, *o, p(pts), big, None) == E
    # a workspace one byte short of what the smallest model needs (a given model's own size is checked with the handle in hand)
    short = C.c_size_t(L.pcreg_dev_model_fit_cylinders_workspace(0, 16) - 1)
    assert L.pcreg_dev_model_fit_cylinders_f32(fake, *geo, fake, 8, *ok, 0, *outs, p(pts), short, None) == E
    assert n.value == -5 and not lab.any() and not cy.any() and not ex.any() and not cnt.any() and not used.any()      # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    nrm = np.zeros(64 * 3, np.float32)
    lab = np.zeros(64, np.int32)
    cy, ex = np.zeros(64 * 7), np.zeros(64 * 2)
    cnt, rm, used = np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32)
    n = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = (p(lab), p(cy), p(ex), p(cnt), p(rm), p(used), C.byref(n), None, None, None)
    rv = (C.c_double * 3)(0.0, 0.0, 2.0)
    N = _l.PCREG_E_NODEVICE
    assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 9, 0.1, 0.0, INF, None, 99.0, p(nrm), 9, 0, 64, 1 << 20, 4, 2 ** 64 - 1, None, *outs) == N
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_point_fit_cylinders_f32(p(pts), 8, 8, 0.1, 2.0, 2.0, rv, math.pi / 2, None, 0, 3, 1, 1, 4, 0, None, *outs) == N
    assert L.pcreg_point_fit_cylinders_f32(None, 0, 0, 0.1, 0.0, INF, None, 0.0, None, 0, 32, 1, 1, 4, 0, None, None, None, None, None, None,
                                           None, C.byref(n), None, None, None) == N
    with pytest.raises(PcregError) as e:
        pc.point_fit_cylinders(np.ones((7, 3)), 0.5)
    assert e.value.code == N


def test_point_fit_cylinders_rejects_bad_arguments():
    import pcreg_amd as pc
    from pcreg_amd.api import fit_cylinders_args
    pts = np.ones((7, 3))
    for bad in (0.0, -1.0, float("nan"), INF, 1e-30, 1e30):
        with pytest.raises(ValueError):
            pc.point_fit_cylinders(pts, bad)
    for kw in (dict(max_cylinders=0), dict(max_cylinders=65), dict(n_trials=0), dict(n_trials=(1 << 20) + 1), dict(min_inliers=3),
               dict(min_radius=-1.0), dict(min_radius=float("nan")), dict(max_radius=float("nan")), dict(min_radius=3.0, max_radius=2.0),
               dict(ref_vec=(0, 0, 0)), dict(ref_vec=(0, 0, 1), max_angle=0.0), dict(ref_vec=(0, 0, 1), max_angle=2.0),
               dict(ref_vec=(0, 1)), dict(k_normals=2), dict(k_normals=33), dict(normals=np.ones((6, 3))), dict(normals=np.ones((7, 2))),
               dict(samples=np.zeros((1, 4, 3), np.int32), n_trials=4), dict(samples=np.zeros((1, 5, 2), np.int32), n_trials=4)):
        with pytest.raises(ValueError):
            pc.point_fit_cylinders(pts, 0.5, **kw)
    for shape in ((7, 2), (7, 4), (7,), (2, 7, 3)):
        with pytest.raises(ValueError):
            pc.point_fit_cylinders(np.ones(shape), 0.5)
    t, r0, r1, rv, ang, P, B, mi, sd = fit_cylinders_args(0.1, 0.3, math.inf, (0, 0, 2), 0.25, 3, 100, 5, -1)
    assert t == float(np.float32(0.1)) and r0 == float(np.float32(0.3)) and r1 == math.inf and (P, B, mi) == (3, 100, 5) and sd == 2 ** 64 - 1
    assert rv.tolist() == [0.0, 0.0, 2.0] and ang == 0.25
    assert fit_cylinders_args(0.1, 0.0, 1.0, None, 99.0, 1, 1, 4, 0)[3:5] == (None, 0.0)
