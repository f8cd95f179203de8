"""The cylinder extraction's MEX commands and MATLAB wrappers.  Without a GPU: 'modelFitCylinders' and 'pointFitCylinders' of
mex/pcreg_mex.cpp (tests/mexfitcylinders/fit_cylinders_driver.cpp on tests/mexstub/mex.h) refuse bad usage through
mexErrMsgIdAndTxt and leak no array; matlab/fitCylindersModel.m, matlab/fitCylindersFast.m and matlab/pcfitcylinderFast.m call them
the way the gateway checks.  With one: the round trip equals the ctypes path bit for bit, with the cylinders as n x 7 columns and
1-based winning trials."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cylinders_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# maxDistance, minRadius, maxRadius (singles), refVec ([]), maxAngle, normals ([]), kNormals, maxCylinders, nTrials, minInliers, seed
GOOD_KINDS, GOOD_VALS = (2, 2, 2, 4, 0, 4, 0, 0, 0, 0, 0), (0.5, 0.0, math.inf, 0.0, 0.0, 0.0, 12.0, 2.0, 16.0, 4.0, 7.0)


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexfitcylinders") / "libmexfitcylinders.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexfitcylinders", "fit_cylinders_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.ds_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.ds_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_double, C.c_void_p, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


def _usage(drv, via_handle, nargs=13, first_kind=0, kinds=GOOD_KINDS, vals=GOOD_VALS, samples_kind=0, samples_cols=32):
    e = _err()
    rc = drv.ds_usage(via_handle, nargs, first_kind, (C.c_int * 11)(*kinds), (C.c_double * 11)(*vals), samples_kind, samples_cols, e, 1024)
    return rc, e.value.decode()


def _with(i, kind=None, val=None, **more):
    kinds, vals = list(GOOD_KINDS), list(GOOD_VALS)
    if kind is not None:
        kinds[i] = kind
    if val is not None:
        vals[i] = val
    for j, v in more.items():
        if j.startswith("k"):
            kinds[int(j[1:])] = v
        else:
            vals[int(j[1:])] = v
    return dict(kinds=kinds, vals=vals)


BAD = ([_with(i, kind=k) for i in (0, 1, 2) for k in (0, 5)]                                          # a double or a 1 x 2 where a single scalar goes
       + [_with(0, val=v) for v in (0.0, -4.0, 1e-40, float("inf"), float("nan"))]
       + [_with(1, val=v) for v in (-1.0, float("nan"))]
       + [_with(2, val=v) for v in (float("nan"), -1.0)] + [_with(1, val=3.0, v2=2.0)]                 # maxRadius below minRadius
       + [_with(3, kind=k, val=1.0, v4=0.5) for k in (0, 3, 2)]                                        # refVec: a scalar, 1 x 2, a single
       + [_with(3, kind=6, val=v, v4=0.5) for v in (0.0, float("nan"), float("inf"))]                  # zero or not finite
       + [_with(3, kind=6, val=1.0, v4=v) for v in (0.0, -0.5, 1.6, float("nan"))]                     # maxAngle outside (0, pi / 2] with refVec
       + [_with(4, kind=k) for k in (2, 3, 4)]                                                         # maxAngle: a single, 1 x 2, empty
       + [_with(5, kind=k, val=1.0) for k in (9, 2)]                                                   # normals: double 4 x 3, a single scalar
       + [_with(i, kind=k) for i in (6, 7, 8, 9, 10) for k in (2, 3)]                                  # a single or 1 x 2 scalar
       + [_with(6, val=v) for v in (2.0, 33.0, 3.5)]
       + [_with(7, val=v) for v in (0.0, 65.0, 1.5, float("nan"))]
       + [_with(8, val=v) for v in (0.0, 1048577.0, 2.5)]
       + [_with(9, val=v) for v in (3.0, -1.0, 4.5)]
       + [_with(10, val=v) for v in (-1.0, 0.5, float("inf"))]
       + [dict(samples_kind=2), dict(samples_kind=3), dict(samples_kind=1, samples_cols=31)])         # double samples; three rows; not nTrials * maxCylinders columns


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("kw", BAD)
def test_usage_errors(drv, via_handle, kw):
    rc, msg = _usage(drv, via_handle, **kw)
    cmd = "modelFitCylinders" if via_handle else "pointFitCylinders"
    assert rc == 1 and msg.startswith(f"pcreg:usage: {cmd}:"), msg
    assert drv.ds_live_arrays() == 0


def test_point_fit_cylinders_refuses_normals_of_other_rows(drv):
    rc, msg = _usage(drv, 0, **_with(5, kind=8, val=1.0))                   # single 3 x 3 normals for a 4 x 3 cloud
    assert rc == 1 and msg.startswith("pcreg:usage: pointFitCylinders:"), msg
    assert drv.ds_live_arrays() == 0


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs", [12, 14])
def test_a_missing_or_surplus_argument(drv, via_handle, nargs):
    rc, msg = _usage(drv, via_handle, nargs=nargs)
    assert rc == 1 and msg.startswith("pcreg:usage: " + ("modelFitCylinders" if via_handle else "pointFitCylinders") + ":"), msg
    assert drv.ds_live_arrays() == 0


@pytest.mark.parametrize("first_kind", [1, 2])
def test_point_fit_cylinders_refuses_a_double_or_two_column_cloud(drv, first_kind):
    rc, msg = _usage(drv, 0, first_kind=first_kind)
    assert rc == 1 and msg.startswith("pcreg:usage: pointFitCylinders:"), msg
    assert drv.ds_live_arrays() == 0


def test_null_handle_is_a_library_error(drv):
    rc, msg = _usage(drv, 1, samples_kind=1)
    assert rc == 1 and msg.startswith("pcreg:hip: bad argument"), msg
    assert drv.ds_live_arrays() == 0


def _round_trip(drv, via_handle, m, nrm, t, rmin, rmax, rv, ang, kn, P, B, mi, seed, samples, nlhs):
    M = len(m)
    lab = np.full(max(M, 1), -7, np.int32)
    cy, ex = np.full((P, 7), -7.0), np.full((P, 2), -7.0)
    cnt, rm, used, dg = np.full(P, -7, np.int32), np.full(P, -7.0), np.full(P, -7, np.int32), np.full((P, 3), -7.0)
    e = _err(); n_out = C.c_int(-1); n_cy = C.c_int(-1)
    mf = np.asfortranarray(m) if M else np.zeros((1, 3), np.float32, order="F")
    nf = None if nrm is None else np.asfortranarray(np.asarray(nrm, np.float32))
    ref_v = None if rv is None else np.ascontiguousarray(rv, np.float64)
    smp = None if samples is None else np.ascontiguousarray(samples, np.int32)            # [P][B][2] row-major = 2 x (B P) column-major
    rc = drv.ds_round_trip(via_handle, mf.ctypes.data, M, t, rmin, rmax, None if ref_v is None else ref_v.ctypes.data, ang,
                           None if nf is None else nf.ctypes.data, kn, P, B, mi, float(seed), None if smp is None else smp.ctypes.data, nlhs,
                           lab.ctypes.data, cy.ctypes.data, ex.ctypes.data, cnt.ctypes.data, rm.ctypes.data, used.ctypes.data, dg.ctypes.data,
                           C.byref(n_cy), C.byref(n_out), e, 1024)
    n = max(n_cy.value, 0)
    return rc, e.value.decode(), n_out.value, n, lab[:M], cy[:n], ex[:n], cnt[:n], rm[:n], used[:n], dg


@pytest.mark.parametrize("via_handle", [0, 1])
def test_reports_nodevice_through_mexerr(drv, via_handle):
    _no_gpu()
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    rc, msg, *_ = _round_trip(drv, via_handle, m, m, 0.1, 0.0, math.inf, None, 0.0, 12, 2, 16, 4, 1, None, 7)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.ds_live_arrays() == 0


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("case", ["scene", "radius", "ref", "computed", "samples", "M2", "M0"])
def test_round_trip_equals_the_host_tier(drv, via_handle, case):
    """[labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('modelFitCylinders', h, ...) / ('pointFitCylinders',
    single(pts), ...) with one to seven outputs: the bits of Model.fit_cylinders, the winning trials 1-based"""
    import pcreg_amd as pc
    M, B, mi = ref.SCENES[0]
    m, nrm, _ = ref.scene(M)
    kw = dict(max_radius=ref.SCENE_RMAX, max_cylinders=5, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED)
    t = ref.SCENE_T
    if case == "radius":
        kw.update(min_radius=1.0, max_radius=2.0, max_cylinders=2)
    elif case == "ref":
        kw.update(ref_vec=ref.SCENE_CYLINDERS[1][1], max_angle=0.3, max_cylinders=2)
    elif case == "computed":
        nrm = None
        kw.update(k_normals=10, max_cylinders=2)
    elif case == "samples":
        rng = np.random.default_rng(3)
        kw.update(max_cylinders=2, n_trials=64, samples=rng.integers(0, len(m) + 2, (2, 64, 2)).astype(np.int32))
    elif case in ("M2", "M0"):
        m = (np.array([[0, 0, 0], [1, 1, 0]], np.float32) + 5)[:int(case[1])]
        nrm = np.array([[1, 0, 0], [0, 1, 0]], np.float32)[:int(case[1])]
        kw = dict(max_cylinders=2, n_trials=32, min_inliers=4, seed=2)
        t = 0.1
    with pc.Model(m) as h:
        want = h.fit_cylinders(t, normals=nrm, **kw)
    n = want["n_cylinders"]
    P = kw["max_cylinders"]
    for nlhs in (1, 2, 3, 4, 5, 6, 7):
        rc, msg, n_out, n_cy, lab, cy, ex, cnt, rm, used, dg = _round_trip(
            drv, via_handle, m, nrm, t, kw.get("min_radius", 0.0), kw.get("max_radius", math.inf), kw.get("ref_vec"), kw.get("max_angle", 0.0),
            kw.get("k_normals", 12), P, kw["n_trials"], kw["min_inliers"], kw.get("seed", 0), kw.get("samples"), nlhs)
        assert rc == 0, msg
        assert n_out == nlhs and drv.ds_live_arrays() == 0
        assert np.array_equal(lab, want["labels"])
        if nlhs > 1:
            assert n_cy == n and np.array_equal(_b64(cy), _b64(want["cylinders"][:n]))
        if nlhs > 2:
            assert np.array_equal(_b64(ex), _b64(want["extents"][:n]))
        if nlhs > 3:
            assert np.array_equal(cnt, want["counts"][:n])
        if nlhs > 4:
            assert np.array_equal(_b64(rm), _b64(want["rmse"][:n]))
        if nlhs > 5:
            assert np.array_equal(used, want["refit_used"][:n])
        if nlhs > 6:
            ran = min(n + 1, P) if len(m) else 0
            assert np.array_equal(dg[:ran, 0], want["best_trial"][:ran] + 1.0) and not dg[ran:].any()
            assert np.array_equal(dg[:, 1], want["best_cost"].astype(np.float64)) and np.array_equal(dg[:, 2], want["best_count"])
    if case == "scene":
        assert n == 2
    if case in ("radius", "ref", "computed"):
        assert n >= 1
    if case in ("M2", "M0"):
        assert n == 0


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    args = "t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp"
    for wrapper, cmd, first in (("fitCylindersModel", "modelFitCylinders", "h"), ("fitCylindersFast", "pointFitCylinders", "single(pts)")):
        src = open(os.path.join(ROOT, "matlab", wrapper + ".m")).read()
        assert f"labels = pcreg_mex('{cmd}', {first}, {args});" in src                                           # 14 arguments
        assert f"[labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('{cmd}', {first}, {args});" in src
        # maxDistance and the radius bounds as singles; the angle from degrees to radians; single normals; int32 samples
        assert "t = single(maxDistance);" in src and "rmin = single(p.Results.MinRadius);" in src
        assert "rmax = single(p.Results.MaxRadius);" in src and "smp = int32(p.Results.Samples);" in src
        assert "ang = double(p.Results.MaxAngularDistance) * pi / 180;" in src and "nrm = single(p.Results.Normals);" in src
        assert "rv = double(p.Results.ReferenceVector(:)');" in src and "kn = double(p.Results.NumNeighborsNormals);" in src
        for name in ("'Normals', []", "'NumNeighborsNormals', 12", "'ReferenceVector', []", "'MaxAngularDistance', 5", "'MaxNumCylinders', 1",
                     "'MaxNumTrials', 1000", "'MinInliers', 4", "'MinRadius', 0", "'MaxRadius', Inf", "'Seed', 0", "'Samples', []"):
            assert f"addParameter(p, {name}" in src, name
        block = gw.split(f'strcmp(cmd, "{cmd}")')[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 14\b", block) and "fit_cylinders_on_handle(" in block
        assert f"'{cmd}'" in head and wrapper + ".m" in head
    one = open(os.path.join(ROOT, "matlab", "pcfitcylinderFast.m")).read()
    assert one.startswith("function [model, inlierIndices, outlierIndices, rmse] = pcfitcylinderFast(pts, maxDistance, varargin)")
    assert "fitCylindersFast(pts, maxDistance, 'MaxNumCylinders', 1, args{:})" in one and "pcfitcylinderFast.m" in head
    assert "model = [c + extents(1, 1) * w, c + extents(1, 2) * w, cylinders(1, 7)];" in one                    # [x1 y1 z1 x2 y2 z2 r]
    assert "inlierIndices = uint32(find(labels == 1));" in one and "outlierIndices = uint32(find(labels ~= 1));" in one
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fitCylindersModel" in integ and "pcreg_model_fit_cylinders_f32" in integ and "pcfitcylinder" in integ
