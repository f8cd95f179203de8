"""Fast global registration's MEX command and MATLAB wrappers.  Without a GPU: 'fgrBatched' of mex/pcreg_mex.cpp
(tests/mexfgr/fgr_driver.cpp on tests/mexstub/mex.h) refuses bad usage through mexErrMsgIdAndTxt, hands the library's argument
rules on and leaks no array; matlab/fgrBatched.m and matlab/pcregisterfgrFast.m call the gateway the way it checks.  With one:
the round trip equals the ctypes path (pcreg_amd.fgr_batched) bit for bit, with one to four outputs, with and without a triple
table and a start."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fgr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
KEYS = ("delta2", "iterations", "decrease_every", "division_factor", "mu0", "n_tuples", "tuple_scale", "seed")


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexfgr") / "libmexfgr.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexfgr", "fgr_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.fd_usage.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    L.fd_round_trip.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


def _o(**kw):
    """the driver's eight option slots: a NaN leaves the field out of the struct"""
    o = dict(delta2=1.0)
    o.update(kw)
    return np.array([o.get(k, NAN) for k in KEYS], np.float64)


@pytest.mark.parametrize("nargs, kind, o", [
    (3, 0, _o()), (7, 0, _o()), (4, 1, _o()), (4, 2, _o()), (4, 3, _o()), (4, 4, _o()), (4, 5, _o()), (4, 9, _o()), (4, 0, _o(delta2=NAN)),
    (5, 6, _o(n_tuples=4)), (5, 7, _o(n_tuples=4)), (6, 8, _o())])
def test_usage_errors(drv, nargs, kind, o):
    """a missing or surplus argument; single points, double offsets, opts no struct, offsets short of the rows, a two-column cloud, pts2
    with fewer rows, no delta2; a triple table of the wrong size or class; a T0 of the wrong size"""
    e = _err()
    assert drv.fd_usage(nargs, kind, o.ctypes.data, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: fgrBatched:"), e.value
    assert drv.fd_live_arrays() == 0


@pytest.mark.parametrize("kw", [dict(delta2=-1.0), dict(iterations=0), dict(decrease_every=0), dict(division_factor=1.0), dict(mu0=-1.0),
                                dict(n_tuples=-1), dict(tuple_scale=0.0), dict(tuple_scale=1.5)])
def test_the_librarys_argument_rules_come_through(drv, kw):
    e = _err()
    assert drv.fd_usage(4, 0, _o(**kw).ctypes.data, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.fd_live_arrays() == 0


def _round_trip(drv, p1s, p2s, o, nlhs, table=None, T0=None):
    sizes = [len(p) for p in p1s]
    B, total = len(sizes), int(sum(sizes))
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    a1 = np.asfortranarray(np.concatenate(p1s).reshape(-1, 3)) if total else np.zeros((1, 3), order="F")
    a2 = np.asfortranarray(np.concatenate(p2s).reshape(-1, 3)) if total else np.zeros((1, 3), order="F")
    tb = None if table is None else np.ascontiguousarray(table, np.int32)                   # [B][n_tuples][3] = 3 x (n_tuples B) column-major
    t0 = None if T0 is None else np.ascontiguousarray(np.asarray(T0, np.float64).transpose(0, 2, 1))
    T, inl, stats, kept = np.full(16 * max(B, 1), -7.0), np.full(max(total, 1), -7.0), np.full(9 * max(B, 1), -7.0), np.full(max(total, 1), 9, np.uint8)
    e, n_inl = _err(), C.c_int(-2)
    rc = drv.fd_round_trip(a1.ctypes.data, a2.ctypes.data, total, off.ctypes.data, B, o.ctypes.data, None if tb is None else tb.ctypes.data,
                           None if t0 is None else t0.ctypes.data, nlhs, T.ctypes.data, inl.ctypes.data, C.byref(n_inl), stats.ctypes.data,
                           kept.ctypes.data, e, 1024)
    return rc, e.value.decode(), T.reshape(max(B, 1), 4, 4).transpose(0, 2, 1), inl[:max(n_inl.value, 0)], n_inl.value, stats.reshape(9, max(B, 1)).T, kept[:total], off


def test_reports_nodevice_through_mexerr(drv):
    _no_gpu()
    sc = fgr_ref.scenes()[0]
    rc, msg, *_ = _round_trip(drv, [sc["p1"]], [sc["p2"]], _o(), 4)
    assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg
    assert drv.fd_live_arrays() == 0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "tuples", "table and T0"])
def test_round_trip_equals_the_ctypes_path(drv, case):
    """[T, inlierIdx, stats, kept] = pcreg_mex('fgrBatched', ...) with one to four outputs: the bits of pcreg_amd.fgr_batched"""
    import pcreg_amd as pc
    scs = fgr_ref.scenes()
    p1s = [scs[0]["p1"], scs[0]["p1"][:2], np.zeros((0, 3)), scs[1]["p1"]]              # (a failed and an empty registration among them)
    p2s = [scs[0]["p2"], scs[0]["p2"][:2], np.zeros((0, 3)), scs[1]["p2"]]
    opts, table, T0 = dict(delta2=1.0), None, None
    if case == "tuples":
        opts = dict(delta2=1.0, n_tuples=900, seed=5, tuple_scale=0.9, iterations=40, decrease_every=2, division_factor=1.5, mu0=5000.0)
    if case == "table and T0":
        rng = np.random.default_rng(3)
        opts = dict(delta2=1.0, n_tuples=600, iterations=24, decrease_every=2)
        table = rng.integers(-5, 520, (4, 600, 3))
        T0 = np.stack([scs[0]["T"], np.eye(4), np.eye(4), scs[1]["T"]])
    want = pc.fgr_batched(p1s, p2s, opts, table, T0=T0)
    assert not want[0]["failed"] and want[1]["failed"] and want[2]["failed"] and not want[3]["failed"]
    for nlhs in (1, 2, 3, 4):
        rc, msg, T, inl, n_inl, stats, kept, off = _round_trip(drv, p1s, p2s, _o(**opts), nlhs, table, T0)
        assert rc == 0, msg
        assert drv.fd_live_arrays() == 0
        k = 0
        for b, w in enumerate(want):
            np.testing.assert_array_equal(_bits(T[b]), _bits(np.zeros((4, 4)) if w["failed"] else w["T"]))
            if nlhs > 1:
                np.testing.assert_array_equal(inl[k:k + w["n_inliers"]], w["inlier_idx"].astype(np.float64))
                k += w["n_inliers"]
            if nlhs > 2:
                assert stats[b, :4].tolist() == [float(w["failed"]), w["n_live"], w["n_kept"], w["n_inliers"]] and stats[b, 8] == len(p1s[b])
                np.testing.assert_array_equal(_bits(stats[b, 4:8]), _bits([w["mu0"], w["mu_final"], w["cost"], w["sum_d2"]]))
            if nlhs > 3:
                np.testing.assert_array_equal(kept[off[b]:off[b + 1]].astype(bool), w["kept"])
        assert n_inl == (k if nlhs > 1 else -1)
    rc, msg, T, inl, n_inl, stats, kept, off = _round_trip(drv, [], [], _o(), 4)          # B = 0: empty outputs, no call
    assert rc == 0 and n_inl == 0 and drv.fd_live_arrays() == 0


def test_wrappers_call_the_command_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    assert "'fgrBatched'" in head and "fgrBatched.m" in head and "pcregisterfgrFast.m" in head
    block = gw.split('strcmp(cmd, "fgrBatched")')[1].split("strcmp(cmd,")[0]
    assert "nrhs < 5 || nrhs > 7" in block and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 3 and "pcreg_fgr_batched(" in block
    src = open(os.path.join(ROOT, "matlab", "fgrBatched.m")).read()
    assert src.startswith("function [TCells, inlierCells, stats, keptCells] = fgrBatched(pts1Cells, pts2Cells, opts, tupleCells, T0Cells)")
    assert "[T, inlierIdx, s, kept] = pcreg_mex('fgrBatched', pts1, pts2, offsets, opts, tupleIdx, T0);" in src          # 7 arguments, 4 outputs
    assert "offsets = int32([0; cumsum(lens)]);" in src and "zeros(3, opts.n_tuples * B, 'int32')" in src
    for col, name in enumerate(("failed", "n_live", "n_kept", "n_inliers", "mu0", "mu_final", "cost", "sum_d2"), 1):
        assert f"'{name}', s(:, {col})" in src                        # the gateway's column order
    assert re.search(r"const double v\[9\] = \{\(double\)r\[b\]\.failed, \(double\)r\[b\]\.n_live, \(double\)r\[b\]\.n_kept, \(double\)r\[b\]\.n_inliers, "
                     r"r\[b\]\.mu0, r\[b\]\.mu_final,\s+r\[b\]\.cost, r\[b\]\.sum_d2", block)
    reg = open(os.path.join(ROOT, "matlab", "pcregisterfgrFast.m")).read()
    assert reg.startswith("function [T, info] = pcregisterfgrFast(moving, fixed, gridStep, varargin)")
    for call in ("pcdownsampleFast(moving, gridStep)", "pcdownsampleFast(fixed, gridStep)", "pcnormalsFast(movingDown, k)", "pcnormalsFast(fixedDown, k)",
                 "extractFPFHFast(movingDown, 'NumNeighbors', k, 'Normals'", "getMatches(descMoving, descFixed, match)",
                 "fgrBatched({double(fixedDown(matches(:, 2), :))}, {double(movingDown(matches(:, 1), :))}, opts)"):
        assert call in reg, call
    import pcreg_amd as pc
    for k, v in pc.api.REGISTER_FGR_MATCH.items():                    # the same match parameters as register_fgr
        lit = f"'{v}'" if isinstance(v, str) else ("true" if v is True else "false" if v is False else f"{v:g}")
        assert f"'{k}', {lit}" in reg, k
    for w in ("fgrBatched", "pcregisterfgrFast"):
        assert os.path.exists(os.path.join(ROOT, "matlab", w + ".m"))
