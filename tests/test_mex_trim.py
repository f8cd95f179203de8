"""The trimmed scoring and refits' MEX commands and MATLAB wrappers, in the manner of tests/test_mex_refit_gicp.py.
Without a GPU: the four commands of mex/pcreg_mex.cpp (tests/mextrim/trim_driver.cpp on tests/mexstub/mex.h) refuse bad usage through
mexErrMsgIdAndTxt and leak no array; the wrappers call them the way the gateway checks, and without 'InlierRatio' they go to the
untrimmed wrappers, which call the commands they always called.  With one: the four commands on a 300-row model equal the Python
host tier bit for bit, and the untrimmed command through the same driver path equals the untrimmed host call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("modelScoreTrimmed", "modelRefitTrimmed", "modelRefitPlaneTrimmed", "modelRefitGicpTrimmed")
NRHS = (6, 7, 9, 11)
NOUT = (6, 5, 7, 7)


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mextrim") / "libmextrim.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mextrim", "trim_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.td_usage.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.td_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("which", range(4), ids=NAMES)
@pytest.mark.parametrize("kw", [dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.5), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(r=-1.0),
                                dict(r=float("nan")), dict(drop=1), dict(extra=1), dict(bad_ratio_class=1), dict(steps=0.0), dict(steps=1.5)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_usage_errors(drv, which, kw):
    """keepRatio 0, negative, above 1, NaN, inf or single; a negative / NaN radius; an argument too few or too many; steps 0 or fractional"""
    if which == 0 and "steps" in kw:
        return                                                 # (scoring takes no steps)
    a = dict(dict(r=1.0, ratio=0.5, steps=1.0, drop=0, extra=0, bad_ratio_class=0), **kw)
    e = _err()
    assert drv.td_usage(which, a["r"], a["ratio"], a["steps"], a["drop"], a["extra"], a["bad_ratio_class"], e, 1024) == 1
    assert e.value.decode().startswith(f"pcreg:usage: {NAMES[which]}:"), e.value
    assert drv.td_live_arrays() == 0


@pytest.mark.parametrize("which", range(4), ids=NAMES)
@pytest.mark.parametrize("ratio", [0.5, 1.0, 5e-324])
def test_null_handle_is_a_library_error(drv, which, ratio):
    e = _err()
    assert drv.td_usage(which, 1.5, ratio, 2.0, 0, 0, 0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.td_live_arrays() == 0


_NP = {0: np.float64, 1: np.float32, 2: np.int32}


def _round_trip(drv, which, m, pts, T16, r, ratio, steps, normals, qnormals, k, eps, nlhs):
    cap = 8 * max(16 * len(T16), len(pts) * len(T16), 1)
    bufs = [np.zeros(cap, np.uint8) for _ in range(7)]
    out = (C.c_void_p * 7)(*[b.ctypes.data for b in bufs])
    cls, rows, cols = ((C.c_int * 7)(*([-1] * 7)) for _ in range(3))
    e, n_out = _err(), C.c_int(-1)
    col = lambda a: None if a is None else np.asfortranarray(a, np.float32) if len(a) else np.zeros((1, 3), np.float32, order="F")
    mf, pf, nf, qf = col(m), col(pts), col(normals), col(qnormals)
    rc = drv.td_round_trip(which, mf.ctypes.data, len(m), pf.ctypes.data, len(pts), T16.ctypes.data, len(T16), float(r), float(ratio), steps,
                           None if nf is None else nf.ctypes.data, 0 if normals is None else len(normals), None if qf is None else qf.ctypes.data,
                           0 if qnormals is None else len(qnormals), k, float(eps), nlhs, out, cap, cls, rows, cols, C.byref(n_out), e, 1024)
    got = []
    for j in range(7):
        if cls[j] < 0:
            continue
        dt = _NP[cls[j]]
        got.append(bufs[j][:rows[j] * cols[j] * np.dtype(dt).itemsize].view(dt).reshape(cols[j], rows[j]).copy())      # column-major: [cols][rows]
    return rc, e.value.decode(), n_out.value, got


def test_commands_report_nodevice_through_mexerr(drv):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    m = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    T16 = np.eye(4).ravel(order="F")[None].copy()
    for which in range(4):
        rc, msg, *_ = _round_trip(drv, which, m, m[:5], T16, 0.5, 0.5, 1, None, None, 6, 1e-3, NOUT[which])
        assert rc == 1 and msg.startswith("pcreg:hip") and "no CPU fallback" in msg, (which, msg)
        assert drv.td_live_arrays() == 0


def _pages(a, B):
    """a 4 x 4 x B output as the driver returns it ([4 B][4]) -> [B, 4, 4] as quickTF uses them"""
    return np.ascontiguousarray(a.reshape(B, 16).reshape(B, 4, 4).transpose(0, 2, 1))


@pytest.mark.gpu
def test_round_trips_equal_the_host_tier(drv):
    """the four trimmed commands on a 300-row model with every output, and 'modelRefit' through the same path as the wrapper calls it
    without 'InlierRatio': maxDist squared once in single, 1-based idx with 0 for none, a zero page for an empty result; the same
    bits as Model.score_transforms / refit_transforms / refit_plane / refit_gicp with keep_ratio"""
    import pcreg_amd as pc
    import plane_ref
    sc = plane_ref.scene()
    m = sc["model"][:300]
    pts = sc["cloud"][:200].astype(np.float32)
    pts = pts[np.argsort(np.linalg.norm(pts[:, None, :] - m[None, :, :], axis=2).min(axis=1))][:120]      # the points nearest the 300 rows
    B = 4
    T = np.tile(np.eye(4), (B, 1, 1))
    rng = np.random.default_rng(5)
    for b in range(1, B):
        T[b, 3, :3] = rng.normal(size=3) * 0.05 * b
    T[2] = 0.0
    T16 = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)
    r, ratio, eps, steps = 2.5, 0.6, 1e-2, 2
    r2 = np.float32(r) * np.float32(r)
    with pc.Model(m) as h, pc.Model(pts) as hq:
        nrm, nq = h.normals(8), hq.normals(8)
        want = [h.score_transforms(pts, T, r2, rows=True, keep_ratio=ratio), h.refit_transforms(pts, T, r2, steps=steps, keep_ratio=ratio),
                h.refit_plane(pts, T, r2, steps=steps, normals=nrm, keep_ratio=ratio),
                h.refit_gicp(pts, T, r2, steps=steps, normals=nrm, query_normals=nq, epsilon=eps, keep_ratio=ratio)]
        plain = h.refit_transforms(pts, T, r2, steps=steps)
    assert want[0]["n_within"][0] > 50 and want[0]["n_close"][0] < want[0]["n_within"][0] and want[0]["n_within"][2] == 0       # premises
    same = lambda a, b: np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    for which in range(4):
        rc, msg, n_out, got = _round_trip(drv, which, m, pts, T16, r, ratio, steps, nrm, nq, 8, eps, NOUT[which])
        assert rc == 0, msg
        assert n_out == NOUT[which] and drv.td_live_arrays() == 0
        w = want[which]
        if which == 0:
            n_close, sum_d2, idx, d2, n_within, cut = got
            same(n_close[0], w["n_close"]); same(sum_d2[0], w["sum_d2"]); same(idx, w["idx"] + 1); same(d2, w["dist"])
        else:
            same(_pages(got[0], B), w["T"])
            for b in range(B):
                assert w["empty"][b] == (not _pages(got[0], B)[b].any())
            same(got[1][0], w["n_close"]); same(got[2][0], w["sum_d2"])
            if which >= 2:
                same(got[3][0], w["n_plane" if which == 2 else "n_pairs"]); same(got[4][0], w["sum_res2"])
            n_within, cut = got[-2:]
        same(n_within[0], w["n_within"]); same(cut[0], w["d2_cut"])
        assert n_within.dtype == np.int32 and cut.dtype == np.float32
        rc, msg, n_out, got1 = _round_trip(drv, which, m, pts, T16, r, ratio, steps, nrm, nq, 8, eps, 1)           # one output
        assert rc == 0 and n_out == (2 if which == 0 else 1) and drv.td_live_arrays() == 0, msg
    # without 'InlierRatio' the wrapper's path ends in 'modelRefit': the untrimmed host call's bits
    rc, msg, n_out, got = _round_trip(drv, 1, m, pts, T16, r, 0.0, steps, None, None, 8, eps, 3)
    assert rc == 0 and n_out == 3, msg
    same(_pages(got[0], B), plain["T"]); same(got[1][0], plain["n_close"]); same(got[2][0], plain["sum_d2"])


def test_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    files = ("scoreTransformsTrimmedModel", "refitTransformsTrimmedModel", "refitPlaneTrimmedModel", "refitGicpTrimmedModel")
    old = ("scoreTransformsModel", "refitTransformsModel", "refitPlaneModel", "refitGicpModel")
    entry = ("pcreg_model_score_trimmed_f32", "pcreg_model_refit_trimmed_f32", "pcreg_model_refit_plane_trimmed_f32", "pcreg_model_refit_gicp_trimmed_f32")
    for which, name in enumerate(NAMES):
        block = gw.split(f'strcmp(cmd, "{name}")')[1].split("strcmp(cmd,")[0]
        assert re.search(rf"nrhs != {NRHS[which]}\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == NOUT[which] - 1
        assert "r * r" in block and entry[which] + "(" in block and "ratio_ok(prhs[5])" in block
        assert f"'{name}'" in head and files[which] + ".m" in head
        src = open(os.path.join(ROOT, "matlab", files[which] + ".m")).read()
        assert src.startswith("function [") and f"= {files[which]}(h, pts, T, maxDist, varargin)" in src.split("\n")[0]
        assert src.split("\n")[0].count(",") == NOUT[which] - 1 + (1 if which == 0 else 0) + 4           # the outputs (scoring adds fitness, rmse for sumD2)
        assert f"pcreg_mex('{name}', h, single(pts), " in src and "double(rho)" in src and "'InlierRatio'" in src
        assert f"= {old[which]}(h, pts, T, maxDist, args{{:}});" in src                                 # without the pair: the untrimmed wrapper
        assert files[which] in integ and entry[which] in integ
    # ... and the untrimmed wrappers still call the commands they always called
    for f, cmd in zip(old, ("modelScore", "modelRefit", "modelRefitPlane", "modelRefitGicp")):
        src = open(os.path.join(ROOT, "matlab", f + ".m")).read()
        assert f"pcreg_mex('{cmd}'," in src and "Trimmed" not in src
