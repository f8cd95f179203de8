"""DBSCAN's C ABI and MEX commands without a GPU: the entry points are exported, declared and listed; argument errors (a negative or
NaN r2, minpts < 1, null pointers, one of cl_off / members alone, bad sizes) are PCREG_E_ARG before anything runs; a valid call
without a device is PCREG_E_NODEVICE; the workspace follows the header's formula; knn_dbscan.hip holds no fence and no loop that
waits on global memory; the 'modelDbscan' / 'dbscanPoints' commands of mex/pcreg_mex.cpp (tests/mexdbscan/dbscan_driver.cpp on
tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array; the MATLAB wrappers call them the way the
gateway checks; the sweep's min_spheres keyword, on the CPU references."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_ref
import dbscan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_dbscan_workspace", "pcreg_dev_model_dbscan_f32", "pcreg_model_dbscan_f32", "pcreg_dbscan_points_f32")


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
    from pcreg_amd.device import PreparedModel
    assert callable(pc.dbscan_points) and callable(pc.Model.dbscan) and callable(PreparedModel.dbscan)
    assert "dbscan_points" in pc.__all__
    assert "knn_dbscan.hip" in open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()


def test_workspace_follows_the_headers_formula():
    """include/pcreg.h: 4 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes: O(M), no other argument"""
    _, L = _lib()
    f = L.pcreg_dev_model_dbscan_workspace
    up = lambda x: (x + 255) // 256 * 256
    for M in (0, 1, 512, 513, 10 ** 6):
        assert f(M) == 4 * up(4 * max(M, 1)) + up(4 * max((M + 2047) // 2048, 1)), M
    assert f(0) == f(1) == 1280
    assert f(10 ** 6) <= 16 * 10 ** 6 + 4096
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "4 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256)" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    ub = np.zeros(256, np.uint8)
    nc = C.c_int32(0)
    n = C.byref(nc)
    p = lambda a: a.ctypes.data
    fake = 16                                          # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    big = 1 << 40
    pts = lambda *a: L.pcreg_dbscan_points_f32(*a)
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert pts(p(buf), 4, 4, r2, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E, r2
        assert L.pcreg_model_dbscan_f32(fake, r2, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
        assert L.pcreg_dev_model_dbscan_f32(fake, r2, 3, p(ib), p(ib), p(ub), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    for minpts in (0, -1, -2 ** 31):
        assert pts(p(buf), 4, 4, 1.0, minpts, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E, minpts
        assert L.pcreg_model_dbscan_f32(fake, 1.0, minpts, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
        assert L.pcreg_dev_model_dbscan_f32(fake, 1.0, minpts, p(ib), p(ib), p(ub), p(ib), p(ib), p(ib), p(buf), big, None) == E
    # null pointers; cl_off and members come together or not at all
    assert pts(None, 4, 4, 1.0, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
    assert pts(p(buf), 4, 4, 1.0, 3, None, n, p(ub), p(ib), p(ib), p(ib)) == E                       # a NULL label with M > 0
    assert pts(p(buf), 4, 4, 1.0, 3, p(ib), None, p(ub), p(ib), p(ib), p(ib)) == E                   # a NULL n_clusters
    assert pts(p(buf), 4, 4, 1.0, 3, p(ib), n, p(ub), p(ib), None, p(ib)) == E
    assert pts(p(buf), 4, 4, 1.0, 3, p(ib), n, p(ub), p(ib), p(ib), None) == E
    assert L.pcreg_model_dbscan_f32(None, 1.0, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
    assert L.pcreg_model_dbscan_f32(fake, 1.0, 3, p(ib), None, p(ub), p(ib), p(ib), p(ib)) == E
    assert L.pcreg_model_dbscan_f32(fake, 1.0, 3, p(ib), n, p(ub), p(ib), None, p(ib)) == E
    assert L.pcreg_dev_model_dbscan_f32(None, 1.0, 3, p(ib), p(ib), p(ub), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_dbscan_f32(fake, 1.0, 3, None, p(ib), p(ub), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_dbscan_f32(fake, 1.0, 3, p(ib), None, p(ub), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_dbscan_f32(fake, 1.0, 3, p(ib), p(ib), p(ub), p(ib), p(ib), p(ib), None, big, None) == E
    # bad sizes
    assert pts(p(buf), -1, 4, 1.0, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
    assert pts(p(buf), 4, 3, 1.0, 3, p(ib), n, p(ub), p(ib), p(ib), p(ib)) == E
    # the Python tiers refuse a bad radius and a bad minpts themselves
    import pcreg_amd as pc
    for r2, minpts in ((-1.0, 3), (float("nan"), 3), (1.0, 0), (1.0, 2.5), (1.0, -4)):
        with pytest.raises(ValueError):
            pc.dbscan_points(np.zeros((5, 3)), r2, minpts)


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    ub = np.zeros(256, np.uint8)
    nc = C.c_int32(0)
    p = lambda a: a.ctypes.data
    N = _l.PCREG_E_NODEVICE
    assert L.pcreg_dbscan_points_f32(p(buf), 4, 4, 1.0, 3, p(ib), C.byref(nc), p(ub), p(ib), p(ib), p(ib)) == N
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_dbscan_points_f32(p(buf), 4, 4, 0.0, 1, p(ib), C.byref(nc), None, None, None, None) == N           # label alone
    assert L.pcreg_dbscan_points_f32(p(buf), 4, 4, float("inf"), 9, p(ib), C.byref(nc), None, None, None, None) == N  # minpts > M is valid
    assert L.pcreg_dbscan_points_f32(None, 0, 0, 1.0, 3, None, C.byref(nc), None, None, None, None) == N              # M = 0 needs no array
    assert L.pcreg_dev_model_dbscan_f32(16, 1.0, 3, p(ib), p(ib), None, None, None, None, p(buf), 1 << 20, None) == N  # four outputs may be NULL
    with pytest.raises(PcregError) as e:
        pc.dbscan_points(np.zeros((5, 3)), 4.0, 2)
    assert e.value.code == N


def test_the_new_kernels_wait_for_nobody():
    """knn_dbscan.hip: no fence, no sleep, no atomic, no flag to spin on, and no loop at all outside the shared walk (knn_walk.hpp's
    loops run over tile numbers and LDS lists).  The core walk lives in knn_cluster.hip on its union-find, which
    tests/test_cluster_abi.py pins; it adds no `while` there."""
    src = open(os.path.join(ROOT, "pcreg_amd", "csrc", "knn_dbscan.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    code = code[:code.index("void enqueue_dbscan_count")]                  # the device code: everything before the host launchers
    for word in ("__threadfence", "__builtin_amdgcn_fence", "s_sleep", "__builtin_amdgcn_s_sleep", "atomic", "volatile", "__hip_atomic",
                 "flag", "ticket", "do {", "do{", "while", "goto", "__ATOMIC"):
        assert word not in code, word
    assert code.count("for (") == 2 == code.count("for (int u = 0; u < 4; ++u)")          # the unrolled four rows of a trip
    # the border walk reads parent[] of staged (core) rows and writes parent[] of its own (non-core) row, after the flatten launch
    border = code[code.index("void dbscan_border_kernel"):]
    assert "best = min(best, parent[__float_as_int(p[u].w)]);" in border and "parent[q.row_i] = best;" in border
    assert "walk_row_core(ms, perm, M, cnt_sorted, minpts, r)" in border and "cnt_sorted[q.sr] < minpts" in border
    assert "__syncthreads_or(live ? 1 : 0)" in border
    # the count walk: one plain store per row
    count = code[code.index("void dbscan_count_kernel"):code.index("void dbscan_init_kernel")]
    assert count.count("cnt_sorted[") == 1 and "__shfl_xor(n, 1)" in count and "__shfl_xor(n, 2)" in count
    # the core walk is cluster_walk_kernel under a compile-time switch, on uf_unite
    cl = open(os.path.join(ROOT, "pcreg_amd", "csrc", "knn_cluster.hip")).read()
    assert "template <bool kCoreOnly>" in cl and "cluster_walk_kernel<true>" in cl and "cluster_walk_kernel<false>" in cl
    assert cl.count("__hip_atomic_compare_exchange_strong") == 1


# ---- the MEX commands --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexdbscan") / "libmexdbscan.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexdbscan", "dbscan_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.dd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.dd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, first_double, r_kind, r, k_kind, minpts",
                         [(2, 0, 0, 1.0, 0, 3.0), (4, 0, 0, 1.0, 0, 3.0), (3, 1, 0, 1.0, 0, 3.0), (3, 0, 0, -1.0, 0, 3.0), (3, 0, 0, float("nan"), 0, 3.0),
                          (3, 0, 1, 2.0, 0, 3.0), (3, 0, 2, 1.0, 0, 3.0), (3, 0, 0, 1.0, 0, 0.0), (3, 0, 0, 1.0, 0, 2.5), (3, 0, 0, 1.0, 0, float("nan")),
                          (3, 0, 0, 1.0, 1, 3.0), (3, 0, 0, 1.0, 2, 3.0), (3, 0, 0, 1.0, 0, -2.0)])
def test_usage_errors(drv, via_handle, nargs, first_double, r_kind, r, k_kind, minpts):
    """wrong argument counts, a double cloud / handle, a negative / NaN radius, an int32 radius, a 1 x 2 radius, minpts 0, 2.5, NaN,
    int32, 1 x 2, negative"""
    e = _err()
    assert drv.dd_usage(via_handle, nargs, first_double, r_kind, r, k_kind, minpts, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: " + ("modelDbscan:" if via_handle else "dbscanPoints:")), e.value
    assert drv.dd_live_arrays() == 0


def test_a_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.dd_usage(1, 3, 0, 0, 1.5, 0, 3.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.dd_live_arrays() == 0


def test_the_commands_report_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.asfortranarray(np.random.default_rng(0).random((20, 3)).astype(np.float32))
    for via_handle in (0, 1):
        label = np.zeros(20, np.int32); core = np.zeros(20, np.uint8); off = np.zeros(21, np.int32); mem = np.zeros(20, np.int32)
        e = _err(); nc = C.c_int(-1); nm = C.c_int(-1)
        assert drv.dd_round_trip(via_handle, m.ctypes.data, 20, 0.5, 3.0, label.ctypes.data, core.ctypes.data, off.ctypes.data, C.byref(nc),
                                 mem.ctypes.data, C.byref(nm), e, 1024) == 1
        assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
        assert drv.dd_live_arrays() == 0


def test_the_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for cmd, wrapper, call in (("modelDbscan", "dbscanModel.m", "[label, core, ~, ~] = pcreg_mex('modelDbscan', h, epsilon, minpts);"),
                               ("dbscanPoints", "dbscanFast.m", "[label, core, ~, ~] = pcreg_mex('dbscanPoints', single(X), epsilon, minpts);")):
        src = open(os.path.join(ROOT, "matlab", wrapper)).read()
        assert call in src and "idx = double(label(:));" in src and "corepts = logical(core(:));" in src   # 4 arguments, 4 outputs
        assert src.startswith("function [idx, corepts] = ")
        assert not any("dbscan(" in line for line in src.split("\n") if not line.lstrip().startswith("%"))   # no Statistics Toolbox call
        block = gw.split('strcmp(cmd, "%s")' % cmd)[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 4\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 3
        assert "'" + cmd + "'" in head and wrapper in head


# ---- the sweep's keyword, on the CPU references ---------------------------------------------------------------------------------
def test_min_spheres_on_the_cpu_references(monkeypatch):
    import pcreg_amd.sweep as sw
    calls = []

    def fake_cluster(pts, r2):
        calls.append(("cluster", len(pts), float(r2)))
        return cluster_ref.cluster(pts, r2)

    def fake_dbscan(pts, r2, minpts):
        calls.append(("dbscan", len(pts), float(r2), minpts))
        r = dbscan_ref.dbscan(pts, r2, minpts)
        return r["label"], r["core"], r["cl_off"], r["members"]
    monkeypatch.setattr(sw, "cluster_points", fake_cluster)
    monkeypatch.setattr(sw, "dbscan_points", fake_dbscan)
    g = np.array([[0, 0, 0], [5, 0, 0], [5, 5, 0], [100, 0, 0], [40, 40, 0], [45, 40, 0]], np.float64)
    n = len(g)
    T = []
    for t in range(n):
        Tt = np.eye(4); Tt[0, 1] = float(t); T.append(Tt)
    res = dict(centres=g, trial=np.arange(n), statsPutative=np.full(n, 300), statsSuccess=np.ones(n, np.int64), statsInliers=np.full(n, 50),
               statsRatio=np.full(n, 50.0), transforms=T)
    plain, none = sw.promising_clusters(res), sw.promising_clusters(res, min_spheres=None)
    assert calls == [("cluster", 6, 64.0), ("cluster", 6, 64.0)]                                   # the same call: same bits
    assert len(plain) == len(none) == 3
    for (la, Ta), (lb, Tb) in zip(plain, none):
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(Ta, Tb)
    two = sw.promising_clusters(res, min_spheres=2)
    assert calls[-1] == ("dbscan", 6, 64.0, 2) and len(two) == 2                                   # the sphere at (100, 0, 0) is in no cluster
    for (la, Ta), (lb, Tb) in zip(two, [plain[0], plain[2]]):
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(Ta, Tb)
    a, c = sw.largest_cluster(res), sw.largest_cluster(res, min_spheres=2)
    np.testing.assert_array_equal(a[0], [0, 1, 2]); np.testing.assert_array_equal(c[0], a[0]); np.testing.assert_array_equal(c[1], a[1])
    three = sw.largest_cluster(res, min_spheres=3)
    np.testing.assert_array_equal(three[0], [0, 1, 2])                                             # (40,40,0), (45,40,0): two spheres, noise
    assert sw.promising_clusters(res, min_spheres=4) == [] and sw.largest_cluster(res, min_spheres=4)[0].tolist() == []
