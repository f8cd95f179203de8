"""The clustering's C ABI and MEX commands without a GPU: the entry points are exported, declared and listed; argument errors (a
negative or NaN r2, null pointers, bad sizes) are PCREG_E_ARG before anything runs; a valid call without a device is
PCREG_E_NODEVICE; the workspace follows the header's formula; the debug keys exist; knn_cluster.hip holds no loop that waits for
another workgroup; the 'modelCluster' / 'clusterPoints' commands of mex/pcreg_mex.cpp (tests/mexcluster/cluster_driver.cpp on
tests/mexstub/mex.h) refuse bad usage through mexErrMsgIdAndTxt and leak no array; the MATLAB wrappers call them the way the
gateway checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_cluster_workspace", "pcreg_dev_model_cluster_f32", "pcreg_model_cluster_f32", "pcreg_cluster_points_f32",
       "pcreg_debug_cluster_stats", "pcreg_model_size")


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
    assert '"cluster_noskip"' in head and '"cluster_stats"' in head
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    from pcreg_amd.sweep import promising_clusters
    assert callable(pc.cluster_points) and callable(pc.Model.cluster) and callable(PreparedModel.cluster) and callable(promising_clusters)
    assert "cluster_points" in pc.__all__


def test_the_debug_keys_exist():
    _l, L = _lib()
    for key in (b"cluster_noskip", b"cluster_stats"):
        assert L.pcreg_debug_set(key, 1) == _l.PCREG_OK
        assert L.pcreg_debug_set(key, 0) == _l.PCREG_OK
    out = (C.c_longlong * 4)(1, 2, 3, 4)
    assert L.pcreg_debug_cluster_stats(out, 0) == _l.PCREG_OK and list(out) == [0, 0, 0, 0]      # never on: zeros, no device needed
    assert L.pcreg_debug_cluster_stats(None, 0) == _l.PCREG_E_ARG


def test_workspace_follows_the_headers_formula():
    """include/pcreg.h: 2 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes: O(M), no other argument"""
    _, L = _lib()
    f = L.pcreg_dev_model_cluster_workspace
    up = lambda x: (x + 255) // 256 * 256
    for M in (0, 1, 512, 513, 10 ** 6):
        assert f(M) == 2 * up(4 * max(M, 1)) + up(4 * max((M + 2047) // 2048, 1)), M
    assert f(0) == f(1) == 768
    assert f(10 ** 6) <= 8 * 10 ** 6 + 4096
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "2 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256)" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    nc = C.c_int32(0)
    n = C.byref(nc)
    p = lambda a: a.ctypes.data
    fake = 16                                          # never dereferenced: the checks refuse first
    E = _l.PCREG_E_ARG
    big = 1 << 40
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert L.pcreg_cluster_points_f32(p(buf), 4, 4, r2, p(ib), n, p(ib), p(ib)) == E, r2
        assert L.pcreg_model_cluster_f32(fake, r2, p(ib), n, p(ib), p(ib)) == E
        assert L.pcreg_dev_model_cluster_f32(fake, r2, p(ib), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert b"bad argument" in L.pcreg_last_error()
    # null pointers; cl_off and members come together or not at all
    assert L.pcreg_cluster_points_f32(None, 4, 4, 1.0, p(ib), n, p(ib), p(ib)) == E
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 1.0, None, n, p(ib), p(ib)) == E
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 1.0, p(ib), None, p(ib), p(ib)) == E
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 1.0, p(ib), n, None, p(ib)) == E
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 1.0, p(ib), n, p(ib), None) == E
    assert L.pcreg_model_cluster_f32(None, 1.0, p(ib), n, p(ib), p(ib)) == E
    assert L.pcreg_model_cluster_f32(fake, 1.0, p(ib), None, p(ib), p(ib)) == E
    assert L.pcreg_model_cluster_f32(fake, 1.0, p(ib), n, None, p(ib)) == E
    assert L.pcreg_dev_model_cluster_f32(None, 1.0, p(ib), p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_cluster_f32(fake, 1.0, None, p(ib), p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_cluster_f32(fake, 1.0, p(ib), None, p(ib), p(ib), p(buf), big, None) == E
    assert L.pcreg_dev_model_cluster_f32(fake, 1.0, p(ib), p(ib), p(ib), p(ib), None, big, None) == E
    assert L.pcreg_model_size(None, n) == E and L.pcreg_model_size(fake, None) == E
    # bad sizes
    assert L.pcreg_cluster_points_f32(p(buf), -1, 4, 1.0, p(ib), n, p(ib), p(ib)) == E
    assert L.pcreg_cluster_points_f32(p(buf), 4, 3, 1.0, p(ib), n, p(ib), p(ib)) == E
    # the Python tiers refuse a bad radius themselves
    import pcreg_amd as pc
    for r2 in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pc.cluster_points(np.zeros((5, 3)), r2)


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    buf = np.zeros(64 * 3, np.float32)
    ib = np.zeros(256, np.int32)
    nc = C.c_int32(0)
    p = lambda a: a.ctypes.data
    N = _l.PCREG_E_NODEVICE
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 1.0, p(ib), C.byref(nc), p(ib), p(ib)) == N
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, 0.0, p(ib), C.byref(nc), None, None) == N              # label alone
    assert L.pcreg_cluster_points_f32(p(buf), 4, 4, float("inf"), p(ib), C.byref(nc), None, None) == N
    assert L.pcreg_cluster_points_f32(None, 0, 0, 1.0, None, C.byref(nc), None, None) == N                 # M = 0 needs no array
    assert L.pcreg_dev_model_cluster_f32(16, 1.0, p(ib), p(ib), None, None, p(buf), 1 << 20, None) == N    # first / sizes may be NULL
    with pytest.raises(PcregError) as e:
        pc.cluster_points(np.zeros((5, 3)), 4.0)
    assert e.value.code == N


def test_the_kernels_wait_for_nobody():
    """knn_cluster.hip: no fence, no sleep, no flag to spin on.  Its only loops whose exit depends on global memory are find
    (follows parent[] downwards: parent[x] <= x) and the compare-and-swap retry of unite (bounded by the number of merges)."""
    src = open(os.path.join(ROOT, "pcreg_amd", "csrc", "knn_cluster.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    code = code[:code.index("struct ClusterWs")]                    # the device code: everything before the host launcher
    for word in ("__threadfence", "__builtin_amdgcn_fence", "s_sleep", "__builtin_amdgcn_s_sleep", "atomicExch", "volatile", "__hip_atomic_exchange",
                 "__hip_atomic_fetch", "flag", "ticket", "do {", "do{"):
        assert word not in code, word
    whiles = re.findall(r"while\s*\(([^\n]*)\)\s*\{", code)
    assert sorted(w.strip() for w in whiles) == sorted(["cur > (next = uf_load(parent, cur))", "ra != rb", "true", "todo"]), whiles
    # (`while (todo)` walks a ballot mask in registers: the label kernel's per-wave count of equal clusters; no memory in its condition)
    assert re.search(r"todo &= ~same;", code)
    assert code.count("__hip_atomic_compare_exchange_strong") == 1
    # the `while (true)` is the flatten kernel's read-only walk to the root; it leaves by `if (n == r) break`
    assert re.search(r"while \(true\) \{ const int n = uf_load\(parent, r\); if \(n == r\) break; r = n; \}", code)
    # every access to parent[] inside the walk launch goes through the relaxed agent-scope helpers
    walk = code[code.index("void cluster_walk_kernel"):code.index("void cluster_flatten_kernel")]
    assert "parent[" not in walk and "uf_load(parent" in walk and "uf_unite(parent" in walk
    helpers = code[code.index("uf_load"):code.index("void cluster_init_kernel")]
    assert "#define PCREG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT" in code
    assert helpers.count("PCREG_RLX_AGENT") >= 2 and "__ATOMIC_RELAXED, __ATOMIC_RELAXED" in helpers and "__HIP_MEMORY_SCOPE_AGENT" in helpers
    assert "__ATOMIC_SEQ_CST" not in code and "__ATOMIC_ACQ" not in code and "__ATOMIC_RELEASE" not in code


# ---- the MEX commands --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexcluster") / "libmexcluster.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexcluster", "cluster_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.cd_usage.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    L.cd_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("via_handle", [0, 1])
@pytest.mark.parametrize("nargs, first_double, r_kind, r", [(1, 0, 0, 1.0), (3, 0, 0, 1.0), (2, 1, 0, 1.0), (2, 0, 0, -1.0), (2, 0, 0, float("nan")),
                                                            (2, 0, 1, 2.0), (2, 0, 2, 1.0)])
def test_usage_errors(drv, via_handle, nargs, first_double, r_kind, r):
    """wrong argument counts, a double cloud / handle, a negative / NaN radius, an int32 radius, a 1 x 2 radius"""
    e = _err()
    assert drv.cd_usage(via_handle, nargs, first_double, r_kind, r, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: " + ("modelCluster:" if via_handle else "clusterPoints:")), e.value
    assert drv.cd_live_arrays() == 0


def test_a_null_handle_is_a_library_error(drv):
    e = _err()
    assert drv.cd_usage(1, 2, 0, 0, 1.5, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
    assert drv.cd_live_arrays() == 0


def test_the_commands_report_nodevice_through_mexerr(drv):
    _no_gpu()
    m = np.asfortranarray(np.random.default_rng(0).random((20, 3)).astype(np.float32))
    for via_handle in (0, 1):
        label = np.zeros(20, np.int32); off = np.zeros(21, np.int32); mem = np.zeros(20, np.int32); e = _err(); nc = C.c_int(-1)
        assert drv.cd_round_trip(via_handle, m.ctypes.data, 20, 0.5, label.ctypes.data, off.ctypes.data, C.byref(nc), mem.ctypes.data, e, 1024) == 1
        assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
        assert drv.cd_live_arrays() == 0


def test_the_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for cmd, wrapper, call in (("modelCluster", "clusterPointsModel.m", "[~, clOff, members] = pcreg_mex('modelCluster', h, r);"),
                               ("clusterPoints", "clusterPointsFast.m", "[~, clOff, members] = pcreg_mex('clusterPoints', single(pts), r);")):
        src = open(os.path.join(ROOT, "matlab", wrapper)).read()
        assert call in src and "mat2cell" in src and "double(members" in src                   # 3 arguments, 3 outputs, a cell of doubles
        assert "rangesearch" not in src.split("\n", 1)[1].replace("%", "")                     # no Statistics Toolbox call
        block = gw.split('strcmp(cmd, "%s")' % cmd)[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != 3\b", block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == 2
        assert "'" + cmd + "'" in head and wrapper in head
