"""unique_rows / aggregate_matches / the indexed estimateTransform at the C ABI and the MEX boundary, without a GPU: the entry points
are exported, declared and listed; the workspaces follow the header's formulas; argument errors (null pointers, n < 0, ld < n, a
NaN at the host tier, a short workspace) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE;
the device code of unique_rows.hip holds no fence, sleep or loop that waits on memory; the 'uniqueRows3' / 'aggregateMatches'
commands of mex/pcreg_mex.cpp (tests/mexunique/unique_driver.cpp on tests/mexstub/mex.h) refuse bad usage through
mexErrMsgIdAndTxt and leak no array; the MATLAB wrappers call them the way the gateway checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_unique_rows3", "pcreg_aggregate_matches", "pcreg_dev_unique_rows3_workspace", "pcreg_dev_unique_rows3_f64",
       "pcreg_dev_aggregate_matches_workspace", "pcreg_dev_aggregate_matches", "pcreg_dev_estimate_transform_indexed")
T = 2048                                               # the tile of unique_rows.hip (kUT)


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
    from pcreg_amd.sweep import SphereSweep, largest_cluster, promising_clusters
    assert callable(pc.unique_rows) and callable(pc.aggregate_matches) and callable(largest_cluster) and callable(promising_clusters)
    assert callable(SphereSweep.aggregate)
    assert "unique_rows" in pc.__all__ and "aggregate_matches" in pc.__all__
    src = open(os.path.join(ROOT, "pcreg_amd", "csrc", "unique_rows.hip")).read()
    assert "constexpr int kUT = %d;" % T in src
    assert "unique_rows.hip" in open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()


def test_workspaces_follow_the_headers_formulas():
    _, L = _lib()
    up = lambda x: (x + 255) // 256 * 256
    uniq = lambda n: 2 * (3 * up(8 * max(n, 1)) + up(4 * max(n, 1))) + up(4 * max((n + 2047) // 2048, 1))
    for n in (0, 1, T, T + 1, 10 ** 6):
        assert L.pcreg_dev_unique_rows3_workspace(n) == uniq(n), n
        assert L.pcreg_dev_aggregate_matches_workspace(n) == 2 * up(4 * max(n, 1)) + 256 + up(24 * max(n, 1)) + uniq(n), n
    assert L.pcreg_dev_unique_rows3_workspace(0) == L.pcreg_dev_unique_rows3_workspace(1) == 2 * 4 * 256 + 256
    assert L.pcreg_dev_unique_rows3_workspace(10 ** 6) <= 56 * 10 ** 6 + 4096          # two buffers of 28-byte records
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    flat = re.sub(r"\s*\n \* ", " ", head)
    assert "2 * (3 * roundup(8 * max(n, 1), 256) + roundup(4 * max(n, 1), 256)) + roundup(4 * max(ceil(n / 2048), 1), 256) bytes" in flat
    assert "2 * roundup(4 * max(n, 1), 256) + 256 + roundup(24 * max(n, 1), 256) + pcreg_dev_unique_rows3_workspace(n) bytes" in flat


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    E = _l.PCREG_E_ARG
    a = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(8, 3))
    b = a.copy(order="F")
    o1 = np.zeros((8, 3), order="F"); o2 = np.zeros((8, 3), order="F")
    ia = np.zeros(8, np.int32)
    nu = C.c_int(0)
    p = lambda x: C.c_void_p(x.ctypes.data)
    n = C.byref(nu)
    big = C.c_size_t(1 << 40)
    fake = C.c_void_p(16)                              # never dereferenced: the checks refuse first
    # host tier: null pointers, n < 0, ld < n, a NaN anywhere
    assert L.pcreg_unique_rows3(None, 8, 8, p(ia), n) == E
    assert L.pcreg_unique_rows3(p(a), 8, 8, None, n) == E
    assert L.pcreg_unique_rows3(p(a), 8, 8, p(ia), None) == E
    assert L.pcreg_unique_rows3(p(a), -1, 8, p(ia), n) == E
    assert L.pcreg_unique_rows3(p(a), 8, 7, p(ia), n) == E
    assert b"bad argument" in L.pcreg_last_error()
    for r, c in ((0, 0), (7, 2), (3, 1)):
        bad = a.copy(order="F"); bad[r, c] = np.nan
        assert L.pcreg_unique_rows3(p(bad), 8, 8, p(ia), n) == E, (r, c)
        assert b"has_nan3" in L.pcreg_last_error()
        assert L.pcreg_aggregate_matches(p(bad), p(b), 8, 8, p(o1), p(o2), 8, p(ia), n) == E
        assert L.pcreg_aggregate_matches(p(a), p(bad), 8, 8, p(o1), p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(None, p(b), 8, 8, p(o1), p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), None, 8, 8, p(o1), p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), 8, 8, None, p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), 8, 8, p(o1), None, 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), 8, 8, p(o1), p(o2), 8, p(ia), None) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), -1, 8, p(o1), p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), 8, 7, p(o1), p(o2), 8, p(ia), n) == E
    assert L.pcreg_aggregate_matches(p(a), p(b), 8, 8, p(o1), p(o2), 7, p(ia), n) == E
    # device tier: null pointers, sizes, a workspace one byte short
    need = L.pcreg_dev_unique_rows3_workspace(8)
    f = L.pcreg_dev_unique_rows3_f64
    assert f(None, fake, 8, 8, 0, fake, fake, fake, big, None) == E
    assert f(fake, None, 8, 8, 0, fake, fake, fake, big, None) == E
    assert f(fake, fake, 8, 8, 0, None, fake, fake, big, None) == E
    assert f(fake, fake, 8, 8, 0, fake, None, fake, big, None) == E
    assert f(fake, fake, 8, 8, 0, fake, fake, None, big, None) == E
    assert f(fake, fake, -1, 8, 0, fake, fake, fake, big, None) == E
    assert f(fake, fake, 8, 7, 0, fake, fake, fake, big, None) == E
    assert f(fake, fake, 8, 8, 0, fake, fake, fake, C.c_size_t(need - 1), None) == E
    need = L.pcreg_dev_aggregate_matches_workspace(8)
    g = L.pcreg_dev_aggregate_matches
    assert g(None, fake, fake, 8, 8, fake, fake, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, None, fake, 8, 8, fake, fake, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, None, 8, 8, fake, fake, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, None, fake, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, fake, None, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, fake, fake, 8, 0, fake, None, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, fake, fake, 8, 0, fake, fake, None, big, None) == E
    assert g(fake, fake, fake, 8, 7, fake, fake, 8, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, fake, fake, 7, 0, fake, fake, fake, big, None) == E
    assert g(fake, fake, fake, 8, 8, fake, fake, 8, 0, None, fake, fake, C.c_size_t(need - 1), None) == E
    h = L.pcreg_dev_estimate_transform_indexed
    assert h(None, fake, 8, fake, 1, fake, 8, fake, fake, None) == E
    assert h(fake, fake, 8, None, 1, fake, 8, fake, fake, None) == E
    assert h(fake, fake, 8, fake, 1, None, 8, fake, fake, None) == E
    assert h(fake, fake, 8, fake, 1, fake, 8, None, fake, None) == E
    assert h(fake, fake, 8, fake, 1, fake, 8, fake, None, None) == E
    assert h(fake, fake, 7, fake, 1, fake, 8, fake, fake, None) == E
    assert h(fake, fake, 8, fake, 1, fake, -1, fake, fake, None) == E
    # the Python tier refuses a wrong shape itself
    import pcreg_amd as pc
    with pytest.raises(ValueError):
        pc.unique_rows(np.zeros((5, 2)))
    with pytest.raises(ValueError):
        pc.aggregate_matches(np.zeros((5, 3)), np.zeros((4, 3)))


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    N = _l.PCREG_E_NODEVICE
    a = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(8, 3))
    o1 = np.zeros((8, 3), order="F"); o2 = np.zeros((8, 3), order="F")
    ia = np.zeros(8, np.int32)
    nu = C.c_int(0)
    p = lambda x: C.c_void_p(x.ctypes.data)
    fake = C.c_void_p(16)
    assert L.pcreg_unique_rows3(p(a), 8, 8, p(ia), C.byref(nu)) == N
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_unique_rows3(None, 0, 0, None, C.byref(nu)) == N                                         # n = 0 needs no array
    assert L.pcreg_aggregate_matches(p(a), p(a), 8, 8, p(o1), p(o2), 8, None, C.byref(nu)) == N             # ia may be NULL
    big = C.c_size_t(1 << 30)
    assert L.pcreg_dev_unique_rows3_f64(fake, fake, 8, 8, 0, fake, fake, fake, big, None) == N
    assert L.pcreg_dev_aggregate_matches(fake, fake, fake, 8, 8, fake, fake, 8, 0, None, fake, fake, big, None) == N
    assert L.pcreg_dev_estimate_transform_indexed(fake, fake, 8, fake, 1, fake, 8, fake, fake, None) == N
    with pytest.raises(PcregError) as e:
        pc.unique_rows(np.zeros((5, 3)))
    assert e.value.code == N
    with pytest.raises(PcregError) as e:
        pc.aggregate_matches(np.zeros((5, 3)), np.zeros((5, 3)))
    assert e.value.code == N


def test_the_kernels_wait_for_nobody():
    """unique_rows.hip: no fence, no sleep, no atomic, no flag to spin on.  Its only `while` loops are binary searches whose
    condition is `lo < hi` over registers, and every pass halves hi - lo."""
    src = open(os.path.join(ROOT, "pcreg_amd", "csrc", "unique_rows.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    code = code[:code.index("struct UniqueWs")]                      # the device code: everything before the host launchers
    for word in ("__threadfence", "__builtin_amdgcn_fence", "s_sleep", "__builtin_amdgcn_s_sleep", "atomic", "volatile", "flag", "ticket",
                 "do {", "do{", "goto"):
        assert word not in code, word
    whiles = re.findall(r"while\s*\(([^\n]*)\)\s*\{", code)
    assert [w.strip() for w in whiles] == ["lo < hi", "lo < hi"], whiles
    assert code.count("lo = mid + 1") == 2 and code.count("hi = mid;") == 2 and code.count("const int mid = (lo + hi) >> 1;") == 2
    # every `for` has a trip count fixed by constants, the thread index or a register bound: none reads memory in its condition
    for cond in re.findall(r"for\s*\([^;]*;([^;]*);", code):
        assert "[" not in cond and "*" not in cond, cond
    # the kernels read n through one clamped helper
    assert code.count("read_n(n_dev, n_cap)") >= 6 and "return max(0, min(*n_dev, n_cap));" in code


# ---- the MEX commands --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("mexunique") / "libmexunique.so")
    srcs = [os.path.join(ROOT, "mex", "pcreg_mex.cpp"), os.path.join(ROOT, "tests", "mexunique", "unique_driver.cpp")]
    inc = ["-I" + os.path.join(ROOT, "tests", "mexstub"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", *inc, *srcs, "-o", out,
                           "-L" + os.path.join(ROOT, "pcreg_amd"), "-lpcreg_hip", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    L = C.CDLL(out)
    L.ud_usage.argtypes = [C.c_int] * 6 + [C.c_double, C.c_char_p, C.c_int]
    L.ud_round_trip.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return L


def _err():
    return C.create_string_buffer(1024)


@pytest.mark.parametrize("aggregate, nargs, first_single, n, cols, rows2", [
    (0, 0, 0, 4, 3, 4), (0, 2, 0, 4, 3, 4), (0, 1, 1, 4, 3, 4), (0, 1, 0, 4, 2, 4),              # counts, a single matrix, n x 2
    (1, 1, 0, 4, 3, 4), (1, 3, 0, 4, 3, 4), (1, 2, 1, 4, 3, 4), (1, 2, 0, 4, 2, 4), (1, 2, 0, 4, 3, 5)])     # ... and unequal rows
def test_usage_errors(drv, aggregate, nargs, first_single, n, cols, rows2):
    e = _err()
    assert drv.ud_usage(aggregate, nargs, first_single, n, cols, rows2, 1.0, e, 1024) == 1
    assert e.value.decode().startswith("pcreg:usage: " + ("aggregateMatches:" if aggregate else "uniqueRows3:")), e.value
    assert drv.ud_live_arrays() == 0


def test_a_nan_is_a_library_error(drv):
    for aggregate, nargs in ((0, 1), (1, 2)):
        e = _err()
        assert drv.ud_usage(aggregate, nargs, 0, 4, 3, 4, float("nan"), e, 1024) == 1
        assert e.value.decode().startswith("pcreg:hip: bad argument"), e.value
        assert drv.ud_live_arrays() == 0


def test_the_commands_report_nodevice_through_mexerr(drv):
    _no_gpu()
    a = np.asfortranarray(np.random.default_rng(0).integers(0, 3, (20, 3)).astype(np.float64))
    for aggregate in (0, 1):
        ia = np.zeros(20); o1 = np.zeros(60); o2 = np.zeros(60); e = _err(); nu = C.c_int(-1)
        assert drv.ud_round_trip(aggregate, a.ctypes.data, a.ctypes.data, 20, ia.ctypes.data, C.byref(nu), o1.ctypes.data, o2.ctypes.data, e, 1024) == 1
        assert e.value.decode().startswith("pcreg:hip") and "no CPU fallback" in e.value.decode()
        assert drv.ud_live_arrays() == 0


def test_the_wrappers_call_the_commands_as_the_gateway_checks():
    gw = open(os.path.join(ROOT, "mex", "pcreg_mex.cpp")).read()
    head = gw[:gw.index("#if __has_include")]
    for cmd, wrapper, call, nrhs, nout in (("uniqueRows3", "uniqueRowsFast.m", "ia = pcreg_mex('uniqueRows3', double(A));", 2, 1),
                                           ("aggregateMatches", "aggregateMatches.m",
                                            "[pts1, pts2, ia] = pcreg_mex('aggregateMatches', double(pts1_agg), double(pts2_agg));", 3, 3)):
        src = open(os.path.join(ROOT, "matlab", wrapper)).read()
        assert call in src
        assert "unique(" not in "\n".join(ln.split("%")[0] for ln in src.split("\n"))              # the wrapper does not call MATLAB's unique
        block = gw.split('strcmp(cmd, "%s")' % cmd)[1].split("strcmp(cmd,")[0]
        assert re.search(r"nrhs != %d\b" % nrhs, block) and max(int(k) for k in re.findall(r"plhs\[(\d+)\]", block)) == nout - 1
        assert "'" + cmd + "'" in head and wrapper in head
    assert "C = A(ia, :);" in open(os.path.join(ROOT, "matlab", "uniqueRowsFast.m")).read()
