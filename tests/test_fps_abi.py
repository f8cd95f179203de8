"""The farthest point sampling's C ABI without a GPU, in the manner of tests/test_cpd_abi.py: the four entry points are exported,
declared and listed, and the Python methods exist with the contract's defaults; the workspace function against the header's
formula; every argument error of the contract is PCREG_E_ARG before anything runs; a valid call without a device is
PCREG_E_NODEVICE.  The handle entries read the handle's row count for the checks, so a stand-in that holds a row count is given
wherever the checks get that far.  tests/fpsabi/check_fps_header.c takes the entry points through the header from C and C++."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_fps_workspace", "pcreg_dev_model_fps_f32", "pcreg_model_fps_f32", "pcreg_point_fps_f32")
CAP = 1 << 21


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
    for name in NEW + ("pcreg_debug_fps_stats",):
        assert hasattr(L, name), name
        assert name + "(" in head, name
        assert name in _l.SYMBOLS, name
    assert "#define PCREG_FPS_MAX_ROWS 2097152" in head
    import inspect
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    for fn, names in ((pc.Model.farthest_points, ["self", "K", "start", "stop_d2"]), (pc.point_farthest_points, ["pts", "K", "start", "stop_d2"]),
                      (PreparedModel.farthest_points, ["self", "K", "start", "stop_d2", "out"])):
        sig = inspect.signature(fn).parameters
        assert list(sig) == names and sig["start"].default == -1 and sig["stop_d2"].default == 0.0, fn
        assert sig["K"].default is inspect.Parameter.empty
    assert inspect.signature(PreparedModel.farthest_points).parameters["out"].default is None
    assert "point_farthest_points" in pc.__all__
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "knn_fps.hip" in mk


def roundup(x):
    return (x + 255) // 256 * 256


def formula(M):
    """the size the header states at pcreg_dev_model_fps_workspace"""
    R, U = max(M, 1), 8 * max(-(-M // 512), 1)
    return 2 * roundup(4 * R) + roundup(16 * U) + 256


def test_workspace_is_the_headers_formula():
    _, L = _lib()
    f = L.pcreg_dev_model_fps_workspace
    for M in (0, 1, 63, 64, 65, 511, 512, 513, 1025, 5000, 600_000, CAP - 1, CAP):
        for K in (0, 1, 63, 64, 65, 511, 512, 513, CAP, CAP + 1):
            assert f(M, K) == formula(M) > 0, (M, K)
    for K in (0, 1, 512):
        assert f(CAP + 1, K) == 0 and f(-1, K) == 0 and f((1 << 31) - 1, K) == 0          # refused: no size


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    p = lambda a: a.ctypes.data
    rows100 = np.full(1024, 100, np.int32)                    # stands for a handle of 100 rows: only its row count is read
    rows0 = np.zeros(1024, np.int32)
    rows_big = np.full(1024, CAP + 1, np.int32)
    b = dict(idx=np.zeros(8, np.int32), dist=np.zeros(8, np.float32), n=np.zeros(1, np.int32), cov=np.zeros(1, np.float32),
             md=np.zeros(128, np.float32), lab=np.zeros(128, np.int32), info=np.zeros(1, np.int32), m=np.zeros(300, np.float32))
    big, E = 1 << 40, _l.PCREG_E_ARG
    dev = lambda h=p(rows100), K=8, start=-1, stop=0.0, n=p(b["n"]), ws=p(b["m"]), wsb=big: \
        L.pcreg_dev_model_fps_f32(h, K, start, stop, p(b["idx"]), p(b["dist"]), n, p(b["cov"]), p(b["md"]), p(b["lab"]), p(b["info"]), ws, wsb, None)
    host = lambda h=p(rows100), K=8, start=-1, stop=0.0, n=p(b["n"]): \
        L.pcreg_model_fps_f32(h, K, start, stop, p(b["idx"]), p(b["dist"]), n, p(b["cov"]), p(b["md"]), p(b["lab"]))
    point = lambda m=p(b["m"]), M=100, ldm=100, K=8, start=-1, stop=0.0, n=p(b["n"]): \
        L.pcreg_point_fps_f32(m, M, ldm, K, start, stop, p(b["idx"]), p(b["dist"]), n, p(b["cov"]), p(b["md"]), p(b["lab"]))
    for kw in (dict(K=-1), dict(start=-2), dict(start=100), dict(start=1 << 30), dict(stop=-1e-30), dict(stop=float("nan")),
               dict(stop=float("-inf")), dict(n=None)):
        assert dev(**kw) == E and host(**kw) == E and point(**kw) == E, kw
        assert b"bad argument" in L.pcreg_last_error()
    assert dev(h=None) == E and host(h=None) == E and point(m=None) == E
    assert dev(h=p(rows_big)) == E and host(h=p(rows_big)) == E and point(M=CAP + 1, ldm=CAP + 1) == E        # above the documented cap
    assert point(M=-1) == E and point(ldm=99) == E
    assert dev(ws=None) == E
    need = L.pcreg_dev_model_fps_workspace(100, 8)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    # M = 0: any start is allowed; the call gets as far as the device
    if not __import__("torch").cuda.is_available():
        assert dev(h=p(rows0), start=55) == _l.PCREG_E_NODEVICE


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    p = lambda a: a.ctypes.data
    rows100 = np.full(1024, 100, np.int32)
    n, ws = np.zeros(1, np.int32), np.zeros(4096, np.uint8)
    m = np.zeros(300, np.float32)
    need = L.pcreg_dev_model_fps_workspace(100, 8)
    assert need <= ws.nbytes
    for start, stop in ((-1, 0.0), (0, float("inf")), (99, 2.5)):
        assert L.pcreg_dev_model_fps_f32(p(rows100), 8, start, stop, None, None, p(n), None, None, None, None, p(ws), need, None) == _l.PCREG_E_NODEVICE
        assert b"no CPU fallback" in L.pcreg_last_error()
        assert L.pcreg_model_fps_f32(p(rows100), 8, start, stop, None, None, p(n), None, None, None) == _l.PCREG_E_NODEVICE
        assert L.pcreg_point_fps_f32(p(m), 100, 100, 8, start, stop, None, None, p(n), None, None, None) == _l.PCREG_E_NODEVICE
    assert L.pcreg_point_fps_f32(None, 0, 0, 0, 7, 0.0, None, None, p(n), None, None, None) == _l.PCREG_E_NODEVICE


def test_python_argument_errors():
    import pcreg_amd as pc
    pts = np.zeros((10, 3), np.float32)
    for kw in (dict(K=-1), dict(K=2, start=10), dict(K=2, start=-2), dict(K=2, stop_d2=-1.0), dict(K=2, stop_d2=float("nan"))):
        with pytest.raises(ValueError):
            pc.point_farthest_points(pts, **kw)
    with pytest.raises(ValueError):
        pc.point_farthest_points(np.zeros((10, 2), np.float32), 2)


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_header_declares_what_a_caller_would_write(lang, tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    exe = str(tmp_path / f"check_fps_header_{lang}")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-x", "c++", "-std=c++17"]
    subprocess.check_call(cc + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "fpsabi", "check_fps_header.c"), "-o", exe, "-L" + os.path.join(ROOT, "pcreg_amd"),
                                "-lpcreg_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "bad argument" in r.stdout, r.stdout + r.stderr
