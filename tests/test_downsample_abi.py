"""The downsampling's C ABI without a GPU: the entry points are exported, declared and listed; the workspace is the one formula
the header states; every argument error (a step that is not finite or not positive, ld < n, ldo < n, a negative n, null pointers,
a short workspace) is PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_downsample_grid_f32", "pcreg_dev_downsample_grid_workspace", "pcreg_dev_downsample_grid_chunk", "pcreg_dev_downsample_grid_f32")


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
    assert "pcdownsample" in pc.__all__ and callable(pc.pcdownsample)
    from pcreg_amd import device
    assert callable(device.downsample_grid) and "PreparedModel(" in device.downsample_grid.__doc__
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "downsample.hip" in mk.split("SRCS")[1].split("\n")[0]


def _roundup(x, a=256):
    return -(-x // a) * a


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_downsample_grid_workspace
    assert L.pcreg_dev_downsample_grid_chunk() == 2048
    for n in (0, 1, 63, 2047, 2048, 2049, 4097, 200_000, 10_000_000, (1 << 31) - 1 - 2048):
        nn = max(n, 1)
        chunks = -(-nn // 2048)
        want = (256 + _roundup(24 * chunks) + _roundup(4 * chunks) + 2 * (_roundup(8 * nn) + _roundup(4 * nn)) + _roundup(1024 * chunks) + 1024
                + _roundup(4 * chunks) + _roundup(4 * nn))
        assert f(n) == want, n


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 3, np.float32)
    cnt = np.zeros(64, np.int32); lab = np.zeros(64, np.int32)
    no = C.c_int(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)                             # never dereferenced: the checks refuse first
    big = C.c_size_t(1 << 30)
    E = _l.PCREG_E_ARG
    host = lambda **k: L.pcreg_downsample_grid_f32(*[k.get(a, d) for a, d in (("pts", p(pts)), ("n", 8), ("ld", 8), ("step", 0.5), ("out", p(out)),
                                                                               ("ldo", 8), ("count", p(cnt)), ("label", p(lab)), ("n_out", C.byref(no)))])
    dev = lambda **k: L.pcreg_dev_downsample_grid_f32(*[k.get(a, d) for a, d in (("pts", fake), ("n", 8), ("ld", 8), ("step", 0.5), ("out", fake),
                                                                                  ("ldo", 8), ("count", fake), ("label", fake), ("n_out", fake), ("info", fake),
                                                                                  ("ws", fake), ("wsb", big), ("stream", None))])
    for call in (host, dev):
        for step in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(step=step) == E, step
        assert b"bad argument" in L.pcreg_last_error()
        assert call(ld=7) == E
        assert call(ldo=7) == E
        assert call(n=-1) == E
        assert call(pts=None) == E
        assert call(out=None) == E
        assert call(n_out=None) == E
    assert dev(info=None) == E
    assert dev(ws=None) == E
    assert dev(wsb=C.c_size_t(L.pcreg_dev_downsample_grid_workspace(8) - 1)) == E
    assert no.value == -5                             # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    out = np.zeros(64 * 3, np.float32)
    no = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pcreg_downsample_grid_f32(p(pts), 8, 9, 0.5, p(out), 10, None, None, C.byref(no)) == _l.PCREG_E_NODEVICE
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_downsample_grid_f32(None, 0, 0, 0.5, None, 0, None, None, C.byref(no)) == _l.PCREG_E_NODEVICE
    fake = C.c_void_p(16)
    assert L.pcreg_dev_downsample_grid_f32(fake, 8, 8, 0.5, fake, 8, None, None, fake, fake, fake, C.c_size_t(1 << 30), None) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.pcdownsample(np.ones((7, 3)), 0.5)
    assert e.value.code == _l.PCREG_E_NODEVICE
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.pcdownsample(np.ones((7, 3)), bad)
    with pytest.raises(ValueError):
        pc.pcdownsample(np.ones((7, 2)), 0.5)
