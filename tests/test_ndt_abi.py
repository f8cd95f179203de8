"""The NDT's C ABI without a GPU: the entry points are exported, declared and listed; the step's workspace is the one formula
the header states; the argument errors of the table's creation (a step that is not finite or not positive, min_points < 3, ld < n,
a negative n, null pointers) and a NULL handle anywhere are PCREG_E_ARG before anything runs; a valid creation without a device is
PCREG_E_NODEVICE; the Python tiers refuse what the library would."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_ndt_create", "pcreg_ndt_destroy", "pcreg_ndt_size", "pcreg_ndt_get", "pcreg_ndt_refit_f32", "pcreg_dev_ndt_create",
       "pcreg_dev_ndt_destroy", "pcreg_dev_ndt_size", "pcreg_dev_ndt_get", "pcreg_dev_ndt_refit_workspace", "pcreg_dev_ndt_refit_f32")


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
    assert "NdtModel" in pc.__all__ and all(hasattr(pc.NdtModel, m) for m in ("gaussians", "refit", "close"))
    from pcreg_amd import device, sweep
    assert all(hasattr(device.NdtModel, m) for m in ("gaussians", "refit", "close"))
    assert "ndt" in sweep.refine_trials.__code__.co_varnames
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "ndt.hip" in mk.split("SRCS")[1].split("\n")[0] and "ndt_gauss.hpp" in mk


def _roundup(x, a=256):
    return -(-x // a) * a


def test_workspace_is_the_stated_formula():
    _, L = _lib()
    f = L.pcreg_dev_ndt_refit_workspace
    for Q, B in ((0, 0), (0, 5), (1, 1), (2047, 3), (2048, 3), (2049, 3), (50_000, 107), (4 << 20, 1), (5, 100_000)):
        P = B * max(-(-Q // 2048), 1)
        assert f(Q, B) == _roundup(224 * P) + _roundup(4 * P), (Q, B)
    assert f(-1, 1) == 0 and f(1, -1) == 0 and f((4 << 20) + 1, 1) == 0


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    pts = np.zeros(64 * 3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    E = _l.PCREG_E_ARG
    host = lambda **k: L.pcreg_ndt_create(*[k.get(a, d) for a, d in (("pts", p(pts)), ("n", 8), ("ld", 8), ("step", 0.5), ("min_points", 6), ("out", C.byref(h)))])
    dev = lambda **k: L.pcreg_dev_ndt_create(*[k.get(a, d) for a, d in (("pts", C.c_void_p(16)), ("n", 8), ("ld", 8), ("step", 0.5), ("min_points", 6),
                                                                         ("stream", None), ("out", C.byref(h)))])
    for call in (host, dev):
        for step in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(step=step) == E, step
        assert b"bad argument" in L.pcreg_last_error()
        for k in (dict(ld=7), dict(n=-1), dict(pts=None), dict(min_points=2), dict(min_points=0), dict(out=None)):
            assert call(**k) == E, k
    assert not h.value
    fake, nv = C.c_void_p(16), C.c_int(-5)
    for fn in (L.pcreg_ndt_size, L.pcreg_dev_ndt_size):
        assert fn(None, C.byref(nv), C.byref(nv)) == E
    for fn in (L.pcreg_ndt_get, L.pcreg_dev_ndt_get):
        assert fn(None, fake, fake, fake, fake, fake, fake) == E
    assert L.pcreg_ndt_refit_f32(None, fake, 8, 8, fake, 1, 1, 0.55, 1, fake, fake, fake, fake) == E
    assert L.pcreg_dev_ndt_refit_f32(None, fake, 8, 8, fake, 1, 1, 0.55, fake, fake, fake, fake, fake, fake, C.c_size_t(1 << 20), None) == E
    assert L.pcreg_ndt_destroy(None) == 0 and L.pcreg_dev_ndt_destroy(None) == 0
    assert nv.value == -5                             # nothing was written


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    pts = np.zeros(64 * 3, np.float32)
    h = C.c_void_p()
    assert L.pcreg_ndt_create(pts.ctypes.data_as(C.c_void_p), 8, 9, 0.5, 6, C.byref(h)) == _l.PCREG_E_NODEVICE and not h.value
    assert b"no CPU fallback" in L.pcreg_last_error()
    assert L.pcreg_ndt_create(None, 0, 0, 0.5, 3, C.byref(h)) == _l.PCREG_E_NODEVICE
    assert L.pcreg_dev_ndt_create(C.c_void_p(16), 8, 8, 0.5, 6, None, C.byref(h)) == _l.PCREG_E_NODEVICE
    with pytest.raises(PcregError) as e:
        pc.NdtModel(np.ones((7, 3)), 0.5)
    assert e.value.code == _l.PCREG_E_NODEVICE


def test_the_python_tier_refuses_what_the_library_would():
    import pcreg_amd as pc
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.NdtModel(np.ones((7, 3)), bad)
    with pytest.raises(ValueError):
        pc.NdtModel(np.ones((7, 2)), 0.5)
    with pytest.raises(ValueError):
        pc.NdtModel(np.ones((7, 3)), 0.5, min_points=2)
