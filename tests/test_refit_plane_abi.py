"""The point-to-plane refit's C ABI without a GPU, in the manner of tests/test_refit_abi.py: the three entry points are exported,
declared and listed; the workspace follows the header's formula; argument errors (a negative or NaN r2, null pointers -- the
normals at the device tier among them --, bad sizes, a negative ldn, T_out aliasing T_dev, a workspace one byte short, steps < 1,
k out of range when the normals are to be computed) are PCREG_E_ARG before anything runs; a valid call without a device is
PCREG_E_NODEVICE.  A handle that holds rows needs a device, so ldn < M is asked of a stand-in: a block of memory whose every int32
is 100, which reads as M = 100 wherever the row count lies in it and is refused before any pointer in it is followed (the valid
call uses a block of zeros, M = 0, in the same way); tests/test_gpu_refit_plane.py asks it of real handles."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_refit_plane_workspace", "pcreg_dev_model_refit_plane_f32", "pcreg_model_refit_plane_f32")
MAXQ = 4 << 20
FORMULA = "131 328 + 2 roundup(12 S, 256) + 3 roundup(4 S, 256) + roundup(8 P, 256) + 2 roundup(4 P, 256) + roundup(224 P, 256) bytes"


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
    import inspect
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    from pcreg_amd.sweep import refine_trials
    assert callable(pc.Model.refit_plane) and callable(PreparedModel.refit_plane)
    assert inspect.signature(refine_trials).parameters["normals"].default is None
    sig = inspect.signature(pc.Model.refit_plane).parameters
    assert sig["steps"].default == 1 and sig["normals"].default is None and sig["k"].default == 6
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "plane_fit.hpp" in mk and os.path.exists(os.path.join(ROOT, "pcreg_amd", "csrc", "plane_fit.hpp"))


def test_workspace_follows_the_header_and_is_bounded():
    _, L = _lib()
    f, g = L.pcreg_dev_model_refit_plane_workspace, L.pcreg_dev_model_refit_workspace
    up = lambda x: (x + 255) // 256 * 256
    for Q, B in ((0, 0), (1, 1), (2500, 6), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        nb = max(1, min(B, MAXQ // max(Q, 1)))
        S, P = max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)
        want = 131_328 + 2 * up(12 * S) + 3 * up(4 * S) + up(8 * P) + 2 * up(4 * P) + up(224 * P)
        assert f(Q, B, 0) == f(Q, B, 1 << 20) == want == g(Q, B, 0) - up(216 * P) + up(224 * P) + up(4 * S) + up(4 * P), (Q, B)
    assert f(50_000, 107, 0) == f(50_000, 83, 0) == f(50_000, 1 << 20, 0)         # 83 transforms fill the 4 Mi slots
    assert f(-1, 1, 0) == 0 and f(1, -1, 0) == 0 and f(MAXQ + 1, 1, 0) == 0
    assert FORMULA in open(os.path.join(ROOT, "include", "pcreg.h")).read()


def _buffers():
    return dict(buf=np.zeros(64 * 3, np.float32), nrm=np.zeros(64 * 3, np.float32), T=np.zeros(3 * 16), To=np.zeros(3 * 16), Ts=np.zeros(3 * 16),
                n=np.zeros(3, np.int32), s=np.zeros(3), npl=np.zeros(3, np.int32), res=np.zeros(3), e=np.zeros(3, np.int32))


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    fake, big, E = 16, 1 << 40, _l.PCREG_E_ARG               # (the handle is never dereferenced: the checks refuse first)
    dev = lambda h=fake, q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, r2=1.0, nr=p(b["nrm"]), ldn=8, to=p(b["To"]), ts=None, nc=p(b["n"]), \
        sd=p(b["s"]), npl=p(b["npl"]), res=p(b["res"]), em=p(b["e"]), ws=p(b["buf"]), wsb=big: \
        L.pcreg_dev_model_refit_plane_f32(h, q, Q, ldq, t, B, r2, nr, ldn, to, ts, nc, sd, npl, res, em, ws, wsb, None)
    host = lambda h=fake, q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, r2=1.0, steps=1, nr=p(b["nrm"]), ldn=8, k=6, to=p(b["To"]), nc=p(b["n"]), \
        sd=p(b["s"]), npl=p(b["npl"]), res=p(b["res"]), em=p(b["e"]): \
        L.pcreg_model_refit_plane_f32(h, q, Q, ldq, t, B, r2, steps, nr, ldn, k, to, nc, sd, npl, res, em)
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert dev(r2=r2) == E and host(r2=r2) == E, r2
    assert b"bad argument" in L.pcreg_last_error()
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(to=None), dict(nc=None), dict(sd=None), dict(npl=None), dict(res=None), dict(em=None),
               dict(Q=-1), dict(B=-1), dict(ldq=3), dict(Q=MAXQ + 1, ldq=MAXQ + 1), dict(ldn=-1)):
        assert dev(**kw) == E and host(**kw) == E, kw
    rows100 = np.full(1024, 100, np.int32)                    # stands for a handle of 100 rows: see the module docstring
    assert dev(h=p(rows100), ldn=8) == E and b"bad argument" in L.pcreg_last_error()
    assert host(h=p(rows100), ldn=8) == E and b"bad argument" in L.pcreg_last_error()
    assert dev(ws=None) == E
    assert dev(nr=None) == E                                  # the device tier computes no normals
    assert dev(to=p(b["T"])) == E                             # T_out may not alias T_dev
    need = L.pcreg_dev_model_refit_plane_workspace(4, 3, 0)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    for steps in (0, -1, -(1 << 31)):
        assert host(steps=steps) == E and b"steps >= 1" in L.pcreg_last_error(), steps
    for k in (2, 33, 0, -1):                                  # normals NULL: k is pcreg_model_normals_f32's
        assert host(nr=None, k=k) == E, k


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    need = L.pcreg_dev_model_refit_plane_workspace(4, 3, 0)
    rows0 = np.zeros(1024, np.int32)                          # stands for a handle without rows: the entry reads M before the device
    for ts, r2 in ((None, 1.0), (p(b["Ts"]), float("inf")), (p(b["Ts"]), 0.0)):
        assert L.pcreg_dev_model_refit_plane_f32(p(rows0), p(b["buf"]), 4, 4, p(b["T"]), 3, r2, p(b["nrm"]), 1 << 30, p(b["To"]), ts,
                                                 p(b["n"]), p(b["s"]), p(b["npl"]), p(b["res"]), p(b["e"]), p(b["buf"]), need, None) \
            == _l.PCREG_E_NODEVICE
        assert b"no CPU fallback" in L.pcreg_last_error()
