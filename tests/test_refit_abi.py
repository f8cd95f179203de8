"""The transform refit's C ABI without a GPU: the three entry points are exported, declared and listed; the workspace follows the
header's formula; argument errors (a negative or NaN r2, null pointers, bad sizes, T_out aliasing T_dev, a workspace one byte short,
steps < 1 at the host tier) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_refit_workspace", "pcreg_dev_model_refit_f32", "pcreg_model_refit_f32")
MAXQ = 4 << 20


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
    from pcreg_amd.sweep import refine_trials
    assert callable(pc.Model.refit_transforms) and callable(PreparedModel.refit_transforms) and callable(refine_trials)
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "moments.hpp" in mk and os.path.exists(os.path.join(ROOT, "pcreg_amd", "csrc", "moments.hpp"))


def test_workspace_follows_the_header_and_is_bounded():
    _, L = _lib()
    f, g = L.pcreg_dev_model_refit_workspace, L.pcreg_dev_model_score_workspace
    up = lambda x: (x + 255) // 256 * 256
    for Q, B in ((0, 0), (1, 1), (2500, 6), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        nb = max(1, min(B, MAXQ // max(Q, 1)))
        S, P = max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)
        want = 131_328 + 2 * up(12 * S) + 2 * up(4 * S) + up(8 * P) + up(4 * P) + up(216 * P)
        assert f(Q, B, 0) == f(Q, B, 1 << 20) == want == g(Q, B, 0) + up(12 * S) + up(216 * P), (Q, B)
    assert f(50_000, 107, 0) == f(50_000, 83, 0) == f(50_000, 1 << 20, 0)         # 83 transforms fill the 4 Mi slots
    assert f(1, 1 << 30, 0) <= 131_328 + 260 * MAXQ
    assert f(-1, 1, 0) == 0 and f(1, -1, 0) == 0 and f(MAXQ + 1, 1, 0) == 0
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    assert "131 328 + 2 roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256) + roundup(216 P, 256) bytes" in head


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    T = np.zeros(3 * 16, np.float64)
    To = np.zeros(3 * 16, np.float64)
    n = np.zeros(3, np.int32)
    s = np.zeros(3, np.float64)
    e = np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data
    fake, big, E = 16, 1 << 40, _l.PCREG_E_ARG               # (the handle is never dereferenced: the checks refuse first)
    dev = lambda h=fake, q=p(buf), Q=4, ldq=4, t=p(T), B=3, r2=1.0, to=p(To), ts=None, nc=p(n), sd=p(s), em=p(e), ws=p(buf), wsb=big: \
        L.pcreg_dev_model_refit_f32(h, q, Q, ldq, t, B, r2, to, ts, nc, sd, em, ws, wsb, None)
    host = lambda h=fake, q=p(buf), Q=4, ldq=4, t=p(T), B=3, r2=1.0, steps=1, to=p(To), nc=p(n), sd=p(s), em=p(e): \
        L.pcreg_model_refit_f32(h, q, Q, ldq, t, B, r2, steps, to, nc, sd, em)
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert dev(r2=r2) == E and host(r2=r2) == E, r2
    assert b"bad argument" in L.pcreg_last_error()
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(to=None), dict(nc=None), dict(sd=None), dict(em=None), dict(Q=-1), dict(B=-1),
               dict(ldq=3), dict(Q=MAXQ + 1, ldq=MAXQ + 1)):
        assert dev(**kw) == E and host(**kw) == E, kw
    assert dev(ws=None) == E
    assert dev(to=p(T)) == E                                  # T_out may not alias T_dev
    need = L.pcreg_dev_model_refit_workspace(4, 3, 0)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    for steps in (0, -1, -(1 << 31)):
        assert host(steps=steps) == E and b"steps >= 1" in L.pcreg_last_error(), steps


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    buf = np.zeros(64 * 3, np.float32)
    T = np.zeros(3 * 16, np.float64)
    To = np.zeros(3 * 16, np.float64)
    Ts = np.zeros(3 * 16, np.float64)
    n = np.zeros(3, np.int32)
    s = np.zeros(3, np.float64)
    e = np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data
    need = L.pcreg_dev_model_refit_workspace(4, 3, 0)
    for ts, r2 in ((None, 1.0), (p(Ts), float("inf")), (p(Ts), 0.0)):
        assert L.pcreg_dev_model_refit_f32(16, p(buf), 4, 4, p(T), 3, r2, p(To), ts, p(n), p(s), p(e), p(buf), need, None) == _l.PCREG_E_NODEVICE
        assert b"no CPU fallback" in L.pcreg_last_error()
    import pcreg_amd as pc
    from pcreg_amd._lib import PcregError
    with pytest.raises(PcregError) as err:
        pc.Model(np.zeros((5, 3), np.float32))
    assert err.value.code == _l.PCREG_E_NODEVICE
