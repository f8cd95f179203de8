"""The plane-to-plane refit's C ABI without a GPU, in the manner of tests/test_refit_plane_abi.py: the three entry points are
exported, declared and listed; the workspace is the plane refit's; argument errors (those of the plane refit, and ldnq < Q, null
query normals at the device tier, an epsilon that is NaN or outside (0, 1]) are PCREG_E_ARG before anything runs; a valid call
without a device is PCREG_E_NODEVICE.  A handle that holds rows needs a device, so ldn < M is asked of a stand-in as
tests/test_refit_plane_abi.py does.  tests/gicpabi/check_gicp_header.c takes the entry points through the header from C and C++."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_refit_gicp_workspace", "pcreg_dev_model_refit_gicp_f32", "pcreg_model_refit_gicp_f32")
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
    import inspect
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    from pcreg_amd.sweep import refine_trials
    assert callable(pc.Model.refit_gicp) and callable(PreparedModel.refit_gicp)
    sig = inspect.signature(refine_trials).parameters
    assert sig["surface_normals"].default is None and sig["epsilon"].default == 1e-3 and sig["normals"].default is None
    sig = inspect.signature(pc.Model.refit_gicp).parameters
    assert sig["steps"].default == 1 and sig["normals"].default is None and sig["query_normals"].default is None and sig["epsilon"].default == 1e-3
    sig = inspect.signature(PreparedModel.refit_gicp).parameters
    assert list(sig)[1:] == ["q_soa", "T_dev", "r2", "normals", "q_normals", "epsilon", "steps", "out"] and sig["epsilon"].default == 1e-3
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "gicp_pair.hpp" in mk and os.path.exists(os.path.join(ROOT, "pcreg_amd", "csrc", "gicp_pair.hpp"))
    hdr = open(os.path.join(ROOT, "pcreg_amd", "csrc", "gicp_pair.hpp")).read()
    assert "fma(" not in hdr.split("#pragma once")[1] and "#include <hip" not in hdr           # plain C++: nothing fused, no HIP header


def test_workspace_is_the_plane_refits():
    _, L = _lib()
    f, g = L.pcreg_dev_model_refit_gicp_workspace, L.pcreg_dev_model_refit_plane_workspace
    for Q, B in ((0, 0), (1, 1), (2500, 6), (50_000, 107), (4 << 20, 5), (2049, 4000)):
        assert f(Q, B, 0) == f(Q, B, 1 << 20) == g(Q, B, 0) > 0, (Q, B)
    assert f(-1, 1, 0) == 0 and f(1, -1, 0) == 0 and f(MAXQ + 1, 1, 0) == 0


def _buffers():
    return dict(buf=np.zeros(64 * 3, np.float32), nrm=np.zeros(64 * 3, np.float32), nq=np.zeros(64 * 3, np.float32), T=np.zeros(3 * 16),
                To=np.zeros(3 * 16), Ts=np.zeros(3 * 16), n=np.zeros(3, np.int32), s=np.zeros(3), npr=np.zeros(3, np.int32), res=np.zeros(3),
                e=np.zeros(3, np.int32))


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    fake, big, E = 16, 1 << 40, _l.PCREG_E_ARG               # (the handle is never dereferenced: the checks refuse first)
    dev = lambda h=fake, q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, r2=1.0, nr=p(b["nrm"]), ldn=8, qn=p(b["nq"]), ldnq=4, eps=1e-3, to=p(b["To"]), \
        ts=None, nc=p(b["n"]), sd=p(b["s"]), npr=p(b["npr"]), res=p(b["res"]), em=p(b["e"]), ws=p(b["buf"]), wsb=big: \
        L.pcreg_dev_model_refit_gicp_f32(h, q, Q, ldq, t, B, r2, nr, ldn, qn, ldnq, eps, to, ts, nc, sd, npr, res, em, ws, wsb, None)
    host = lambda h=fake, q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, r2=1.0, steps=1, nr=p(b["nrm"]), ldn=8, qn=p(b["nq"]), ldnq=4, k=6, eps=1e-3, \
        to=p(b["To"]), nc=p(b["n"]), sd=p(b["s"]), npr=p(b["npr"]), res=p(b["res"]), em=p(b["e"]): \
        L.pcreg_model_refit_gicp_f32(h, q, Q, ldq, t, B, r2, steps, nr, ldn, qn, ldnq, k, eps, to, nc, sd, npr, res, em)
    for r2 in (-1.0, float("nan"), -0.5, float("-inf")):
        assert dev(r2=r2) == E and host(r2=r2) == E, r2
    assert b"bad argument" in L.pcreg_last_error()
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(to=None), dict(nc=None), dict(sd=None), dict(npr=None), dict(res=None), dict(em=None),
               dict(Q=-1), dict(B=-1), dict(ldq=3), dict(Q=MAXQ + 1, ldq=MAXQ + 1, ldnq=MAXQ + 1), dict(ldn=-1), dict(ldnq=3), dict(ldnq=-1)):
        assert dev(**kw) == E and host(**kw) == E, kw
    for eps in (float("nan"), 0.0, -1e-3, 1.0 + 2.0 ** -52, 2.0, float("inf"), float("-inf")):
        assert dev(eps=eps) == E and host(eps=eps) == E, eps
        assert b"epsilon" in L.pcreg_last_error()
    rows100 = np.full(1024, 100, np.int32)                    # stands for a handle of 100 rows
    assert dev(h=p(rows100), ldn=8) == E and b"bad argument" in L.pcreg_last_error()
    assert host(h=p(rows100), ldn=8) == E and b"bad argument" in L.pcreg_last_error()
    assert dev(ws=None) == E
    assert dev(nr=None) == E and dev(qn=None) == E            # the device tier computes no normals
    assert dev(to=p(b["T"])) == E                             # T_out may not alias T_dev
    need = L.pcreg_dev_model_refit_gicp_workspace(4, 3, 0)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    for steps in (0, -1, -(1 << 31)):
        assert host(steps=steps) == E and b"steps >= 1" in L.pcreg_last_error(), steps
    for k in (2, 33, 0, -1):                                  # either set NULL: k is pcreg_model_normals_f32's
        assert host(nr=None, k=k) == E and host(qn=None, k=k) == E and host(nr=None, qn=None, k=k) == E, k


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    need = L.pcreg_dev_model_refit_gicp_workspace(4, 3, 0)
    rows0 = np.zeros(1024, np.int32)                          # stands for a handle without rows: the entry reads M before the device
    for ts, r2, eps in ((None, 1.0, 1e-3), (p(b["Ts"]), float("inf"), 1.0), (p(b["Ts"]), 0.0, 5e-324)):
        assert L.pcreg_dev_model_refit_gicp_f32(p(rows0), p(b["buf"]), 4, 4, p(b["T"]), 3, r2, p(b["nrm"]), 1 << 30, p(b["nq"]), 1 << 30, eps,
                                                p(b["To"]), ts, p(b["n"]), p(b["s"]), p(b["npr"]), p(b["res"]), p(b["e"]), p(b["buf"]), need, None) \
            == _l.PCREG_E_NODEVICE
        assert b"no CPU fallback" in L.pcreg_last_error()


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_header_declares_what_a_caller_would_write(lang, tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    exe = str(tmp_path / f"check_gicp_header_{lang}")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-x", "c++", "-std=c++17"]
    subprocess.check_call(cc + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "gicpabi", "check_gicp_header.c"), "-o", exe, "-L" + os.path.join(ROOT, "pcreg_amd"),
                                "-lpcreg_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "bad argument" in r.stdout, r.stdout + r.stderr
