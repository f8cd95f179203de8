"""The coherent-point-drift refit's C ABI without a GPU, in the manner of tests/test_refit_gicp_abi.py: the three entry points are
exported, declared and listed; the workspace function against the header's formula; argument errors (the siblings', an outlier
weight that is NaN or outside [0, 1), steps < 1, a short workspace) are PCREG_E_ARG before anything runs; a valid call without a
device is PCREG_E_NODEVICE.  The device entry reads the handle's row count for the workspace check, so a stand-in that holds a
row count is given wherever the checks get that far.  tests/cpdabi/check_cpd_header.c takes the entry points through the header
from C and C++."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcreg_dev_model_refit_cpd_workspace", "pcreg_dev_model_refit_cpd_f32", "pcreg_model_refit_cpd_f32")
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
    assert callable(pc.Model.refit_cpd) and callable(PreparedModel.refit_cpd)
    assert inspect.signature(refine_trials).parameters["cpd"].default is None
    sig = inspect.signature(pc.Model.refit_cpd).parameters
    assert sig["steps"].default == 1 and sig["sigma2"].default == 0.0 and sig["outlier"].default == 0.1
    sig = inspect.signature(PreparedModel.refit_cpd).parameters
    assert list(sig)[1:] == ["q_soa", "T_dev", "sigma2", "outlier", "steps", "out"] and sig["outlier"].default == 0.1
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "cpd_fit.hpp" in mk and "cpd.hip" in mk
    hdr = open(os.path.join(ROOT, "pcreg_amd", "csrc", "cpd_fit.hpp")).read()
    assert "fma(" not in hdr.split("#pragma once")[1] and "#include <hip" not in hdr           # plain C++: nothing fused, no HIP header


def roundup(x):
    return (x + 255) // 256 * 256


def formula(Q, B, M, score):
    """the size the header states at pcreg_dev_model_refit_cpd_workspace"""
    nb = max(1, min(B, 131072 // max(Q, 1)))
    S, P = max(nb * Q, 1), nb * max(-(-Q // 2048), 1)
    R = 256 * -(-max(-(-M // 256), 1) // 32)
    L = max(-(-M // R), 1)
    return (roundup(score) + roundup(4 * max(B * Q, 1)) + roundup(4 * max(B, 1)) + 256 + roundup(12 * S) + roundup(32 * P) + roundup(4 * P)
            + roundup(48 * nb) + roundup(20 * L * S) + roundup(152 * P))


def test_workspace_is_the_headers_formula():
    _, L = _lib()
    f, g = L.pcreg_dev_model_refit_cpd_workspace, L.pcreg_dev_model_score_workspace
    for Q, B, M in ((0, 0, 0), (1, 1, 1), (3, 2, 3), (2500, 6, 4096), (2500, 6, 4097), (2048, 1, 255), (2049, 107, 256), (5000, 107, 20_000),
                    (50_000, 107, 8193), (131_073, 3, 8449), (4 << 20, 2, 1000), (100, 4000, 65)):
        assert f(Q, B, M) == formula(Q, B, M, g(Q, B, M)) > 0, (Q, B, M)
    assert f(-1, 1, 1) == 0 and f(1, -1, 1) == 0 and f(1, 1, -1) == 0 and f(MAXQ + 1, 1, 1) == 0


def _buffers():
    return dict(buf=np.zeros(64 * 3, np.float32), T=np.zeros(3 * 16), sg=np.zeros(3), To=np.zeros(3 * 16), Ts=np.zeros(3 * 16), so=np.zeros(3),
                Np=np.zeros(3), res=np.zeros(3), s=np.zeros(3), n=np.zeros(3, np.int32), e=np.zeros(3, np.int32))


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    rows100 = np.full(1024, 100, np.int32)                    # stands for a handle of 100 rows: only its row count is read
    big, E = 1 << 40, _l.PCREG_E_ARG
    dev = lambda h=p(rows100), q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, sg=p(b["sg"]), w=0.1, to=p(b["To"]), ts=None, so=p(b["so"]), \
        Np=p(b["Np"]), res=p(b["res"]), sd=p(b["s"]), nl=p(b["n"]), em=p(b["e"]), ws=p(b["buf"]), wsb=big: \
        L.pcreg_dev_model_refit_cpd_f32(h, q, Q, ldq, t, B, sg, w, to, ts, so, Np, res, sd, nl, em, ws, wsb, None)
    host = lambda h=p(rows100), q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, sg=p(b["sg"]), w=0.1, steps=1, to=p(b["To"]), so=p(b["so"]), \
        Np=p(b["Np"]), res=p(b["res"]), sd=p(b["s"]), nl=p(b["n"]), em=p(b["e"]): \
        L.pcreg_model_refit_cpd_f32(h, q, Q, ldq, t, B, sg, w, steps, to, so, Np, res, sd, nl, em)
    for w in (float("nan"), -1e-9, 1.0, 1.5, float("inf"), float("-inf")):
        assert dev(w=w) == E and host(w=w) == E, w
        assert b"outlier" in L.pcreg_last_error()
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(sg=None), dict(to=None), dict(so=None), dict(Np=None), dict(res=None), dict(sd=None),
               dict(nl=None), dict(em=None), dict(Q=-1), dict(B=-1), dict(ldq=3), dict(Q=MAXQ + 1, ldq=MAXQ + 1)):
        assert dev(**kw) == E and host(**kw) == E, kw
        assert b"bad argument" in L.pcreg_last_error()
    assert dev(ws=None) == E
    assert dev(to=p(b["T"])) == E                             # T_out may not alias T_dev
    need = L.pcreg_dev_model_refit_cpd_workspace(4, 3, 100)
    assert dev(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error()
    for steps in (0, -1, -(1 << 31)):
        assert host(steps=steps) == E and b"steps >= 1" in L.pcreg_last_error(), steps


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    b = _buffers()
    p = lambda a: a.ctypes.data
    rows0 = np.zeros(1024, np.int32)                          # stands for a handle without rows: the entry reads M before the device
    need = L.pcreg_dev_model_refit_cpd_workspace(4, 3, 0)
    for ts, w in ((None, 0.1), (p(b["Ts"]), 0.0), (p(b["Ts"]), 1.0 - 2.0 ** -53)):
        assert L.pcreg_dev_model_refit_cpd_f32(p(rows0), p(b["buf"]), 4, 4, p(b["T"]), 3, p(b["sg"]), w, p(b["To"]), ts, p(b["so"]), p(b["Np"]),
                                               p(b["res"]), p(b["s"]), p(b["n"]), p(b["e"]), p(b["buf"]), need, None) == _l.PCREG_E_NODEVICE
        assert b"no CPU fallback" in L.pcreg_last_error()


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_header_declares_what_a_caller_would_write(lang, tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    exe = str(tmp_path / f"check_cpd_header_{lang}")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-x", "c++", "-std=c++17"]
    subprocess.check_call(cc + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "cpdabi", "check_cpd_header.c"), "-o", exe, "-L" + os.path.join(ROOT, "pcreg_amd"),
                                "-lpcreg_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "bad argument" in r.stdout, r.stdout + r.stderr
