"""The trimmed scoring and refits' C ABI without a GPU, in the manner of tests/test_refit_gicp_abi.py: the eight entry
points are exported, declared and listed, and the Python tiers take keep_ratio; the trimmed entries take the UNTRIMMED workspace, so
there is no new size function, and the four untrimmed ones still give the formula their layout comment documents
(tests/golden/workspace_sizes.json records other functions, not these, so the formula is restated here), which leaves the trim
its 1040 bytes a transform in blocks that are dead when it runs; argument errors (those of the untrimmed twins, and a
keep_ratio that is NaN, <= 0 or > 1) are PCREG_E_ARG before anything runs; a valid call without a device is PCREG_E_NODEVICE.
tests/trimabi/check_trim_header.c takes the entry points through the header from C and C++."""
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("score", "refit", "refit_plane", "refit_gicp")
NEW = tuple(n for k in KINDS for n in (f"pcreg_model_{k}_trimmed_f32", f"pcreg_dev_model_{k}_trimmed_f32"))
MAXQ = 4 << 20
BAD_RATIOS = (float("nan"), 0.0, -0.0, -0.5, 1.0 + 2.0 ** -52, 2.0, float("inf"), float("-inf"))


def _lib():
    from pcreg_amd import _lib
    return _lib, _lib.lib()


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def test_new_symbols_are_declared_exported_and_listed():
    _l, L = _lib()
    assert len(NEW) == 8
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in head, name
        assert name in _l.SYMBOLS, name
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel
    from pcreg_amd.sweep import refine_trials, score_trials
    for cls in (pc.Model, PreparedModel):
        for m in ("score_transforms", "refit_transforms", "refit_plane", "refit_gicp"):
            if (cls, m) == (PreparedModel, "refit_gicp"):         # (its parameter list is pinned by tests/test_refit_gicp_abi.py: a method of its own)
                assert list(inspect.signature(PreparedModel.refit_gicp_trimmed).parameters)[1:5] == ["q_soa", "T_dev", "r2", "keep_ratio"]
                continue
            sig = inspect.signature(getattr(cls, m)).parameters
            assert list(sig)[-1] == "keep_ratio" and sig["keep_ratio"].default is None, (cls, m)
    for f in (score_trials, refine_trials):
        sig = inspect.signature(f).parameters
        assert list(sig)[-1] == "keep_ratio" and sig["keep_ratio"].default is None, f
    mk = open(os.path.join(ROOT, "pcreg_amd", "csrc", "Makefile")).read()
    assert "knn_trim.hip" in mk and os.path.exists(os.path.join(ROOT, "pcreg_amd", "csrc", "knn_trim.hip"))


def _r(x):
    return (x + 255) // 256 * 256


def _layout(Q, B):
    """nb, S, P of the scoring chain's workspace (include/pcreg.h)"""
    nb = max(1, min(B, (4 << 20) // max(Q, 1)))
    return nb, max(nb * Q, 1), nb * max((Q + 2047) // 2048, 1)


def _untrimmed(kind, Q, B):
    """the documented formulas of the four untrimmed layouts (knn_score.hip's layout comment)"""
    _nb, S, P = _layout(Q, B)
    score = 131328 + _r(12 * S) + 2 * _r(4 * S) + _r(8 * P) + _r(4 * P)
    if kind == "score":
        return score
    if kind == "refit":
        return score + _r(12 * S) + _r(216 * P)
    return score + _r(12 * S) + _r(224 * P) + _r(4 * S) + _r(4 * P)


SHAPES = ((0, 0), (0, 5), (1, 1), (1, 300), (4, 3), (2048, 1), (2049, 1), (2500, 6), (2500, 8), (50_000, 107), (4 << 20, 5), (2049, 4000), (3, 4 << 20))


def test_untrimmed_workspaces_are_unchanged_and_there_is_no_trimmed_size_function():
    _l, L = _lib()
    head = open(os.path.join(ROOT, "include", "pcreg.h")).read()
    for kind in KINDS:
        old = getattr(L, f"pcreg_dev_model_{kind}_workspace")
        assert not hasattr(L, f"pcreg_dev_model_{kind}_trimmed_workspace") and f"{kind}_trimmed_workspace" not in head
        for Q, B in SHAPES:
            nb, S, P = _layout(Q, B)
            assert old(Q, B, 0) == old(Q, B, 1 << 20) == _untrimmed(kind, Q, B), (kind, Q, B)
            # what the trim works in: the larger of the cell counters and the slot -> query block holds 126 transforms' state or
            # the whole batch's, and the chunk counts hold the P tie counts
            assert max(131328, _r(4 * S)) // 1040 >= min(nb, 126)


def _buffers():
    return dict(buf=np.zeros(64 * 3, np.float32), nrm=np.zeros(64 * 3, np.float32), nq=np.zeros(64 * 3, np.float32), T=np.zeros(3 * 16),
                To=np.zeros(3 * 16), Ts=np.zeros(3 * 16), n=np.zeros(3, np.int32), s=np.zeros(3), npr=np.zeros(3, np.int32), res=np.zeros(3),
                e=np.zeros(3, np.int32), w=np.zeros(3, np.int32), cut=np.zeros(3, np.float32))


def _calls(L, b, fake=16, big=1 << 40):
    """the eight entries as functions of keyword overrides; the handle is never dereferenced where the checks refuse first"""
    p = lambda a: a.ctypes.data
    base = dict(h=fake, q=p(b["buf"]), Q=4, ldq=4, t=p(b["T"]), B=3, r2=1.0, kr=0.5, steps=1, nr=p(b["nrm"]), ldn=8, qn=p(b["nq"]), ldnq=4, k=6, eps=1e-3,
                to=p(b["To"]), ts=None, nc=p(b["n"]), sd=p(b["s"]), npr=p(b["npr"]), res=p(b["res"]), em=p(b["e"]), ws=p(b["buf"]), wsb=big,
                w=p(b["w"]), cut=p(b["cut"]))

    def make(f):
        return lambda **kw: f(**{**base, **kw})
    return dict(
        dev_score=make(lambda h, q, Q, ldq, t, B, r2, kr, nc, sd, ws, wsb, w, cut, **_: L.pcreg_dev_model_score_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, nc, sd, None, None, ws, wsb, None, w, cut)),
        dev_refit=make(lambda h, q, Q, ldq, t, B, r2, kr, to, ts, nc, sd, em, ws, wsb, w, cut, **_: L.pcreg_dev_model_refit_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, to, ts, nc, sd, em, ws, wsb, None, w, cut)),
        dev_plane=make(lambda h, q, Q, ldq, t, B, r2, kr, nr, ldn, to, ts, nc, sd, npr, res, em, ws, wsb, w, cut, **_: L.pcreg_dev_model_refit_plane_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, nr, ldn, to, ts, nc, sd, npr, res, em, ws, wsb, None, w, cut)),
        dev_gicp=make(lambda h, q, Q, ldq, t, B, r2, kr, nr, ldn, qn, ldnq, eps, to, ts, nc, sd, npr, res, em, ws, wsb, w, cut, **_:
                      L.pcreg_dev_model_refit_gicp_trimmed_f32(h, q, Q, ldq, t, B, r2, kr, nr, ldn, qn, ldnq, eps, to, ts, nc, sd, npr, res, em, ws, wsb,
                                                               None, w, cut)),
        host_score=make(lambda h, q, Q, ldq, t, B, r2, kr, nc, sd, w, cut, **_: L.pcreg_model_score_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, nc, sd, None, None, w, cut)),
        host_refit=make(lambda h, q, Q, ldq, t, B, r2, kr, steps, to, nc, sd, em, w, cut, **_: L.pcreg_model_refit_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, steps, to, nc, sd, em, w, cut)),
        host_plane=make(lambda h, q, Q, ldq, t, B, r2, kr, steps, nr, ldn, k, to, nc, sd, npr, res, em, w, cut, **_: L.pcreg_model_refit_plane_trimmed_f32(
            h, q, Q, ldq, t, B, r2, kr, steps, nr, ldn, k, to, nc, sd, npr, res, em, w, cut)),
        host_gicp=make(lambda h, q, Q, ldq, t, B, r2, kr, steps, nr, ldn, qn, ldnq, k, eps, to, nc, sd, npr, res, em, w, cut, **_:
                       L.pcreg_model_refit_gicp_trimmed_f32(h, q, Q, ldq, t, B, r2, kr, steps, nr, ldn, qn, ldnq, k, eps, to, nc, sd, npr, res, em, w, cut)))


def test_argument_errors_come_before_the_device():
    _l, L = _lib()
    b = _buffers()
    E = _l.PCREG_E_ARG
    calls = _calls(L, b)
    for name, f in calls.items():
        for kr in BAD_RATIOS:                                  # the new case
            assert f(kr=kr) == E, (name, kr)
            assert b"bad argument" in L.pcreg_last_error()
        for r2 in (-1.0, float("nan"), float("-inf")):         # ... and the untrimmed twins'
            assert f(r2=r2) == E, (name, r2)
        for kw in (dict(h=None), dict(q=None), dict(t=None), dict(nc=None), dict(sd=None), dict(Q=-1), dict(B=-1), dict(ldq=3),
                   dict(Q=MAXQ + 1, ldq=MAXQ + 1, ldnq=MAXQ + 1)):
            assert f(**kw) == E, (name, kw)
        if name.startswith("dev"):
            assert f(ws=None) == E, name
            kind = {"dev_score": "score", "dev_refit": "refit", "dev_plane": "refit_plane", "dev_gicp": "refit_gicp"}[name]
            need = getattr(L, f"pcreg_dev_model_{kind}_workspace")(4, 3, 0)
            assert f(wsb=need - 1) == E and b"bad argument" in L.pcreg_last_error(), name          # a workspace one byte short
        if "score" not in name:
            assert f(to=None) == E and f(em=None) == E, name
        if name.startswith("host") and "score" not in name:
            assert f(steps=0) == E and f(steps=-1) == E, name
        if name in ("dev_refit", "dev_plane", "dev_gicp"):
            assert f(to=b["T"].ctypes.data) == E, name         # T_out may not alias T_dev
        if "plane" in name or "gicp" in name:
            assert f(npr=None) == E and f(res=None) == E and f(ldn=-1) == E, name
        if "gicp" in name:
            assert f(eps=0.0) == E and f(eps=float("nan")) == E and f(ldnq=3) == E, name


def test_python_refuses_bad_ratios_before_the_library():
    from pcreg_amd.api import _Trim
    from pcreg_amd.device import _keep_ratio
    for kr in BAD_RATIOS:
        with pytest.raises(ValueError):
            _Trim(kr, 3)
        with pytest.raises(ValueError):
            _keep_ratio(kr)
    assert not _Trim(None, 3) and _Trim(1.0, 3) and _keep_ratio(1) == 1.0 and _keep_ratio(1e-6) == 1e-6
    t = _Trim(0.5, 0)
    assert t.into({})["n_within"].shape == (0,) and t.into({})["d2_cut"].dtype == np.float32


def test_valid_calls_report_no_device():
    _no_gpu()
    _l, L = _lib()
    b = _buffers()
    rows0 = np.zeros(1024, np.int32)                          # stands for a handle without rows: the entry reads M before the device
    calls = _calls(L, b, fake=rows0.ctypes.data)
    for name in ("dev_score", "dev_refit", "dev_plane", "dev_gicp"):
        kind = {"dev_score": "score", "dev_refit": "refit", "dev_plane": "refit_plane", "dev_gicp": "refit_gicp"}[name]
        need = getattr(L, f"pcreg_dev_model_{kind}_workspace")(4, 3, 0)                         # the untrimmed size is enough
        for kw in (dict(), dict(kr=1.0, r2=float("inf")), dict(kr=5e-324), dict(w=None, cut=None)):
            assert calls[name](wsb=need, ldn=1 << 30, ldnq=1 << 30, **kw) == _l.PCREG_E_NODEVICE, (name, kw)
            assert b"no CPU fallback" in L.pcreg_last_error()


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_header_declares_what_a_caller_would_write(lang, tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pcreg_amd", "libpcreg_hip.so")):
        g.build()
    exe = str(tmp_path / f"check_trim_header_{lang}")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-x", "c++", "-std=c++17"]
    subprocess.check_call(cc + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "trimabi", "check_trim_header.c"), "-o", exe, "-L" + os.path.join(ROOT, "pcreg_amd"),
                                "-lpcreg_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "pcreg_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "bad argument" in r.stdout, r.stdout + r.stderr
