"""Timing of the point-to-plane refit against a prepared model: one JSON line.

scripts/refit_bench.py's protocol: the 50 k crop against 1 M model rows (bench.synth), scripts/score_bench.py's B = 107 candidate
transforms at r = 1.5, the routes alternating in one process after warm-up, a host clock around a stream synchronise.  The normals
are PreparedModel.normals(8), computed once before anything is timed.  Timed:
  plane      PreparedModel.refit_plane, one step
  point      PreparedModel.refit_transforms, one step (the point-to-point step on the same inputs)
  composed   the plane step as the entry points before it allow: PreparedModel.score_transforms(rows=True) for the [B][Q] rows, the
             moved points again (pcreg_dev_quick_tf_batched and a cast), the gather of the model rows and their normals, the
             residuals and the 6 x 6 normal equations in torch (float64, batched over B, no host synchronisation), torch.linalg.solve
plane and composed must agree on n_close, and their T_step within 1e-9 (tests/test_gpu_refit_plane.py's bound) wherever the
library fits and the composition's matrix is well conditioned.  No time is a pass criterion.

    python3 scripts/refit_plane_bench.py [--reps 25] [--warmup 3] [--B 107] [--routes plane,point,composed]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402
from score_bench import transforms  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def step_of(x, o):
    """T_step (16 numbers, the library's layout) of the solution x = (w, t) about the origin o: the contract's Cayley rotation"""
    h = x[:3] / 2.0
    S = np.sqrt(1.0 + h @ h)
    a, b, c, d = 1.0 / S, h[0] / S, h[1] / S, h[2] / S
    R = np.array([[1 - 2 * (c * c + d * d), 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), 1 - 2 * (b * b + d * d), 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), 1 - 2 * (b * b + c * c)]])
    T = np.zeros(16)
    for j in range(3):
        T[4 * j:4 * j + 3] = R[j]
        T[4 * j + 3] = o[j] + x[3 + j] - R[j] @ o
    T[15] = 1.0
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
    ap.add_argument("--routes", default="plane,point,composed", help="the routes to time, in the order of a round (the checks always run all three)")
    a = ap.parse_args()
    L, dev = lib(), torch.device("cuda", 0)
    model, surf, _ = synth(1_000_000, 50_000)
    surf = surf.astype(np.float32)
    Q, B = len(surf), a.B
    r2 = float(np.float32(1.5) * np.float32(1.5))
    T = transforms(surf, B)
    mt = torch.from_numpy(np.ascontiguousarray(model.T)).to(dev)
    pm = PreparedModel(mt)
    q = torch.from_numpy(np.ascontiguousarray(surf.T)).to(dev)
    Td = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(B, 16)).to(dev)
    nrm = pm.normals(8)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)

    out_plane = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B), f64(B), i32(B),
                 torch.empty(int(L.pcreg_dev_model_refit_plane_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev), None)
    plane = lambda: pm.refit_plane(q, Td, r2, nrm, out=out_plane)
    out_point = (f64(B, 16), f64(B, 16), i32(B), f64(B), i32(B),
                 torch.empty(int(L.pcreg_dev_model_refit_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev), None)
    point = lambda: pm.refit_transforms(q, Td, r2, out=out_point)

    ws = torch.empty(int(L.pcreg_dev_model_score_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev)
    out_rows = (i32(B), f64(B), i32(B, Q), torch.empty((B, Q), dtype=torch.float32, device=dev), ws)
    q64 = q.double()
    tf64 = f64(B, 3, Q)
    lo, hi = mt.min(dim=1).values, mt.max(dim=1).values
    o = (0.5 * lo + 0.5 * hi).double()                                     # the library's origin: the middle of the box, in fp32
    comp = {}

    def composed():
        n, _s, idx, _d = pm.score_transforms(q, Td, r2, rows=True, out=out_rows)
        check(L.pcreg_dev_quick_tf_batched(_p(q64), Q, Q, _p(Td), B, _p(tf64), Q, None, _stream()))
        p = tf64.float().double().permute(0, 2, 1)                         # [B, Q, 3]: rounded once to fp32, widened again
        row = idx.clamp(min=0).long()
        m = mt[:, row].double().permute(1, 2, 0)                           # the model row of every query (row 0 where none)
        nv = nrm[:, row].double().permute(1, 2, 0)
        ok = (idx >= 0) & torch.isfinite(nv).all(dim=2)
        nv = torch.where(ok[:, :, None], nv, torch.zeros((), dtype=torch.float64, device=dev))    # no plane: a zero row of J, r = 0
        r = ((p - m) * nv).sum(dim=2)
        J = torch.cat([torch.linalg.cross(p - o, nv), nv], dim=2)          # [B, Q, 6]
        A = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        sc = torch.sqrt(torch.diagonal(A, dim1=1, dim2=2)).clamp(min=1e-300)
        A_s = A / (sc[:, :, None] * sc[:, None, :]) + torch.diag_embed((sc <= 1e-300).double())   # (a transform without planes: the identity)
        comp["x"] = torch.linalg.solve(A_s, -g / sc) / sc
        comp["cond"] = torch.linalg.cond(A_s)
        comp["n"], comp["n_plane"] = n, ok.sum(dim=1, dtype=torch.int32)

    fns = {"plane": plane, "point": point, "composed": composed}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    fns = {k: fns[k] for k in a.routes.split(",")}
    torch.cuda.synchronize()
    n_new, npl_new, e_new = out_plane[2].cpu().numpy(), out_plane[4].cpu().numpy(), out_plane[6].cpu().numpy() != 0
    agree = bool(np.array_equal(n_new, comp["n"].cpu().numpy()) and np.array_equal(npl_new, comp["n_plane"].cpu().numpy())
                 and np.array_equal(n_new, out_point[2].cpu().numpy()))
    sums_same = bool(np.array_equal(out_plane[3].cpu().numpy().view(np.uint64), out_point[3].cpu().numpy().view(np.uint64)))
    x, cond, o_host = comp["x"].cpu().numpy(), comp["cond"].cpu().numpy(), o.cpu().numpy()
    step_new = out_plane[1].cpu().numpy()
    both = ~e_new & (cond < 1e4)
    diff = np.array([np.linalg.norm(step_new[b] - step_of(x[b], o_host)) for b in np.flatnonzero(both)]) if both.any() else np.zeros(1)
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"Q": Q, "M": pm.M, "B": B, "r": 1.5, "reps": a.reps, "counts_agree": agree, "sum_bits_equal_point_to_point": sums_same,
           "fitted": int((~e_new).sum()), "compared": int(both.sum()), "n_plane_min_max": [int(npl_new.min()), int(npl_new.max())],
           "T_step_max_difference": float(diff.max()), "routes": a.routes, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    pm.close()
    print(json.dumps(res))
    if not agree:
        raise SystemExit("the new call and the composition disagree on n_close or n_plane")
    if not diff.max() < 1e-9:
        raise SystemExit("the new call's T_step and the composition's differ by %g" % diff.max())


if __name__ == "__main__":
    main()
