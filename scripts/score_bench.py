"""Timing of the transform scoring against a prepared model: one JSON line.

The sweep's shape: a 50 k crop against 1 M model rows (bench.synth), B = 107 candidate transforms -- the true motion, 10 within
one unit of it and 96 random rigid motions about the crop's middle -- at r = 1.5 (the reference's maxDist).  Timed, alternately
in one process after warm-up, with a host clock around a stream synchronise:
  score_sums / score_rows   PreparedModel.score_transforms, counts and sums only / with the [B][Q] rows and distances
  composed                  what the entry points before it allow: pcreg_dev_quick_tf_batched (B fp64 copies), a cast, B top-2
                            searches (pcreg_dev_model_search_f32), torch reductions over the first column capped at r2
Both must agree on n_close.  Reported: median, min and max of each, the composition's repeat-to-repeat spread, and the share of
(query block, tile) pairs the scoring walk lists ("knn_stats").

    python3 scripts/score_bench.py [--reps 20] [--warmup 3] [--B 107]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import BBOX, eul2rotm_zyx, synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def transforms(surf, B, seed=3):
    """[B, 4, 4], used as [q, 1] * T: the inverse of bench.synth's motion, 10 of it shifted by up to one unit, the rest random
    rotations about the crop's middle shifted by up to 30 units"""
    rng = np.random.default_rng(seed)
    centre = BBOX * np.array([0.45, 0.55, 0.5])
    R = eul2rotm_zyx([0.010, -0.008, 0.012]).astype(np.float64)
    t = np.array([0.15, -0.10, 0.20])
    true = np.eye(4)
    true[:3, :3] = R.T
    true[3, :3] = centre - (centre + t) @ R.T
    T = [true]
    for _ in range(min(10, B - 1)):
        d = rng.normal(size=3)
        near = true.copy()
        near[3, :3] += d / np.linalg.norm(d) * rng.uniform(0.1, 1.0)
        T.append(near)
    mid = surf.astype(np.float64).mean(axis=0)
    while len(T) < B:
        Rr = _rot(rng)
        wrong = np.eye(4)
        wrong[:3, :3] = Rr
        wrong[3, :3] = mid - mid @ Rr + rng.uniform(-30, 30, 3)
        T.append(wrong)
    return np.stack(T[:B])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=107)
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

    # the new call, with buffers of its own
    ws = torch.empty(int(L.pcreg_dev_model_score_workspace(Q, B, pm.M)), dtype=torch.uint8, device=dev)
    out_sums = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev), None, None, ws)
    out_rows = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev),
                torch.empty((B, Q), dtype=torch.int32, device=dev), torch.empty((B, Q), dtype=torch.float32, device=dev), ws)
    score_sums = lambda: pm.score_transforms(q, Td, r2, out=out_sums)
    score_rows = lambda: pm.score_transforms(q, Td, r2, rows=True, out=out_rows)

    # the composition
    q64 = q.double()
    tf64 = torch.empty((B, 3, Q), dtype=torch.float64, device=dev)
    idx2 = torch.empty((B, Q, 2), dtype=torch.int32, device=dev)
    dist2 = torch.empty((B, Q, 2), dtype=torch.float32, device=dev)
    ws2 = torch.empty(int(L.pcreg_dev_model_search_workspace(Q, pm.M)), dtype=torch.uint8, device=dev)
    comp = {}

    def composed():
        check(L.pcreg_dev_quick_tf_batched(_p(q64), Q, Q, _p(Td), B, _p(tf64), Q, None, _stream()))
        tf32 = tf64.float()
        for b in range(B):
            check(L.pcreg_dev_model_search_f32(pm.handle, _p(tf32[b]), Q, Q, C.c_int32(0), _p(idx2[b]), _p(dist2[b]), _p(ws2),
                                               C.c_size_t(ws2.numel()), _stream()))
        d1 = dist2[:, :, 0]
        hit = d1 <= r2
        comp["n_close"] = hit.sum(dim=1, dtype=torch.int32)
        comp["sum_d2"] = torch.where(hit, d1.double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(dim=1)

    fns = {"composed": composed, "score_sums": score_sums, "score_rows": score_rows}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    n_new, n_rows, n_comp = out_sums[0].cpu().numpy(), out_rows[0].cpu().numpy(), comp["n_close"].cpu().numpy()
    agree = bool(np.array_equal(n_new, n_comp) and np.array_equal(n_new, n_rows))
    sums_same = bool(np.array_equal(out_sums[1].cpu().numpy().view(np.uint64), out_rows[1].cpu().numpy().view(np.uint64)))
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    stats = (C.c_longlong * 4)()
    check(L.pcreg_debug_set(b"knn_stats", 1))
    check(L.pcreg_debug_knn_stats(stats, 1))
    score_sums()
    torch.cuda.synchronize()
    check(L.pcreg_debug_knn_stats(stats, 1))
    check(L.pcreg_debug_set(b"knn_stats", 0))
    res = {"Q": Q, "M": pm.M, "B": B, "r": 1.5, "reps": a.reps, "n_close_agree": agree, "sum_bits_equal_with_and_without_rows": sums_same,
           "n_close_true": int(n_new[0]), "n_close_near_min": int(n_new[1:11].min()) if B > 1 else None,
           "n_close_wrong_min_max": [int(n_new[11:].min()), int(n_new[11:].max())] if B > 11 else None,
           "listed_pairs": int(stats[1]), "nominal_pairs": int(stats[2]), "listed_share": round(stats[1] / stats[2], 5) if stats[2] else None,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        res[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                          "iqr": round(float(np.subtract(*np.percentile(v, [75, 25]))), 3)}
    pm.close()
    print(json.dumps(res))
    if not agree:
        raise SystemExit("the new call and the composition disagree on n_close")


if __name__ == "__main__":
    main()
