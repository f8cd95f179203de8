"""The reference of the trimmed scoring and refits (pcreg_model_score_trimmed_f32's contract, include/pcreg.h), from
references that exist: tests/score_ref.py gives the candidate pairs, numpy's lexsort on (d, query) the order, and refit_ref /
plane_ref / gicp_ref the downstream of each method on the kept pairs.

keep_count(ratio, n)        -> keep: n == 0 ? 0 : min(n, max(1, floor(ratio * n + 0.5))), in double, product first
trim(idx, dist, ratio)      -> idx, dist (copies, -1 / +inf at trimmed slots), n_within, d2_cut (float32; +inf where keep is 0);
                               [Q] or [B, Q]
pairs(q, model, T, r2)      -> (tq [B, Q, 3], idx [B, Q], dist [B, Q]): scoring's candidate pairs, before any trim
step(...), steps(...)       -> the method's reference dict on the kept pairs, plus n_within and d2_cut
"""
from __future__ import annotations

import math

import numpy as np

import gicp_ref
import plane_ref
import refit_ref
import score_ref


def keep_count(ratio, n):
    n = int(n)
    if n == 0:
        return 0
    prod = float(ratio) * float(n)                 # (Python floats are IEEE doubles: the product is rounded, then the sum)
    return min(n, max(1, int(math.floor(prod + 0.5))))


def _trim1(idx, dist, ratio):
    idx, dist = np.asarray(idx, np.int32).copy(), np.asarray(dist, np.float32).copy()
    cand = np.flatnonzero(idx >= 0)
    n = len(cand)
    keep = keep_count(ratio, n)
    if keep == 0:
        return idx, dist, 0, np.float32(np.inf)
    order = cand[np.lexsort((cand, dist[cand]))]   # (d ascending, query ascending)
    cut = dist[order[keep - 1]]
    gone = order[keep:]
    idx[gone] = -1
    dist[gone] = np.inf
    return idx, dist, n, np.float32(cut)


def trim(idx, dist, ratio):
    idx, dist = np.asarray(idx), np.asarray(dist)
    if idx.ndim == 1:
        return _trim1(idx, dist, ratio)
    out = [_trim1(idx[b], dist[b], ratio) for b in range(len(idx))]
    return (np.stack([o[0] for o in out]).reshape(idx.shape), np.stack([o[1] for o in out]).reshape(dist.shape),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.float32))


def pairs(q, model, T, r2, threads=None):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tq = score_ref.transformed(q, T)
    B, Q = tq.shape[:2]
    if len(model) and Q:
        idx, dist = score_ref.within(*score_ref.nearest(tq.reshape(-1, 3), model, threads=threads), r2)
    else:
        idx, dist = np.full(B * Q, -1, np.int32), np.full(B * Q, np.inf, np.float32)
    return tq, idx.reshape(B, Q), dist.reshape(B, Q)


def step_of_pairs(cand, model, T, ratio, method="rigid", normals=None, qnormals=None, epsilon=gicp_ref.EPSILON):
    """one step on given candidate pairs (what pairs() returns for T): trim, then the method's sums and fit on the kept pairs"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tq, idx0, dist0 = cand
    idx, dist, n_within, d2_cut = trim(idx0, dist0, ratio)
    B = len(T)
    n_close, sum_d2 = score_ref.sums(idx, dist)
    T_step, T_out, empty = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.ones(B, bool)
    out = dict(T_step=T_step, T_out=T_out, empty=empty, hit=idx >= 0, idx=idx, dist=dist, tq=tq, n_close=n_close, sum_d2=sum_d2,
               n_within=n_within, d2_cut=d2_cut)
    o = plane_ref.origin(model)
    n_pl, res2, pivot = np.zeros(B, np.int32), np.zeros(B), np.full(B, np.nan)
    for b in range(B):
        if method == "rigid":
            S = refit_ref.fit(model, idx[b], tq[b]) if T[b].any() else None
        else:
            if method == "plane":
                s, n_pl[b] = plane_ref.sums_of_pairs(*plane_ref.plane_pairs(model, normals, idx[b], tq[b]), o)
            else:
                _hit, m, p, n, nq = gicp_ref.pairs(model, normals, qnormals, idx[b], tq[b])
                s, n_pl[b], _ok = gicp_ref.sums_of_pairs(m, p, n, nq, T[b], o, epsilon)
            res2[b] = float(s[27])
            S, pivot[b] = plane_ref.fit(s, n_pl[b], o) if T[b].any() else (None, np.nan)
        if S is not None:
            T_step[b], T_out[b], empty[b] = S, refit_ref.compose(T[b], S), False
    if method == "plane":
        out.update(n_plane=n_pl, sum_res2=res2, pivot=pivot)
    elif method == "gicp":
        out.update(n_pairs=n_pl, sum_res2=res2, pivot=pivot)
    return out


def step(q, model, T, r2, ratio, method="rigid", normals=None, qnormals=None, epsilon=gicp_ref.EPSILON, threads=None):
    return step_of_pairs(pairs(q, model, T, r2, threads=threads), model, T, ratio, method, normals, qnormals, epsilon)


def steps(q, model, T, r2, ratio, n, method="rigid", normals=None, qnormals=None, epsilon=gicp_ref.EPSILON, threads=None):
    """n steps, every one trimming anew; ratio None: the untrimmed method (everything within r2 is kept)"""
    out = []
    for _ in range(n):
        out.append(step(q, model, T, r2, 1.0 if ratio is None else ratio, method, normals, qnormals, epsilon, threads=threads))
        T = out[-1]["T_out"]
    return out


# ---- the partial-overlap scene ------------------------------------------------------------------------------
G = plane_ref.rigid([0.3, -0.2, 0.5], [4, -3, 2])          # tests/test_gpu_refit.py's rigid motion
_OVERLAP = {}


def overlap_scene(seed=7):
    """model: 3000 uniform rows in [-20, 20]^3.  surf: 1500 of those rows + N(0, 0.02^2) -- the part that overlaps, `true` their
    true place -- and 1000 OTHER rows displaced by (0.6, 0.3, 0) + the same noise -- wrong partners well inside r = 1.5 -- all
    moved by G, fp32.  T0: invertTF(G) times the third perturbation of test_gpu_refit.py."""
    if seed in _OVERLAP:
        return _OVERLAP[seed]
    from oracle.pcreg_oracle import invertTF
    rng = np.random.default_rng(seed)
    model = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    rows = rng.choice(3000, 2500, replace=False)
    true = model[rows[:1500]].astype(np.float64) + rng.normal(0, 0.02, (1500, 3))
    other = model[rows[1500:]].astype(np.float64) + np.array([0.6, 0.3, 0.0]) + rng.normal(0, 0.02, (1000, 3))
    cloud = np.vstack([true, other])
    surf = (cloud @ G[:3, :3] + G[3, :3]).astype(np.float32)
    T0 = invertTF(G) @ plane_ref.rigid(*plane_ref.PERTURBATIONS[2])
    _OVERLAP[seed] = dict(model=model, surf=surf, true=true, T0=T0, r2=np.float32(1.5) ** 2, ref={})
    return _OVERLAP[seed]


def overlap_rms(sc, T):
    """the RMS distance of the 1500 overlapping points, moved by T ([p, 1] @ T, float64), from their true place; NaN for no T"""
    if T is None or not np.asarray(T).any():
        return float("nan")
    return plane_ref.rms_to_truth(sc["surf"][:1500], np.asarray(T, np.float64), sc["true"])


def overlap_ref(ratio, n=4, seed=7, threads=None):
    """the reference's n steps on the overlap scene (ratio None: the radius refit), computed once and shared"""
    sc = overlap_scene(seed)
    key = (ratio, n)
    if key not in sc["ref"]:
        sc["ref"][key] = steps(sc["surf"], sc["model"], sc["T0"][None], sc["r2"], ratio, n, threads=threads)
    return sc["ref"][key]
