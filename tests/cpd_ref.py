"""The reference of the coherent-point-drift refit (pcreg_model_refit_cpd_f32's contract, include/pcreg.h).

step_ld(q, model, T, sigma2, w)  THE REFERENCE: the contract in np.longdouble.  The moved points are scoring's (score_ref.transformed:
                                 float64, rounded once to fp32 -- they are the data); every distance, weight and sum over all
                                 (live query, live row) pairs is formed in longdouble, in blocks of queries; the fit is the
                                 textbook one (numpy's SVD of the cross-covariance with the determinant correction) on the sums
                                 rounded to float64, whose own error -- a few 2^-53 -- is far below what it is compared with.
step32(q, model, T, sigma2, w)   THE CONTRACT'S ARITHMETIC restated in numpy: the fp32 distance by the fmaf formula, the shift by its
                                 fp32 minimum, exp2 correctly rounded to fp32, fp32 sums by fmaf, sequential in ascending row
                                 order, then the doubles and fit64.  |step32 - step_ld| is the METHOD ERROR: what the fp32 hot path
                                 costs, whatever the order of its sums.
fit64(sums, o)                   pcreg_amd/csrc/cpd_fit.hpp in float64, one operation per operation.
Both steps return dict(T_step [B, 4, 4], T_out [B, 4, 4] (as quickTF uses them, zeros where empty), empty [B] bool, sigma2_out,
Np, sum_res2, sum_d2 [B] float64, n_live [B] int32, sigma2 [B] the variance the step used, gap [B] -- step_ld only: the mean
distance between a live query's weighted model point and its nearest row).
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import plane_ref
import refit_ref
import score_ref
from cylinders_ref import _div, _sqrt, jacobi64

LD = np.longdouble
MIN_RATIO = 2.0 ** -26
LOG2E = 1.4426950408889634
TWO_PI = 6.283185307179586
BLOCK = 64
CLIP = 100.0


def live_rows(model):
    m = np.asarray(model, np.float32).reshape(-1, 3)
    return m[np.isfinite(m).all(axis=1)]


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded to float64 and then to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def initial_sigma2(u, v, dtype):
    """the mean squared distance over all pairs / 3, from the eight sums about o (u [Ql, 3], v [Ml, 3] in dtype)"""
    ql, ml = dtype(len(u)), dtype(len(v))
    mu, mv = u.sum(axis=0) / ql, v.sum(axis=0) / ml
    return (((u * u).sum() / ql + (v * v).sum() / ml) - 2 * (mu * mv).sum()) / 3


def _empty_result(B):
    z = lambda: np.zeros(B)
    return dict(T_step=np.zeros((B, 4, 4)), T_out=np.zeros((B, 4, 4)), empty=np.ones(B, bool), sigma2_out=z(), Np=z(), sum_res2=z(), sum_d2=z(),
                n_live=np.zeros(B, np.int32), sigma2=z(), gap=z())


def _candidate_ok(Tb, ql, ml, s2):
    return bool(Tb.any()) and bool(np.isfinite(Tb).all()) and ql >= 3 and ml >= 3 and s2 >= 0.0


def fit_svd(sums, o):
    """the textbook fit on the 19 sums (float64): Kabsch with the determinant correction -> (T_step 4 x 4 as quickTF uses it,
    sigma2_out), or None"""
    s = np.asarray(sums, np.float64)
    Np = s[0]
    if not (Np > 0 and np.isfinite(Np)):
        return None
    Sp, Sm, C = s[1:4], s[4:7], s[7:16].reshape(3, 3)
    mp, mm = Sp / Np, Sm / Np
    A = C.T - np.outer(mm, Sp)
    if not np.isfinite(A).all():
        return None
    U, sv, Vt = np.linalg.svd(A)
    if not sv[1] > MIN_RATIO * sv[0]:
        return None
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    sig = ((s[17] - mm @ Sm) - 2 * np.trace(A.T @ R) + (s[16] - mp @ Sp)) / (3 * Np)
    if not (sig > 0 and np.isfinite(sig)):
        return None
    T = np.eye(4)
    T[:3, :3] = R.T                                               # [p, 1] @ T: the row-vector convention
    T[3, :3] = (o + mm) - R @ (o + mp)
    return T, float(sig)


def step_ld(q, model, T, sigma2, w, dtype=LD):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    B = len(T)
    sig_in = np.broadcast_to(np.asarray(sigma2, np.float64).reshape(-1), (B,)) if np.size(sigma2) in (1, B) else None
    res = _empty_result(B)
    rows = live_rows(model)
    if not len(q) or not len(model):
        return res
    o = plane_ref.origin(rows).astype(np.float64)
    tq = score_ref.transformed(q, T)
    m = rows.astype(dtype)
    v = m - o.astype(dtype)
    w = dtype(w)
    with np.errstate(all="ignore"), ThreadPoolExecutor(min(len(os.sched_getaffinity(0)), 16)) as pool:
        for b in range(B):
            live = np.isfinite(tq[b]).all(axis=1)
            p = tq[b][live].astype(dtype)
            ql, ml = len(p), len(m)
            res["n_live"][b] = ql
            if not _candidate_ok(T[b], ql, ml, sig_in[b]):
                continue
            u = p - o.astype(dtype)
            s2 = dtype(sig_in[b]) if sig_in[b] != 0.0 else initial_sigma2(u, v, dtype)
            if not (s2 > 0 and np.isfinite(s2)):
                continue
            res["sigma2"][b] = float(s2)
            h = 1 / (2 * s2)
            c = (dtype(TWO_PI) * s2) ** dtype(1.5) * (w / (1 - w)) * (dtype(ml) / dtype(ql)) if w > 0 else dtype(0)
            def block(i0):
                np.seterr(all="ignore")                           # (the error state is per thread)
                pb, ub = p[i0:i0 + BLOCK], u[i0:i0 + BLOCK]
                d = m[None, :, :] - pb[:, None, :]                # [n, Ml, 3]: m - p'
                d2 = (d * d).sum(axis=2)
                j = d2.argmin(axis=1)
                dmin = d2[np.arange(len(pb)), j]
                arg = -(d2 - dmin[:, None]) * h
                near = arg > -CLIP                                # (a weight below e^-100 is below 2^-64 of S >= 1: no longdouble sees it)
                e = np.zeros_like(arg)
                e[near] = np.exp(arg[near])
                S = e.sum(axis=1)
                V = (e[:, :, None] * d).sum(axis=1)
                W = (e * d2).sum(axis=1)
                out = c * np.exp(dmin * h) if c > 0 else dtype(0)
                g = 1 / (S + out)
                pp = g * S
                gV, gW = g[:, None] * V, g * W
                y = pp[:, None] * ub + gV
                uu = (ub * ub).sum(axis=1)
                t = np.zeros(21, dtype)
                t[0] = pp.sum()
                t[1:4] = (pp[:, None] * ub).sum(axis=0)
                t[4:7] = y.sum(axis=0)
                t[7:16] = (ub[:, :, None] * y[:, None, :]).sum(axis=0).ravel()
                t[16] = (pp * uu).sum()
                t[17] = (pp * uu + 2 * (ub * gV).sum(axis=1) + gW).sum()
                t[18] = gW.sum()
                t[19] = dmin.sum()
                t[20] = np.sqrt(((V / S[:, None] - d[np.arange(len(pb)), j]) ** 2).sum(axis=1)).sum()
                return t
            tot = np.zeros(21, dtype)
            for t in pool.map(block, range(0, ql, BLOCK)):        # (map keeps the blocks' order: one order of the sums)
                tot += t
            sums, sum_d2, gap = tot[:19], tot[19], tot[20]
            res["Np"][b], res["sum_res2"][b], res["sum_d2"][b], res["gap"][b] = float(sums[0]), float(sums[18]), float(sum_d2), float(gap / ql)
            fit = fit_svd(sums.astype(np.float64), o)
            if fit is not None:
                res["T_step"][b], res["sigma2_out"][b] = fit
                res["T_out"][b], res["empty"][b] = refit_ref.compose(T[b], fit[0]), False
    return res


def weights32(p, rows, k2):
    """the hot path's arithmetic for the points p [N, 3] float32, each with its own k2 [N] float32 -> (dmin, S, Vx, Vy, Vz, W), fp32"""
    f0 = lambda: np.zeros(len(p), np.float32)
    with np.errstate(all="ignore"):
        dmin = np.full(len(p), np.inf, np.float32)
        for mj in rows:
            dx, dy, dz = mj[0] - p[:, 0], mj[1] - p[:, 1], mj[2] - p[:, 2]
            dmin = np.minimum(dmin, _fma32(dz, dz, _fma32(dy, dy, dx * dx)))
        S, Vx, Vy, Vz, W = f0(), f0(), f0(), f0(), f0()
        for mj in rows:                                           # sequential, in ascending row order
            dx, dy, dz = mj[0] - p[:, 0], mj[1] - p[:, 1], mj[2] - p[:, 2]
            d2 = _fma32(dz, dz, _fma32(dy, dy, dx * dx))
            e = np.exp2(((d2 - dmin) * k2).astype(np.float64)).astype(np.float32)
            S = S + e
            Vx, Vy, Vz, W = _fma32(e, dx, Vx), _fma32(e, dy, Vy), _fma32(e, dz, Vz), _fma32(e, d2, W)
    return dmin, S, Vx, Vy, Vz, W


def sums_of_weights(p, wts, ml, o, s2, w):
    """the doubles after the fp32 sums: one transform's live points p and their weights -> (sums [19] float64, sum_d2)"""
    dmin, S, Vx, Vy, Vz, W = wts
    ql, h = len(p), 1.0 / (2.0 * s2)
    with np.errstate(all="ignore"):
        Sd, dmd = S.astype(np.float64), dmin.astype(np.float64)
        c = ((TWO_PI * s2) * math.sqrt(TWO_PI * s2)) * (w / (1.0 - w)) * (ml / ql) if w > 0 else 0.0
        out = c * np.exp(dmd * h) if c > 0 else 0.0
        g = 1.0 / (Sd + out)
        pp = g * Sd
        u = p.astype(np.float64) - o
        gV = g[:, None] * np.stack([Vx, Vy, Vz], axis=1).astype(np.float64)
        gW = g * W.astype(np.float64)
        y = pp[:, None] * u + gV
        uu = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        sums = np.zeros(19)
        sums[0] = pp.sum()
        sums[1:4] = (pp[:, None] * u).sum(axis=0)
        sums[4:7] = y.sum(axis=0)
        sums[7:16] = (u[:, :, None] * y[:, None, :]).sum(axis=0).ravel()
        sums[16] = (pp * uu).sum()
        sums[17] = ((pp * uu + 2.0 * ((u[:, 0] * gV[:, 0] + u[:, 1] * gV[:, 1]) + u[:, 2] * gV[:, 2])) + gW).sum()
        sums[18] = gW.sum()
    return sums, float(dmd.sum())


def step32(q, model, T, sigma2, w):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    B = len(T)
    sig_in = np.broadcast_to(np.asarray(sigma2, np.float64).reshape(-1), (B,))
    res = _empty_result(B)
    rows = live_rows(model)
    if not len(q) or not len(model):
        return res
    o = plane_ref.origin(rows).astype(np.float64)
    tq = score_ref.transformed(q, T)
    v = rows.astype(np.float64) - o
    todo = []
    for b in range(B):
        live = np.isfinite(tq[b]).all(axis=1)
        ql, ml = int(live.sum()), len(rows)
        res["n_live"][b] = ql
        if not _candidate_ok(T[b], ql, ml, sig_in[b]):
            continue
        s2 = float(sig_in[b]) if sig_in[b] != 0.0 else float(initial_sigma2(tq[b][live].astype(np.float64) - o, v, np.float64))
        if not (s2 > 0 and math.isfinite(s2)):
            continue
        res["sigma2"][b] = s2
        todo.append(b)
    res["sums"] = np.zeros((B, 19))
    if not todo:
        return res
    pts = [tq[b][np.isfinite(tq[b]).all(axis=1)] for b in todo]   # every candidate's live points in one pass over the rows
    k2 = np.concatenate([np.full(len(p), np.float32(-((1.0 / (2.0 * res["sigma2"][b])) * LOG2E)), np.float32) for b, p in zip(todo, pts)])
    wts = weights32(np.concatenate(pts), rows, k2)
    at = np.cumsum([0] + [len(p) for p in pts])
    for n, (b, p) in enumerate(zip(todo, pts)):
        sums, res["sum_d2"][b] = sums_of_weights(p, [x[at[n]:at[n + 1]] for x in wts], len(rows), o, res["sigma2"][b], float(w))
        res["sums"][b], res["Np"][b], res["sum_res2"][b] = sums, sums[0], sums[18]
        fit = fit64(sums, o)
        if fit is not None:
            S = np.array(fit[0]).reshape(4, 4).T                  # the library's 16 doubles -> as quickTF uses it
            res["T_step"][b], res["sigma2_out"][b] = S, fit[1]
            res["T_out"][b], res["empty"][b] = refit_ref.compose(T[b], S), False
    return res


def fit64(sums, o):
    """cpd_fit.hpp in float64, one operation per operation (Python floats are IEEE doubles, never contracted) -> (T [16] in the
    library's layout, sigma2_out), or None"""
    s = [float(x) for x in sums]
    o = [float(x) for x in o]
    fin = lambda x: x - x == 0.0
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    with np.errstate(all="ignore"):
        Np = s[0]
        if not Np > 0.0 or not fin(Np):
            return None
        Sp, Sm = s[1:4], s[4:7]
        mp, mm = [_div(x, Np) for x in Sp], [_div(x, Np) for x in Sm]
        A = [[0.0] * 3 for _ in range(3)]
        sc = 0.0
        for a in range(3):
            for b in range(3):
                A[a][b] = s[7 + 3 * b + a] - mm[a] * Sp[b]
                if not fin(A[a][b]):
                    return None
                if abs(A[a][b]) > sc:
                    sc = abs(A[a][b])
        if not sc > 0.0:
            return None
        An = [[_div(A[a][b], sc) for b in range(3)] for a in range(3)]
        G = lambda a, b: (An[0][a] * An[0][b] + An[1][a] * An[1][b]) + An[2][a] * An[2][b]
        g, V = jacobi64([G(0, 0), G(0, 1), G(0, 2), G(1, 1), G(1, 2), G(2, 2)])
        l = [g[0], g[3], g[5]]
        if not all(fin(x) for x in l):
            return None
        i1 = 0
        if l[1] > l[0]:
            i1 = 1
        if l[2] > l[i1]:
            i1 = 2
        oa, ob = (1 if i1 == 0 else 0), (1 if i1 == 2 else 2)
        i2 = ob if l[ob] > l[oa] else oa
        v1, v2 = [V[3 * k + i1] for k in range(3)], [V[3 * k + i2] for k in range(3)]
        w1 = [(An[a][0] * v1[0] + An[a][1] * v1[1]) + An[a][2] * v1[2] for a in range(3)]
        w2 = [(An[a][0] * v2[0] + An[a][1] * v2[1]) + An[a][2] * v2[2] for a in range(3)]
        n1 = dot(w1, w1)
        if not (n1 > 0.0 and fin(n1)):
            return None
        s1 = _sqrt(n1)
        u1 = [_div(x, s1) for x in w1]
        d = dot(u1, w2)
        w2 = [w2[a] - d * u1[a] for a in range(3)]
        n2 = dot(w2, w2)
        if not (n2 > 0.0 and fin(n2)):
            return None
        s2 = _sqrt(n2)
        if not s2 > MIN_RATIO * s1:
            return None
        u2 = [_div(x, s2) for x in w2]
        u3, v3 = cross(u1, u2), cross(v1, v2)
        R = [[0.0] * 3 for _ in range(3)]
        tr = 0.0
        for a in range(3):
            for b in range(3):
                R[a][b] = (u1[a] * v1[b] + u2[a] * v2[b]) + u3[a] * v3[b]
                tr = tr + A[a][b] * R[a][b]
        sig = _div(((s[17] - dot(mm, Sm)) - 2.0 * tr) + (s[16] - dot(mp, Sp)), 3.0 * Np)
        if not sig > 0.0 or not fin(sig):
            return None
        c = [o[k] + mp[k] for k in range(3)]
        out = [0.0] * 16
        for j in range(3):
            for i in range(3):
                out[4 * j + i] = R[j][i]
            out[4 * j + 3] = (o[j] + mm[j]) - ((R[j][0] * c[0] + R[j][1] * c[1]) + R[j][2] * c[2])
        out[15] = 1.0
        if not all(fin(x) for x in out[:12]):
            return None
    return np.array(out, np.float64), float(sig)


def steps_ld(q, model, T, sigma2, w, n, dtype=np.float64):
    """n steps, each feeding the next its T_out and sigma2_out -> the list of the n results"""
    out = []
    for _ in range(n):
        r = step_ld(q, model, T, sigma2, w, dtype=dtype)
        out.append(r)
        T, sigma2 = r["T_out"], r["sigma2_out"]
    return out


def spacing2(model):
    """the square of the model's median nearest-row spacing (float64)"""
    import knn_k_ref
    m = live_rows(model)
    _, d = knn_k_ref.knn(m, m, 2)
    return float(np.median(d[:, 1].astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------- the main scene
OUTLIERS = (0.0, 0.1)
_CASES = {}


def scene_sigma2s():
    """the three variances of the main scene's cases: the initial value, 1.0, and (spacing / 100)^2"""
    return (0.0, 1.0, spacing2(plane_ref.scene()["model"]) / 1e4)


def scene_case(w, sigma2):
    """(step_ld, step32) of plane_ref.scene() at (w, sigma2), computed once a process"""
    key = (float(w), float(sigma2))
    if key not in _CASES:
        sc = plane_ref.scene()
        _CASES[key] = (step_ld(sc["surf"], sc["model"], sc["T"], sigma2, w), step32(sc["surf"], sc["model"], sc["T"], sigma2, w))
    return _CASES[key]


E_FLOOR = 2.0 ** -49      # the double arithmetic after the fp32 sums: two roundings a query and a tree of depth 12, 16 x 2^-53


def method_error(ld, s32):
    """per OUTPUT the method error |step32 - step_ld| of one call: T_step in Frobenius norm, sigma2_out, Np and sum_res2 relative, each
    the WORST over the candidates both computations fit -- the error is a property of the fp32 method at the call's sizes, and one
    candidate's figure is a single draw of it, now and then several times below its neighbours' -- and never below E_FLOOR, what
    the doubles themselves cost -> (both [B] bool, dict of floats (NaN when no candidate is fitted by both), dict of the [B] draws)"""
    both = ~ld["empty"] & ~s32["empty"]
    with np.errstate(all="ignore"):
        draws = {"T_step": np.where(both, np.linalg.norm(ld["T_step"] - s32["T_step"], axis=(1, 2)), np.nan)}
        for k in ("sigma2_out", "Np", "sum_res2"):
            draws[k] = np.where(both, np.abs(ld[k] - s32[k]) / np.abs(ld[k]), np.nan)
    E = {k: max(float(np.nanmax(v)), E_FLOOR) if both.any() else float("nan") for k, v in draws.items()}
    return both, E, draws


TRAJECTORY_STEPS = (1, 5, 10, 20)
_TRAJECTORY = []


def trajectory():
    """the worst perturbation of the main scene from sigma2_in = 0 with w = 0.1: the RMS to truth after 1, 5, 10 and 20 steps of
    step_ld (in float64: twenty all-pairs steps in longdouble take a minute, and the figures are held to 1e-3) -> [4] floats"""
    if not _TRAJECTORY:
        sc = plane_ref.scene()
        rs = steps_ld(sc["surf"], sc["model"], sc["T"][3:4], 0.0, 0.1, max(TRAJECTORY_STEPS))
        _TRAJECTORY.extend(plane_ref.rms_to_truth(sc["surf"], rs[n - 1]["T_out"][0], sc["cloud"]) for n in TRAJECTORY_STEPS)
    return list(_TRAJECTORY)
