"""TEST REFERENCE for MSAC cylinder fitting and extraction on a prepared model (pcreg_model_fit_cylinders_f32's contract in
include/pcreg.h), in numpy and Python integers.

The fp32 scoring chain (the cross product with the axis by fmaf, c2 = fmaf(cz, cz, fmaf(cy, cy, cx * cx)), rho = sqrt(c2),
r = rho - Rf, r2 = r * r) is taken exactly: each fmaf by tests/planes_ref.py's round-to-odd construction, the root by numpy.sqrt on
float32 (IEEE: correctly rounded).  The trial's cylinder is float64, operation by operation (a Python float operation is one
correctly rounded double operation).  cost, count and both sets of the refit's sums are Python integers; N and h are Python integers
rounded once by float(int).  finish64 restates pcreg_amd/csrc/cylinder_fit.hpp in float64 -- its Jacobi included, which is the
library's jacobi_sym3 with the cosine as 1 / sqrt, so that every operation is a correctly rounded one; finish_exact solves the same
rounded 2 x 2 system in fractions.Fraction, given the basis.

round_(m, nrm, alive, p, ...) runs ONE round from a given alive set; fit_cylinders(...) the whole extraction; classify(m, alive,
centre, w, R, t) restates the final classification from any cylinder, e.g. the RETURNED one."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from planes_ref import EPS, MASK, QMAX, _fma32, exponent, finite_rows, q_of, sign_flip, splitmix64, thresholds  # noqa: F401

SPLIT = 18
DBL_EPSILON = 2.0 ** -52


def _f32(v) -> np.float32:
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(v)


def _sqrt(v: float) -> float:
    return math.sqrt(v) if v >= 0 else math.nan                            # (NaN in, NaN out: NaN >= 0 is False)


def _div(a: float, b: float) -> float:
    """IEEE a / b in float64 (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mul32(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def usable(nrm) -> np.ndarray:
    """the rows whose normal is usable: three finite components, each at most 2 in magnitude"""
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(nrm) <= np.float32(2)).all(axis=1)


def chain(rows, af, wf, Rf):
    """the contract's fp32 chain -> (r2 [N] float32, h [N] float32) of rows [N, 3] against the cylinder (af, wf float32 [3], Rf)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    af, wf = np.asarray(af, np.float32), np.asarray(wf, np.float32)
    n = len(rows)
    full = lambda v: np.full(n, v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = rows - af[None, :]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        cx = _fma32(dy, full(wf[2]), -_mul32(dz, full(wf[1])))
        cy = _fma32(dz, full(wf[0]), -_mul32(dx, full(wf[2])))
        cz = _fma32(dx, full(wf[1]), -_mul32(dy, full(wf[0])))
        c2 = _fma32(cz, cz, _fma32(cy, cy, _mul32(cx, cx)))
        rho = np.sqrt(c2)                                                   # float32 in, float32 out: correctly rounded
        r = (rho - np.float32(Rf)).astype(np.float32)
        h = _fma32(dz, full(wf[2]), _fma32(dy, full(wf[1]), _mul32(dx, full(wf[0]))))
        return _mul32(r, r), h


def chain_r2(rows, af, wf, Rf) -> np.ndarray:
    return chain(rows, af, wf, Rf)[0]


def trial_rows(p, B, b, seed, A):
    """the sampler: two original rows of the alive list A (ascending), or None where A is empty"""
    if len(A) == 0:
        return None
    return [int(A[splitmix64(seed ^ splitmix64(((p * B + b) * 4 + j) & MASK)) % len(A)]) for j in range(2)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def trial_cylinder(p0, p1, n0, n1, ref_vec=None, max_angle=math.pi / 2):
    """the contract's trial geometry in float64, operation by operation -> (ok, a [3], w [3], R) as Python floats"""
    with np.errstate(all="ignore"):
        p0, p1, n0, n1 = ([float(v) for v in np.asarray(x, np.float32)] for x in (p0, p1, n0, n1))
        W = _cross(n0, n1)
        L2 = _dot(W, W)
        if not (L2 > 0 and math.isfinite(L2)):
            return False, None, None, None
        ln = math.sqrt(L2)
        w = [_div(W[c], ln) for c in range(3)]
        ok = True
        if ref_vec is not None:
            r = [float(v) for v in ref_vec]
            dot = _dot(w, r)
            if dot < 0:
                w = [-v for v in w]
                dot = -dot
            rlen = math.sqrt(_dot(r, r))
            if _div(dot, rlen) < math.cos(max_angle):
                ok = False
        elif sign_flip(w, None):
            w = [-v for v in w]
        d = [p1[c] - p0[c] for c in range(3)]
        mm = _cross(d, n1)
        num = _dot(mm, W)
        s = _div(num, L2)
        a = [p0[c] + s * n0[c] for c in range(3)]
        R = abs(s) * math.sqrt(_dot(n0, n0))
        if not all(math.isfinite(v) for v in [s, *a, R]):
            ok = False
        return ok, a, w, R


def hypothesis(m, nrm, alive, idx, min_radius=0.0, max_radius=math.inf, ref_vec=None, max_angle=math.pi / 2):
    """-> (void, p0 float32 [3], af float32 [3], wf float32 [3], Rf float32) of the trial with the 0-based original rows idx"""
    z = np.zeros(3, np.float32)
    void = (True, z, z, z, np.float32(0))
    M = len(m)
    if idx is None or any(i < 0 or i >= M for i in idx) or any(not alive[i] for i in idx):
        return void
    if idx[0] == idx[1]:
        return void
    ok_n = usable(nrm[list(idx)])
    if not ok_n.all():
        return void
    p0 = m[idx[0]].copy()
    ok, a, w, R = trial_cylinder(m[idx[0]], m[idx[1]], nrm[idx[0]], nrm[idx[1]], ref_vec, max_angle)
    if not ok:
        return True, p0, z, z, np.float32(0)
    af = np.array([_f32(v) for v in a], np.float32)
    wf = np.array([_f32(v) for v in w], np.float32)
    Rf = _f32(R)
    if not (np.isfinite(af).all() and np.isfinite(wf).all() and np.isfinite(Rf)) or Rf < np.float32(min_radius) or Rf > np.float32(max_radius):
        return True, p0, z, z, np.float32(0)
    return False, p0, af, wf, Rf


def classify(m, alive, centre, w, R, max_distance) -> dict:
    """the final classification from (centre, w float64 [3], R float64): mask [M] of the passing alive rows, count, Q, rmse, extents"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    t2, s = thresholds(max_distance)
    rows = np.flatnonzero(alive)
    r2, h = chain(m[rows], np.asarray(centre, np.float64).astype(np.float32), np.asarray(w, np.float64).astype(np.float32), _f32(np.float64(R)))
    with np.errstate(invalid="ignore"):
        ok = r2 <= t2
    mask = np.zeros(len(m), bool)
    mask[rows[ok]] = True
    count = int(ok.sum())
    Q = int(q_of(r2[ok], s).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = float(np.sqrt((np.float64(Q) / np.float64(count)) * (np.float64(t2) * 2.0 ** -20)))
    ext = [float(h[ok].min()), float(h[ok].max())] if count else [math.nan, math.nan]
    return dict(mask=mask, count=count, Q=Q, rmse=rmse, r2=r2, rows=rows, extents=ext)


# ---- the refit ---------------------------------------------------------------------------------------------------------------------
def axis_sums(nrm_inl):
    """the seven sums of the usable normals among nrm_inl [N, 3] float32 -> Python ints: n_n, xx xy xz yy yz zz"""
    nrm_inl = np.asarray(nrm_inl, np.float32).reshape(-1, 3)
    g = [[int(v) for v in row] for row in np.rint(nrm_inl[usable(nrm_inl)].astype(np.float64) * 65536.0)]
    prs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return [len(g)] + [sum(r[a] * r[b] for r in g) for a, b in prs], max((abs(v) for r in g for v in r), default=0)


def circle_sums(g, u, v):
    """the eleven sums of the quantised differences g (rows of three Python ints) projected on (u, v) -> (a list of 11 Python ints,
    max |xi|, |yi|)"""
    xy = []
    for r in g:
        gx, gy, gz = float(r[0]), float(r[1]), float(r[2])
        X = (gx * u[0] + gy * u[1]) + gz * u[2]
        Y = (gx * v[0] + gy * v[1]) + gz * v[2]
        xy.append((int(np.rint(X)), int(np.rint(Y))))
    w2 = [x * x + y * y for x, y in xy]
    lo = [t & ((1 << SPLIT) - 1) for t in w2]
    hi = [t >> SPLIT for t in w2]
    S = [len(xy), sum(x for x, _ in xy), sum(y for _, y in xy), sum(x * x for x, _ in xy), sum(x * y for x, y in xy),
         sum(y * y for _, y in xy), sum(w2), sum(x * l for (x, _), l in zip(xy, lo)), sum(x * h for (x, _), h in zip(xy, hi)),
         sum(y * l for (_, y), l in zip(xy, lo)), sum(y * h for (_, y), h in zip(xy, hi))]
    return S, max((max(abs(x), abs(y)) for x, y in xy), default=0)


def normal_equations(S):
    """(N3, h, S1, sw, n) as float64, each entry of N and h formed exactly as a Python integer and rounded ONCE by float(int)"""
    n, sx, sy, sxx, sxy, syy, sw = S[:7]
    gw = [S[8] * (1 << SPLIT) + S[7], S[10] * (1 << SPLIT) + S[9]]
    N3 = [float(n * sxx - sx * sx), float(n * sxy - sx * sy), float(n * syy - sy * sy)]
    h = [float(n * gw[0] - sx * sw), float(n * gw[1] - sy * sw)]
    return N3, h, [float(sx), float(sy)], float(sw), float(n)


def jacobi64(a6):
    """cylinder_fit.hpp's fit_cylinders_jacobi restated: a6 = [a00, a01, a02, a11, a12, a22] -> (a [6], V [9] row-major)"""
    a = [float(v) for v in a6]
    V = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    with np.errstate(all="ignore"):
        for _ in range(60):
            off = abs(a[1]) + abs(a[2]) + abs(a[4])
            dia = abs(a[0]) + abs(a[3]) + abs(a[5])
            if off <= 1e-300 or off <= DBL_EPSILON * 1e-3 * dia:
                break
            for APP, AQQ, APQ, ARP, ARQ, P, Q in ((0, 3, 1, 2, 4, 0, 1), (0, 5, 2, 1, 4, 0, 2), (3, 5, 4, 1, 2, 1, 2)):
                if a[APQ] != 0.0:
                    h, d = 2.0 * a[APQ], a[AQQ] - a[APP]
                    t = _div(math.copysign(abs(h), 1.0 if h * d >= 0.0 else -1.0), abs(d) + _sqrt(d * d + h * h))
                    c = _div(1.0, _sqrt(t * t + 1.0))
                    s = c * t
                    tp = t * a[APQ]
                    a[APP] -= tp
                    a[AQQ] += tp
                    a[APQ] = 0.0
                    rp, rq = a[ARP], a[ARQ]
                    a[ARP] = c * rp - s * rq
                    a[ARQ] = s * rp + c * rq
                    for k in range(3):
                        vp, vq = V[k * 3 + P], V[k * 3 + Q]
                        V[k * 3 + P] = c * vp - s * vq
                        V[k * 3 + Q] = s * vp + c * vq
    return a, V


def _radicand_ok(v: float) -> bool:
    return v > 0 and math.isfinite(v)


def basis64(A6, n_n, ref_vec=None):
    """fit_cylinders_basis restated -> (ok, w, u, v) as lists of Python floats (None where not ok)"""
    if n_n < 2:
        return False, None, None, None
    with np.errstate(all="ignore"):
        a, V = jacobi64(A6)
        if not all(math.isfinite(a[i]) for i in (0, 3, 5)):
            return False, None, None, None
        c = 0
        if a[3] < a[0]:
            c = 1
        if a[5] < (a[3] if c == 1 else a[0]):
            c = 2
        w = [V[c], V[3 + c], V[6 + c]]
        if not all(math.isfinite(x) for x in w):
            return False, None, None, None
        if sign_flip(w, ref_vec):
            w = [-x for x in w]
        k, wk = 0, abs(w[0])
        if abs(w[1]) < wk:
            k, wk = 1, abs(w[1])
        if abs(w[2]) < wk:
            k = 2
        e = [1.0 if i == k else 0.0 for i in range(3)]
        cr = _cross(w, e)
        l2 = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]
        if not _radicand_ok(l2):
            return False, None, None, None
        ln = math.sqrt(l2)
        u = [_div(x, ln) for x in cr]
        v = _cross(w, u)
    return True, w, u, v


def circle64(N3, h, S1, sw, n, p0, u, v, back, min_radius=0.0, max_radius=math.inf) -> dict:
    """fit_cylinders_circle restated -> dict(used, centre [3], R, a [2], Rg2)"""
    N3, h, S1, p0, u, v = ([float(x) for x in y] for y in (N3, h, S1, p0, u, v))
    sw, n, back = float(sw), float(n), float(back)
    out = dict(used=False, centre=None, R=None, a=None, Rg2=None)
    with np.errstate(all="ignore"):
        r0 = N3[0]
        if not _radicand_ok(r0):
            return out
        L00 = math.sqrt(r0)
        L10 = _div(N3[1], L00)
        r1 = N3[2] - L10 * L10
        if not _radicand_ok(r1):
            return out
        L11 = math.sqrt(r1)
        y0 = _div(h[0], L00)
        y1 = _div(h[1] - L10 * y0, L11)
        a1 = _div(y1, L11)
        a0 = _div(y0 - L10 * a1, L00)
        cx, cy = a0 / 2.0, a1 / 2.0
        beta = _div(sw - (a0 * S1[0] + a1 * S1[1]), n)
        Rg2 = beta + (cx * cx + cy * cy)
        out.update(a=[a0, a1], Rg2=Rg2)
        if not _radicand_ok(Rg2):
            return out
        centre = [p0[i] + (cx * u[i] + cy * v[i]) * back for i in range(3)]
        R = math.sqrt(Rg2) * back
        if not all(math.isfinite(x) for x in centre) or not math.isfinite(R):
            return out
        Rf = _f32(R)
        if not (Rf >= np.float32(min_radius) and Rf <= np.float32(max_radius)):
            return out
    out.update(used=True, centre=centre, R=R)
    return out


def finish64(A6, n_n, circle, p0, back, min_radius=0.0, max_radius=math.inf, ref_vec=None) -> dict:
    """pcreg_amd/csrc/cylinder_fit.hpp restated in float64, both steps: circle is (N3, h, S1, sw, n), or a function (u, v) -> that
    tuple (the circle pass' sums depend on the basis) -> dict(basis_ok, w, u, v, used, centre, R, a, Rg2, circle)"""
    ok, w, u, v = basis64(A6, n_n, ref_vec)
    out = dict(basis_ok=ok, w=w, u=u, v=v, used=False, centre=None, R=None, a=None, Rg2=None, circle=None)
    if not ok:
        return out
    if callable(circle):
        circle = circle(u, v)
    out["circle"] = circle
    out.update(circle64(*circle, p0, u, v, back, min_radius, max_radius))
    return out


def finish_exact(N3, h):
    """N a = h solved exactly for the SAME rounded doubles -> a as two Fractions (None where N is singular)"""
    n00, n01, n11 = (Fraction(x) for x in N3)
    h0, h1 = Fraction(h[0]), Fraction(h[1])
    D = n00 * n11 - n01 * n01
    if D == 0:
        return None
    return [(h0 * n11 - h1 * n01) / D, (n00 * h1 - n01 * h0) / D]


def kappa2(N3) -> float:
    ev = np.linalg.eigvalsh(np.array([[N3[0], N3[1]], [N3[1], N3[2]]], np.float64))
    return float(ev[-1] / ev[0]) if ev[0] > 0 else math.inf


def round_(m, nrm, alive, p, max_distance, n_trials, min_inliers=4, seed=0, samples=None, min_radius=0.0, max_radius=math.inf,
           ref_vec=None, max_angle=math.pi / 2, e=None) -> dict:
    """ONE round of the contract from the alive set `alive` (bool [M]).  samples: 0-based rows [B, 2] of THIS round, or None.
    -> dict: void [B], cost [B] (Python ints), count [B], best_trial (-1: none), best_cost, best_count, stop; and, unless stop,
    trial (p0, af, wf, Rf), asums (7 Python ints), csums (11, None where the basis failed), fit (finish64's dict), used, centre, w, R
    (the round's cylinder), max_gn, max_g, max_xy"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    alive = np.asarray(alive, bool)
    A = np.flatnonzero(alive)
    B = int(n_trials)
    t2, s = thresholds(max_distance)
    if e is None:
        e = exponent(m)
    void = np.zeros(B, bool)
    cost = [0] * B
    count = np.zeros(B, np.int64)
    hyp = []
    rows = m[A]
    for b in range(B):
        idx = [int(v) for v in samples[b]] if samples is not None else trial_rows(p, B, b, seed, A)
        v, p0, af, wf, Rf = hypothesis(m, nrm, alive, idx, min_radius, max_radius, ref_vec, max_angle)
        hyp.append((p0, af, wf, Rf))
        void[b] = v
        if v:
            continue
        r2 = chain_r2(rows, af, wf, Rf)
        with np.errstate(invalid="ignore"):
            ok = r2 <= t2
        count[b] = int(ok.sum())
        cost[b] = int(q_of(r2[ok], s).sum()) + QMAX * int(len(A) - count[b])
    elig = [b for b in range(B) if not void[b] and count[b] >= 4]
    out = dict(void=void, cost=cost, count=count, e=e, alive_rows=A)
    if not elig:
        out.update(best_trial=-1, best_cost=0, best_count=0, stop=True)
        return out
    best = min(elig, key=lambda b: (cost[b], b))
    out.update(best_trial=best, best_cost=cost[best], best_count=int(count[best]), stop=bool(count[best] < min_inliers))
    if out["stop"]:
        return out
    p0, af, wf, Rf = hyp[best]
    r2 = chain_r2(rows, af, wf, Rf)
    with np.errstate(invalid="ignore"):
        inl = r2 <= t2
    asums, max_gn = axis_sums(nrm[A[inl]])
    d = (rows[inl] - p0[None, :]).astype(np.float64) * 2.0 ** (17 - e)      # the fp32 differences, scaled exactly
    g = [[int(v) for v in row] for row in np.rint(d)]
    keep = {}

    def circ(u, v):
        S, mx = circle_sums(g, u, v)
        keep["S"], keep["max_xy"] = S, mx
        return normal_equations(S)

    fit = finish64([float(v) for v in asums[1:]], asums[0], circ, [float(v) for v in p0], 2.0 ** -(17 - e), min_radius, max_radius, ref_vec)
    if fit["used"]:
        centre, w, R = fit["centre"], fit["w"], fit["R"]
    else:
        centre, w, R = [float(v) for v in af], [float(v) for v in wf], float(Rf)
    out.update(trial=(p0, af, wf, Rf), asums=asums, csums=keep.get("S"), fit=fit, used=bool(fit["used"]), centre=centre, w=w, R=R,
               max_gn=max_gn, max_g=max((abs(v) for r in g for v in r), default=0), max_xy=keep.get("max_xy", 0))
    return out


def fit_cylinders(m, nrm, max_distance, min_radius=0.0, max_radius=math.inf, ref_vec=None, max_angle=math.pi / 2, max_cylinders=1,
                  n_trials=100, min_inliers=4, seed=0, samples=None) -> dict:
    """the whole extraction; samples 0-based [P, B, 2] or None"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    M, P = len(m), int(max_cylinders)
    alive = finite_rows(m) if M else np.zeros(0, bool)
    e = exponent(m)
    out = dict(n_cylinders=0, labels=np.zeros(M, np.int32), cylinders=np.zeros((P, 7)), extents=np.zeros((P, 2)),
               counts=np.zeros(P, np.int32), rmse=np.zeros(P), refit_used=np.zeros(P, np.int32), best_trial=np.zeros(P, np.int32),
               best_cost=np.zeros(P, np.int64), best_count=np.zeros(P, np.int32), rounds=[])
    if M == 0:
        return out
    for p in range(P):
        r = round_(m, nrm, alive, p, max_distance, n_trials, min_inliers, seed, None if samples is None else np.asarray(samples)[p],
                   min_radius, max_radius, ref_vec, max_angle, e)
        out["rounds"].append(r)
        out["best_trial"][p], out["best_cost"][p], out["best_count"][p] = r["best_trial"], r["best_cost"], r["best_count"]
        if r["stop"]:
            break
        c = classify(m, alive, r["centre"], r["w"], r["R"], max_distance)
        out["labels"][c["mask"]] = p + 1
        alive = alive & ~c["mask"]
        out["cylinders"][p] = [*r["centre"], *r["w"], r["R"]]
        out["extents"][p] = c["extents"]
        out["counts"][p] = c["count"]
        out["rmse"][p] = c["rmse"]
        out["refit_used"][p] = int(r["used"])
        out["n_cylinders"] = p + 1
    return out


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
SCENE_CYLINDERS = (((7.0, 8.0, 9.0), (1.0, 2.0, 2.0), 3.0, 12.0, 2.0 * math.pi), ((14.0, 12.0, 5.0), (2.0, -1.0, 1.0), 1.5, 8.0, math.pi))
SCENE_OFFSET = (100.0, 50.0, 90.0)


def _frame(w):
    w = np.asarray(w, np.float64) / np.linalg.norm(w)
    k = int(np.argmin(np.abs(w)))
    u = np.cross(w, np.eye(3)[k])
    u /= np.linalg.norm(u)
    return w, u, np.cross(w, u)


def scene(M: int, seed: int = 11):
    """two noisy cylinder surfaces (radius 3, length 12, 40 % of the rows, a full turn; radius 1.5, length 8, 25 %, a half turn, as a
    stereo view sees it; radial sigma 0.02; different oblique axes), a planar patch 10 x 10 with 15 %, and uniform clutter in a box
    of extent 20, everything offset by (100, 50, 90), rows shuffled.  Normals: the analytic ones plus N(0, 0.03) per component,
    renormalised, rounded to fp32; the clutter's are random.  -> (m float32 [M, 3], nrm float32 [M, 3], kind [M]: 1, 2 the
    cylinders, 3 the patch, 0 clutter)"""
    rng = np.random.default_rng(seed)
    ns = (int(0.40 * M), int(0.25 * M), int(0.15 * M))
    nc = M - sum(ns)
    pts, nrm, kind = [], [], []
    for k, ((c, w, R, L, turn), n) in enumerate(zip(SCENE_CYLINDERS, ns[:2])):
        w, u, v = _frame(w)
        th = rng.uniform(0, turn, n)
        hh = rng.uniform(-L / 2, L / 2, n)
        rad = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
        pts.append(np.array(c) + hh[:, None] * w + rad * (R + rng.normal(0, 0.02, (n, 1))))
        nrm.append(rad)
        kind.append(np.full(n, k + 1))
    xy = rng.uniform(0, 10, (ns[2], 2))
    pts.append(np.column_stack([xy[:, 0] + 1.0, xy[:, 1] + 9.0, np.full(ns[2], 18.5) + rng.normal(0, 0.02, ns[2])]))
    nrm.append(np.tile([0.0, 0.0, 1.0], (ns[2], 1)))
    kind.append(np.full(ns[2], 3))
    pts.append(rng.uniform(0, 20, (nc, 3)))
    nrm.append(rng.normal(size=(nc, 3)))
    kind.append(np.zeros(nc, int))
    pts, nrm, kind = np.vstack(pts) + np.array(SCENE_OFFSET), np.vstack(nrm), np.concatenate(kind)
    noisy = nrm + np.where(kind[:, None] > 0, rng.normal(0, 0.03, nrm.shape), 0.0)
    noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
    perm = rng.permutation(M)
    return pts[perm].astype(np.float32), noisy[perm].astype(np.float32), kind[perm]


# ---- the knife edge: rows exactly at radius 5 about the z axis through (16, 32, 0), and pairs on the x axis about R + t ------------------
KNIFE_C, KNIFE_R, KNIFE_T = (16.0, 32.0), 5.0, 0.0625
KNIFE_HEIGHTS = (0.0, 1.0, 2.0, 3.0, 5.0, 8.0)
KNIFE_SAMPLE = (0, 15)                       # the rows (-5, 0) at height 0 and (-3, -4) at height 1 (twelve directions a height)


def knife_scene():
    """-> (m float32 [n + 6, 3], nrm float32 [n + 6, 3], n): n lattice rows at EXACTLY radius 5 about the line (16, 32, z) (the signed
    permutations of (3, 4) and (5, 0) at several integer heights; their normals are the radial directions as (dx, dy, 0) / 4, of
    length 1.25: normals are used as given, and these are exact in fp32, which (dx, dy, 0) / 5 would not be, so every product and
    sum of the trial geometry is exact for them), then three pairs (cx + d, cx - d) on the x axis at height 4 with d = R + t, the
    float below it and the float above it; their normals are (+-1, 0, 0)."""
    dirs = sorted({(a * sa, b * sb) for a, b in ((3, 4), (4, 3), (5, 0), (0, 5)) for sa in (1, -1) for sb in (1, -1)})
    lat = np.array([[KNIFE_C[0] + dx, KNIFE_C[1] + dy, z] for z in KNIFE_HEIGHTS for dx, dy in dirs], np.float64)
    nl = np.array([[dx / 4.0, dy / 4.0, 0.0] for _ in KNIFE_HEIGHTS for dx, dy in dirs], np.float64)
    step = float(np.spacing(np.float32(KNIFE_C[0] + KNIFE_R + KNIFE_T)))      # one float at cx + R + t; cx - d holds it too
    ds = [KNIFE_R + KNIFE_T, KNIFE_R + KNIFE_T - step, KNIFE_R + KNIFE_T + step]
    knife = np.array([[KNIFE_C[0] + sg * d, KNIFE_C[1], 4.0] for d in ds for sg in (1, -1)], np.float64)
    nk = np.array([[float(sg), 0.0, 0.0] for d in ds for sg in (1, -1)], np.float64)
    assert np.array_equal(knife.astype(np.float32).astype(np.float64), knife)
    return np.vstack([lat, knife]).astype(np.float32), np.vstack([nl, nk]).astype(np.float32), len(lat)


# ---- shared cases of tests/test_cylinders_ref.py (their premises, on the CPU) and tests/test_gpu_fit_cylinders.py ---------------------
SCENES = ((1030, 256, 60), (4096, 256, 200))                                  # M, B, min_inliers; t = 0.08, max_radius 6, P = 5
SCENE_T, SCENE_RMAX, SCENE_P, SCENE_SEED = 0.08, 6.0, 5, 7


def sample_table(M, kind, P, B, seed):
    """a caller's table [P, B, 2] of 0-based rows: in every round B / 8 trials drawn within each of the two cylinders' rows and the
    patch's (two different rows each), the rest uniformly among all rows"""
    rng = np.random.default_rng(seed)
    smp = rng.integers(0, M, (P, B, 2)).astype(np.int32)
    for p in range(P):
        for k in (1, 2, 3):
            rows = np.flatnonzero(np.asarray(kind) == k)
            for b in range((k - 1) * (B // 8), k * (B // 8)):
                smp[p, b] = rng.choice(rows, 2, replace=False)
    return smp


def bad_sample_scene():
    """-> (m, nrm, smp, kind): the 1030-row scene with the normals of four clutter rows written over (two exactly parallel, one NaN,
    one with a component of 3) and a table [3, 256, 2] whose first trials are an equal pair, an index past the end, an index below 0,
    the parallel pair (L2 == 0), the NaN normal and the component of 3; trial 6 is a sound pair in round 0 and names two rows that
    round 0 removes in rounds 1 and 2"""
    m, nrm, kind = (np.array(a) for a in scene(1030))
    M = len(m)
    c = [int(v) for v in np.flatnonzero(kind == 0)[:4]]
    nrm[c[0]] = nrm[c[1]] = [0.0, 0.0, 1.0]
    nrm[c[2]] = [np.nan, 0.0, 1.0]
    nrm[c[3]] = [3.0, 0.0, 0.0]
    smp = sample_table(M, kind, 3, 256, 21)
    a = [int(v) for v in np.flatnonzero(kind == 1)[:4]]
    smp[:, 0] = [a[0], a[0]]
    smp[:, 1] = [a[0], M]
    smp[:, 2] = [-1, a[1]]
    smp[:, 3] = [c[0], c[1]]
    smp[:, 4] = [c[2], a[2]]
    smp[:, 5] = [a[3], c[3]]
    alive = finite_rows(m)
    rows1 = np.flatnonzero(kind == 1)
    for j in range(len(rows1) - 1):                                           # a pair of cylinder 1 that makes a trial in bounds
        if not hypothesis(m, nrm, alive, [int(rows1[j]), int(rows1[j + 1])], 0.0, SCENE_RMAX)[0]:
            smp[:, 6] = [rows1[j], rows1[j + 1]]
            break
    r0 = round_(m, nrm, alive, 0, SCENE_T, 256, 60, 0, smp[0], 0.0, SCENE_RMAX)
    gone = classify(m, alive, r0["centre"], r0["w"], r0["R"], SCENE_T)["mask"]
    smp[1:, 6] = np.flatnonzero(gone)[:2]
    return m, nrm, smp, kind
