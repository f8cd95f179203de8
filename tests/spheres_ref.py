"""TEST REFERENCE for MSAC sphere fitting and extraction on a prepared model (pcreg_model_fit_spheres_f32's contract in
include/pcreg.h), in numpy and Python integers.

The fp32 scoring chain d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), rho = sqrt(d2), r = rho - Rf, r2 = r * r is taken exactly: each fmaf
by tests/planes_ref.py's round-to-odd construction, the root by numpy.sqrt on float32 (IEEE: correctly rounded).  The trial's
circumsphere is float64, operation by operation (a Python float operation is one correctly rounded double operation).  cost, count
and the refit's seventeen sums are Python integers; N = n S2 - S1 S1^T and h = n (sum g w) - S1 (sum w) are Python integers rounded
once by float(int).  finish64 restates pcreg_amd/csrc/sphere_fit.hpp in float64; finish_exact solves the same rounded system in
fractions.Fraction.

round_(m, alive, p, ...) runs ONE round from a given alive set; fit_spheres(...) the whole extraction; classify(m, alive, centre, R,
t) restates the final classification from any sphere, e.g. the RETURNED one."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from planes_ref import EPS, MASK, QMAX, _fma32, exponent, finite_rows, q_of, splitmix64, thresholds  # noqa: F401

SPLIT = 18
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def chain_r2(rows, cf, Rf) -> np.ndarray:
    """the contract's fp32 chain: r2 [N] float32 of rows [N, 3] against the sphere (cf float32 [3], Rf float32)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    cf = np.asarray(cf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = rows - cf[None, :]
        t = (d[:, 0].astype(np.float64) * d[:, 0].astype(np.float64)).astype(np.float32)
        d2 = _fma32(d[:, 2], d[:, 2], _fma32(d[:, 1], d[:, 1], t))
        rho = np.sqrt(d2)                                                   # float32 in, float32 out: correctly rounded
        r = (rho - np.float32(Rf)).astype(np.float32)
        return (r.astype(np.float64) * r.astype(np.float64)).astype(np.float32)


def trial_rows(p, B, b, seed, A):
    """the sampler: four original rows of the alive list A (ascending), or None where A is empty"""
    if len(A) == 0:
        return None
    return [int(A[splitmix64(seed ^ splitmix64(((p * B + b) * 4 + j) & MASK)) % len(A)]) for j in range(4)]


def _f32(v) -> np.float32:
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(v)


def _sqrt(v: float) -> float:
    return math.sqrt(v) if v >= 0 else math.nan                            # (NaN in, NaN out: NaN >= 0 is False)


def _div(a: float, b: float) -> float:
    """IEEE a / b in float64 (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def circumsphere(q):
    """the contract's trial geometry from four rows q [4, 3] (float32), in float64 operation by operation
    -> (det, u [3], R) as Python floats; u and R are None where det is zero or not finite"""
    q = [[float(v) for v in row] for row in np.asarray(q, np.float32)]
    d = [[q[i][c] - q[0][c] for c in range(3)] for i in (1, 2, 3)]
    b = [(di[0] * di[0] + di[1] * di[1]) + di[2] * di[2] for di in d]

    def cross(a, c):
        return [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]]

    X = [cross(d[1], d[2]), cross(d[2], d[0]), cross(d[0], d[1])]
    det = (d[0][0] * X[0][0] + d[0][1] * X[0][1]) + d[0][2] * X[0][2]
    if det == 0 or not math.isfinite(det):
        return det, None, None
    den = 2.0 * det
    u = [_div((b[0] * X[0][c] + b[1] * X[1][c]) + b[2] * X[2][c], den) for c in range(3)]
    R = _sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return det, u, R


def hypothesis(m, alive, idx, min_radius=0.0, max_radius=math.inf):
    """-> (void, p0 float32 [3], cf float32 [3], Rf float32) of the trial with the 0-based original rows idx (None: void)"""
    z = np.zeros(3, np.float32)
    M = len(m)
    if idx is None or any(i < 0 or i >= M for i in idx) or any(not alive[i] for i in idx):
        return True, z, z, np.float32(0)
    if len(set(idx)) != 4:
        return True, z, z, np.float32(0)
    q = m[list(idx)]
    p0 = q[0].copy()
    det, u, R = circumsphere(q)
    if u is None or not all(math.isfinite(v) for v in u) or not math.isfinite(R):
        return True, p0, z, np.float32(0)
    cf = np.array([_f32(float(p0[c]) + u[c]) for c in range(3)], np.float32)
    Rf = _f32(R)
    if not np.isfinite(cf).all() or not np.isfinite(Rf) or Rf < np.float32(min_radius) or Rf > np.float32(max_radius):
        return True, p0, z, np.float32(0)
    return False, p0, cf, Rf


def classify(m, alive, centre, R, max_distance) -> dict:
    """the final classification from (centre float64 [3], R float64): mask [M] of the passing alive rows, count, Q and rmse"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    t2, s = thresholds(max_distance)
    rows = np.flatnonzero(alive)
    r2 = chain_r2(m[rows], np.asarray(centre, np.float64).astype(np.float32), _f32(np.float64(R)))
    with np.errstate(invalid="ignore"):
        ok = r2 <= t2
    mask = np.zeros(len(m), bool)
    mask[rows[ok]] = True
    count = int(ok.sum())
    Q = int(q_of(r2[ok], s).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = float(np.sqrt((np.float64(Q) / np.float64(count)) * (np.float64(t2) * 2.0 ** -20)))
    return dict(mask=mask, count=count, Q=Q, rmse=rmse, r2=r2, rows=rows)


def integer_sums(g):
    """the seventeen sums of the quantised differences g (rows of three Python ints) -> a list of 17 Python ints:
    n, S1 [3], S2 [6], sum w, sum g w_lo [3], sum g w_hi [3]"""
    n = len(g)
    S1 = [sum(r[a] for r in g) for a in range(3)]
    S2 = [sum(r[a] * r[b] for r in g) for a, b in PAIRS]
    w = [r[0] * r[0] + r[1] * r[1] + r[2] * r[2] for r in g]
    lo = [v & ((1 << SPLIT) - 1) for v in w]
    hi = [v >> SPLIT for v in w]
    return ([n] + S1 + S2 + [sum(w)] + [sum(r[a] * l for r, l in zip(g, lo)) for a in range(3)]
            + [sum(r[a] * h for r, h in zip(g, hi)) for a in range(3)])


def normal_equations(S):
    """(N6, h, S1, sw, n) as float64, each entry of N and h formed exactly as a Python integer and rounded ONCE by float(int)"""
    n, S1, S2, sw = S[0], S[1:4], S[4:10], S[10]
    gw = [S[14 + k] * (1 << SPLIT) + S[11 + k] for k in range(3)]
    N6 = [float(n * S2[k] - S1[a] * S1[b]) for k, (a, b) in enumerate(PAIRS)]
    h = [float(n * gw[k] - S1[k] * sw) for k in range(3)]
    return N6, h, [float(v) for v in S1], float(sw), float(n)


def _radicand_ok(v: float) -> bool:
    return v > 0 and math.isfinite(v)


def finish64(N6, h, S1, sw, n, p0, back, min_radius=0.0, max_radius=math.inf) -> dict:
    """pcreg_amd/csrc/sphere_fit.hpp restated in float64, operation by operation -> dict(used, centre [3], R, a [3], Rg2); p0 three
    floats (the trial's first row widened), back = 2^-(17 - e)"""
    N6, h, S1, p0 = ([float(v) for v in x] for x in (N6, h, S1, p0))
    sw, n, back = float(sw), float(n), float(back)
    out = dict(used=False, centre=None, R=None, a=None, Rg2=None)
    r0 = N6[0]
    if not _radicand_ok(r0):
        return out
    L00 = math.sqrt(r0)
    L10 = _div(N6[1], L00)
    L20 = _div(N6[2], L00)
    r1 = N6[3] - L10 * L10
    if not _radicand_ok(r1):
        return out
    L11 = math.sqrt(r1)
    L21 = _div(N6[4] - L20 * L10, L11)
    r2 = (N6[5] - L20 * L20) - L21 * L21
    if not _radicand_ok(r2):
        return out
    L22 = math.sqrt(r2)
    y0 = _div(h[0], L00)
    y1 = _div(h[1] - L10 * y0, L11)
    y2 = _div((h[2] - L20 * y0) - L21 * y1, L22)
    a2 = _div(y2, L22)
    a1 = _div(y1 - L21 * a2, L11)
    a0 = _div((y0 - L10 * a1) - L20 * a2, L00)
    cx, cy, cz = a0 / 2.0, a1 / 2.0, a2 / 2.0
    beta = _div(sw - ((a0 * S1[0] + a1 * S1[1]) + a2 * S1[2]), n)
    Rg2 = beta + ((cx * cx + cy * cy) + cz * cz)
    out.update(a=[a0, a1, a2], Rg2=Rg2)
    if not _radicand_ok(Rg2):
        return out
    centre = [p0[0] + cx * back, p0[1] + cy * back, p0[2] + cz * back]
    R = math.sqrt(Rg2) * back
    if not all(math.isfinite(v) for v in centre) or not math.isfinite(R):
        return out
    Rf = _f32(R)
    if not (Rf >= np.float32(min_radius) and Rf <= np.float32(max_radius)):
        return out
    out.update(used=True, centre=centre, R=R)
    return out


def finish_exact(N6, h):
    """N a = h solved exactly for the SAME rounded doubles -> a as three Fractions (None where N is singular)"""
    N = [[Fraction(N6[0]), Fraction(N6[1]), Fraction(N6[2])], [Fraction(N6[1]), Fraction(N6[3]), Fraction(N6[4])],
         [Fraction(N6[2]), Fraction(N6[4]), Fraction(N6[5])]]
    hv = [Fraction(v) for v in h]

    def det3(A):
        return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
                + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))

    D = det3(N)
    if D == 0:
        return None
    out = []
    for k in range(3):                                                       # Cramer's rule: exact in Fractions
        A = [[hv[i] if j == k else N[i][j] for j in range(3)] for i in range(3)]
        out.append(det3(A) / D)
    return out


def kappa2(N6) -> float:
    Nm = np.array([[N6[0], N6[1], N6[2]], [N6[1], N6[3], N6[4]], [N6[2], N6[4], N6[5]]], np.float64)
    ev = np.linalg.eigvalsh(Nm)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else math.inf


def round_(m, alive, p, max_distance, n_trials, min_inliers=4, seed=0, samples=None, min_radius=0.0, max_radius=math.inf, e=None) -> dict:
    """ONE round of the contract from the alive set `alive` (bool [M]).  samples: 0-based rows [B, 4] of THIS round, or None.
    -> dict: void [B], cost [B] (Python ints), count [B], best_trial (-1: none), best_cost, best_count, stop; and, unless stop,
    trial (p0, cf, Rf), sums (17 Python ints), N6, h, S1, sw, n, fit (finish64's dict), used, centre [3], R (the round's sphere)"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
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
        v, p0, cf, Rf = hypothesis(m, alive, idx, min_radius, max_radius)
        hyp.append((p0, cf, Rf))
        void[b] = v
        if v:
            continue
        r2 = chain_r2(rows, cf, Rf)
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
    p0, cf, Rf = hyp[best]
    r2 = chain_r2(rows, cf, Rf)
    with np.errstate(invalid="ignore"):
        inl = rows[r2 <= t2]
    d = (inl - p0[None, :]).astype(np.float64) * 2.0 ** (17 - e)            # the fp32 differences, scaled exactly
    g = [[int(v) for v in row] for row in np.rint(d)]
    S = integer_sums(g)
    N6, h, S1, sw, n = normal_equations(S)
    fit = finish64(N6, h, S1, sw, n, [float(v) for v in p0], 2.0 ** -(17 - e), min_radius, max_radius)
    if fit["used"]:
        centre, R = fit["centre"], fit["R"]
    else:
        centre, R = [float(v) for v in cf], float(Rf)
    out.update(trial=(p0, cf, Rf), sums=S, N6=N6, h=h, S1=S1, sw=sw, n=n, fit=fit, used=bool(fit["used"]), centre=centre, R=R,
               max_g=max((abs(v) for r in g for v in r), default=0))
    return out


def fit_spheres(m, max_distance, min_radius=0.0, max_radius=math.inf, max_spheres=1, n_trials=100, min_inliers=4, seed=0, samples=None) -> dict:
    """the whole extraction; samples 0-based [P, B, 4] or None"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    M, P = len(m), int(max_spheres)
    alive = finite_rows(m) if M else np.zeros(0, bool)
    e = exponent(m)
    out = dict(n_spheres=0, labels=np.zeros(M, np.int32), spheres=np.zeros((P, 4)), counts=np.zeros(P, np.int32), rmse=np.zeros(P),
               refit_used=np.zeros(P, np.int32), best_trial=np.zeros(P, np.int32), best_cost=np.zeros(P, np.int64),
               best_count=np.zeros(P, np.int32), rounds=[])
    if M == 0:
        return out
    for p in range(P):
        r = round_(m, alive, p, max_distance, n_trials, min_inliers, seed, None if samples is None else np.asarray(samples)[p], min_radius,
                   max_radius, e)
        out["rounds"].append(r)
        out["best_trial"][p], out["best_cost"][p], out["best_count"][p] = r["best_trial"], r["best_cost"], r["best_count"]
        if r["stop"]:
            break
        c = classify(m, alive, r["centre"], r["R"], max_distance)
        out["labels"][c["mask"]] = p + 1
        alive = alive & ~c["mask"]
        out["spheres"][p] = [*r["centre"], r["R"]]
        out["counts"][p] = c["count"]
        out["rmse"][p] = c["rmse"]
        out["refit_used"][p] = int(r["used"])
        out["n_spheres"] = p + 1
    return out


SCENE_SPHERES = (((6.0, 6.0, 7.0), 5.0), ((14.0, 13.0, 5.0), 3.0), ((5.0, 15.0, 15.0), 2.0))
SCENE_OFFSET = (100.0, 50.0, 90.0)


def scene(M: int, seed: int = 11) -> np.ndarray:
    """three noisy sphere surfaces of radii 5, 3 and 2 with 40 %, 25 % and 15 % of the rows (radial sigma 0.02; the second only the
    hemisphere facing +z, as a stereo view sees it) plus uniform clutter in a box of extent 20, offset (100, 50, 90), rows shuffled
    -> float32 [M, 3]"""
    rng = np.random.default_rng(seed)
    ns = (int(0.40 * M), int(0.25 * M), int(0.15 * M))
    nc = M - sum(ns)
    parts = []
    for k, ((c, R), n) in enumerate(zip(SCENE_SPHERES, ns)):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        if k == 1:
            v[:, 2] = np.abs(v[:, 2])
        parts.append(np.array(c) + v * (R + rng.normal(0, 0.02, (n, 1))))
    parts.append(rng.uniform(0, 20, (nc, 3)))
    pts = np.vstack(parts) + np.array(SCENE_OFFSET)
    return pts[rng.permutation(M)].astype(np.float32)


# ---- the knife edge: rows exactly on a sphere of radius 9 about (16, 32, 8), and pairs on the x axis about R + t ---------------------
KNIFE_C, KNIFE_R, KNIFE_T = (16.0, 32.0, 8.0), 9.0, 0.0625


def knife_scene():
    """-> (m float32 [n + 6, 3], n): n lattice rows at EXACTLY radius 9 (every signed permutation of the integer triples with squares
    adding up to 81), then three pairs (cx + d, cx - d) on the x axis with d = R + t, the float below it (as a coordinate of the row
    at cx + d) and the float above it: r2 == t2 exactly for the first pair"""
    import itertools
    dirs = set()
    for tri in ((9, 0, 0), (1, 4, 8), (4, 4, 7), (3, 6, 6)):
        for perm in itertools.permutations(tri):
            for sg in itertools.product((1, -1), repeat=3):
                dirs.add(tuple(a * b for a, b in zip(perm, sg)))
    lat = np.array(sorted(dirs), np.float32) + np.array(KNIFE_C, np.float32)
    step = float(np.spacing(np.float32(KNIFE_C[0] + KNIFE_R + KNIFE_T)))      # one float at cx + R + t (2^-19); cx - d holds it too
    ds = [KNIFE_R + KNIFE_T, KNIFE_R + KNIFE_T - step, KNIFE_R + KNIFE_T + step]
    knife = np.array([[KNIFE_C[0] + sg * d, KNIFE_C[1], KNIFE_C[2]] for d in ds for sg in (1, -1)], np.float64)
    assert np.array_equal(knife.astype(np.float32).astype(np.float64), knife)
    return np.vstack([lat, knife.astype(np.float32)]), len(lat)


# ---- shared cases of tests/test_spheres_ref.py (their premises, on the CPU) and tests/test_gpu_fit_spheres.py ------------------------
SCENES = ((1030, 256, 40), (4096, 256, 200))                                  # M, B, min_inliers; t = 0.08, P = 5, seed 7
SCENE_T, SCENE_P, SCENE_SEED = 0.08, 5, 7
COPLANAR = ((100.0, 50.0, 90.0), (101.0, 50.0, 90.0), (100.0, 51.0, 90.0), (101.0, 51.0, 90.0))


def sample_table(M, labels, P, B, seed):
    """a caller's table [P, B, 4] of 0-based rows: in every round B / 8 trials drawn within each of the rows labelled 1, 2 and 3 (four
    different rows each), the rest uniformly among all rows"""
    rng = np.random.default_rng(seed)
    smp = rng.integers(0, M, (P, B, 4)).astype(np.int32)
    for p in range(P):
        for k in (1, 2, 3):
            rows = np.flatnonzero(np.asarray(labels) == k)
            for b in range((k - 1) * (B // 8), k * (B // 8)):
                smp[p, b] = rng.choice(rows, 4, replace=False)
    return smp


def bad_sample_scene(labels_1030):
    """-> (m, smp): the 1030-row scene with four exactly coplanar rows written over rows 0 .. 3 of its clutter, and a table [3, 256, 4]
    whose first trials are an equal pair, an index past the end, an index below 0 and the coplanar four; trial 4 of rounds 1 and 2
    names a row that round 0 removes.  labels_1030: the labels of the plain scene's extraction (who is on which sphere)"""
    m = np.array(scene(1030))
    clutter = np.flatnonzero(np.asarray(labels_1030) == 0)[:4]
    m[clutter] = np.array(COPLANAR, np.float32)
    M = len(m)
    smp = sample_table(M, labels_1030, 3, 256, 21)
    others = [int(v) for v in np.flatnonzero(np.asarray(labels_1030) == 1)[:8]]
    smp[:, 0] = [others[0], others[1], others[0], others[2]]                  # an equal pair
    smp[:, 1] = [others[0], others[1], others[2], M]                          # an index out of range, above
    smp[:, 2] = [-1, others[1], others[2], others[3]]                         # ... and below
    smp[:, 3] = clutter                                                       # det == 0
    smp[1:, 4] = others[4:8]                                                  # rows of sphere 1: round 0 removes them
    return m, smp
