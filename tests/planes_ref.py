"""TEST REFERENCE for MSAC plane fitting and extraction on a prepared model (pcreg_model_fit_planes_f32's contract in
include/pcreg.h), in numpy and Python integers.

The fp32 scoring chain r = fmaf(nz, dz, fmaf(ny, dy, nx * dx)) is taken exactly: every product of two float32 is exact in float64,
every fmaf's sum is rounded to odd in float64 (TwoSum's residual says on which side the exact sum lies) and then once to float32,
as tests/iss_ref.py does it.  cost, count, the refit's n, S1, S2 and N = n S2 - S1 S1^T are Python integers; each entry of N is
rounded once to double and the refit's normal comes from numpy.linalg.eigh -- nothing here restates the library's Jacobi.

round_(m, alive, p, ...) runs ONE round from a given alive set; fit_planes(...) runs the whole extraction with eigh's normals;
classify(m, alive, normal, centre, t) restates the final classification from any (normal, centre), e.g. the RETURNED ones."""
from __future__ import annotations

import math

import numpy as np

QMAX = 1 << 20
MASK = (1 << 64) - 1
EPS = float(np.finfo(np.float64).eps)


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, exactly (see the module text)"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def thresholds(max_distance):
    """-> (t2, s) as float32: t2 = fl32(t * t), s = (float)(2^20 / (double)t2)"""
    t = np.float32(max_distance)
    t2 = np.float32(t * t)
    return t2, np.float32(float(QMAX) / float(t2))


def finite_rows(m) -> np.ndarray:
    return np.isfinite(np.asarray(m, np.float32).reshape(-1, 3)).all(axis=1)


def exponent(m) -> int:
    """frexp's exponent of the largest axis extent of the finite rows (0 where D == 0 or there is no finite row)"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    f = m[finite_rows(m)]
    if not len(f):
        return 0
    D = max(float(f[:, c].max()) - float(f[:, c].min()) for c in range(3))
    return math.frexp(D)[1] if D > 0 else 0


def chain_r2(rows, origin, nf) -> np.ndarray:
    """the contract's fp32 chain: r2 [N] float32 of rows [N, 3] against (origin, nf), both float32 [3]"""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    origin = np.asarray(origin, np.float32)
    nf = np.asarray(nf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = rows - origin[None, :]
        t = (nf[0].astype(np.float64) * d[:, 0].astype(np.float64)).astype(np.float32)
        r = _fma32(np.full(len(d), nf[2], np.float32), d[:, 2], _fma32(np.full(len(d), nf[1], np.float32), d[:, 1], t))
        return (r.astype(np.float64) * r.astype(np.float64)).astype(np.float32)


def q_of(r2, s) -> np.ndarray:
    """min(2^20, (int)rintf(r2 * s)) for the rows that pass; the caller masks"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.minimum(np.asarray(r2, np.float32) * np.float32(s), np.float32(QMAX))
        return np.rint(np.where(np.isfinite(v), v, 0)).astype(np.int64)


def sign_flip(n, ref_vec) -> bool:
    """True where the contract negates n (float64 [3])"""
    if ref_vec is not None:
        r = np.asarray(ref_vec, np.float64)
        return bool((n[0] * r[0] + n[1] * r[1]) + n[2] * r[2] < 0)
    c = 0
    if abs(n[1]) > abs(n[c]):
        c = 1
    if abs(n[2]) > abs(n[c]):
        c = 2
    return bool(n[c] < 0)


def trial_rows(p, B, b, seed, A):
    """the sampler: three original rows of the alive list A (ascending), or None where A is empty"""
    if len(A) == 0:
        return None
    return [int(A[splitmix64(seed ^ splitmix64(((p * B + b) * 4 + j) & MASK)) % len(A)]) for j in range(3)]


def hypothesis(m, alive, idx, ref_vec=None, max_angle=math.pi / 2):
    """-> (void, p0 float32 [3], nf float32 [3]) of the trial with the 0-based original rows idx (None: void)"""
    z = np.zeros(3, np.float32)
    M = len(m)
    if idx is None or any(i < 0 or i >= M for i in idx) or any(not alive[i] for i in idx):
        return True, z, z
    if idx[0] == idx[1] or idx[0] == idx[2] or idx[1] == idx[2]:
        return True, z, z
    q = m[list(idx)].astype(np.float64)
    a, b = q[1] - q[0], q[2] - q[0]
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)
        L2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    if not (L2 > 0) or not math.isfinite(L2):
        return True, m[idx[0]].copy(), z
    n = c / math.sqrt(L2)
    if sign_flip(n, ref_vec):
        n = -n
    if ref_vec is not None:
        r = np.asarray(ref_vec, np.float64)
        dot = (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2]
        rlen = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        if dot / rlen < math.cos(max_angle):
            return True, m[idx[0]].copy(), n.astype(np.float32)
    return False, m[idx[0]].copy(), n.astype(np.float32)


def classify(m, alive, normal, centre, max_distance) -> dict:
    """the final classification from (normal, centre) float64: mask [M] of the passing alive rows, count, Q and rmse"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    t2, s = thresholds(max_distance)
    rows = np.flatnonzero(alive)
    r2 = chain_r2(m[rows], np.asarray(centre, np.float64).astype(np.float32), np.asarray(normal, np.float64).astype(np.float32))
    with np.errstate(invalid="ignore"):
        ok = r2 <= t2
    mask = np.zeros(len(m), bool)
    mask[rows[ok]] = True
    count = int(ok.sum())
    Q = int(q_of(r2[ok], s).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = float(np.sqrt((np.float64(Q) / np.float64(count)) * (np.float64(t2) * 2.0 ** -20)))
    return dict(mask=mask, count=count, Q=Q, rmse=rmse)


def round_(m, alive, p, max_distance, n_trials, min_inliers=3, seed=0, samples=None, ref_vec=None, max_angle=math.pi / 2, e=None) -> dict:
    """ONE round of the contract from the alive set `alive` (bool [M]).  samples: 0-based rows [B, 3] of THIS round, or None.
    -> dict: void [B], cost [B] (Python ints), count [B], best_trial (-1: none), best_cost, best_count, stop; and, unless stop,
    n, S1, S2, N6 (float64: xx xy xz yy yz zz), normN, mu (ascending eigenvalues), normal (eigh's, signed), centre, d4"""
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
        v, p0, nf = hypothesis(m, alive, idx, ref_vec, max_angle)
        hyp.append((p0, nf))
        void[b] = v
        if v:
            continue
        r2 = chain_r2(rows, p0, nf)
        with np.errstate(invalid="ignore"):
            ok = r2 <= t2
        count[b] = int(ok.sum())
        cost[b] = int(q_of(r2[ok], s).sum()) + QMAX * int(len(A) - count[b])
    elig = [b for b in range(B) if not void[b] and count[b] >= 3]
    out = dict(void=void, cost=cost, count=count, e=e, alive_rows=A)
    if not elig:
        out.update(best_trial=-1, best_cost=0, best_count=0, stop=True)
        return out
    best = min(elig, key=lambda b: (cost[b], b))
    out.update(best_trial=best, best_cost=cost[best], best_count=int(count[best]), stop=bool(count[best] < min_inliers))
    if out["stop"]:
        return out
    p0, nf = hyp[best]
    r2 = chain_r2(rows, p0, nf)
    with np.errstate(invalid="ignore"):
        inl = rows[r2 <= t2]
    d = (inl - p0[None, :]).astype(np.float64) * 2.0 ** (17 - e)            # the fp32 differences, scaled exactly
    g = [[int(v) for v in row] for row in np.rint(d)]
    n = len(g)
    S1 = [sum(r[a] for r in g) for a in range(3)]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    S2 = [sum(r[a] * r[b] for r in g) for a, b in pairs]
    Nint = [n * S2[k] - S1[a] * S1[b] for k, (a, b) in enumerate(pairs)]
    N6 = np.array([float(v) for v in Nint], np.float64)                     # one rounding each
    Nm = np.array([[N6[0], N6[1], N6[2]], [N6[1], N6[3], N6[4]], [N6[2], N6[4], N6[5]]], np.float64)
    mu, V = np.linalg.eigh(Nm)
    normal = V[:, 0].copy()
    if sign_flip(normal, ref_vec):
        normal = -normal
    centre = p0.astype(np.float64) + (np.array([float(v) for v in S1], np.float64) / float(n)) * 2.0 ** -(17 - e)
    d4 = -((normal[0] * centre[0] + normal[1] * centre[1]) + normal[2] * centre[2])
    out.update(n=n, S1=S1, S2=S2, N6=N6, normN=float(np.linalg.norm(Nm)), mu=mu, normal=normal, centre=centre, d4=d4,
               max_g=max((abs(v) for r in g for v in r), default=0))
    return out


def plane_d(normal, centre) -> float:
    """d4 = -((nx cx + ny cy) + nz cz) in float64"""
    n, c = np.asarray(normal, np.float64), np.asarray(centre, np.float64)
    return float(-((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]))


def normal_bound(r) -> float:
    """asin(64 eps ||N||_F / (mu2 - mu3)): DESIGN 4.20's backward error of the Jacobi through Davis-Kahan; mu ascending here"""
    gap = float(r["mu"][1] - r["mu"][0])
    x = 64 * EPS * r["normN"] / gap if gap > 0 else np.inf
    return math.asin(x) if x < 1 else math.pi / 2


def angle(a, b) -> float:
    """the angle between the LINES of two unit vectors, accurate near 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.asin(min(1.0, float(np.linalg.norm(np.cross(a, b)))))


def fit_planes(m, max_distance, ref_vec=None, max_angle=math.pi / 2, max_planes=1, n_trials=100, min_inliers=3, seed=0, samples=None) -> dict:
    """the whole extraction with eigh's normals; samples 0-based [P, B, 3] or None"""
    m = np.asarray(m, np.float32).reshape(-1, 3)
    M, P = len(m), int(max_planes)
    alive = finite_rows(m) if M else np.zeros(0, bool)
    e = exponent(m)
    out = dict(n_planes=0, labels=np.zeros(M, np.int32), planes=np.zeros((P, 4)), centres=np.zeros((P, 3)), counts=np.zeros(P, np.int32),
               rmse=np.zeros(P), best_trial=np.zeros(P, np.int32), best_cost=np.zeros(P, np.int64), best_count=np.zeros(P, np.int32), rounds=[])
    if M == 0:
        return out
    for p in range(P):
        r = round_(m, alive, p, max_distance, n_trials, min_inliers, seed, None if samples is None else np.asarray(samples)[p], ref_vec,
                   max_angle, e)
        out["rounds"].append(r)
        out["best_trial"][p], out["best_cost"][p], out["best_count"][p] = r["best_trial"], r["best_cost"], r["best_count"]
        if r["stop"]:
            break
        c = classify(m, alive, r["normal"], r["centre"], max_distance)
        out["labels"][c["mask"]] = p + 1
        alive = alive & ~c["mask"]
        out["planes"][p] = [*r["normal"], r["d4"]]
        out["centres"][p] = r["centre"]
        out["counts"][p] = c["count"]
        out["rmse"][p] = c["rmse"]
        out["n_planes"] = p + 1
    return out


def lattice_scene():
    """a 32 x 32 lattice in z = 7 plus 200 off-plane rows (tests/test_planes_ref.py)"""
    g = np.arange(32, dtype=np.float32)
    plane = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    rng = np.random.default_rng(5)
    off = np.column_stack([rng.uniform(0, 31, 200), rng.uniform(0, 31, 200), rng.uniform(9, 30, 200)]).astype(np.float32)
    return np.vstack([plane, off])


def scene(M: int, seed: int = 11) -> np.ndarray:
    """three noisy planes of 40 %, 25 % and 15 % of the rows (sigma 0.02, extent 20) plus uniform clutter, offset (100, 50, 90), rows
    shuffled -> float32 [M, 3]"""
    rng = np.random.default_rng(seed)
    n1, n2, n3 = int(0.40 * M), int(0.25 * M), int(0.15 * M)
    nc = M - n1 - n2 - n3
    frames = [((0.0, 0.0, 1.0), 4.0), ((1.0, 0.2, 0.1), 9.0), ((-0.3, 1.0, 0.4), 13.0)]
    parts = []
    for (nrm, off), n in zip(frames, (n1, n2, n3)):
        nrm = np.array(nrm) / np.linalg.norm(nrm)
        u = np.cross(nrm, [0.3, 0.5, 0.8])
        u /= np.linalg.norm(u)
        w = np.cross(nrm, u)
        ab = rng.uniform(-10, 10, (n, 2))
        parts.append(ab[:, :1] * u + ab[:, 1:] * w + (off - 10.0 + rng.normal(0, 0.02, (n, 1))) * nrm + 10.0)
    parts.append(rng.uniform(0, 20, (nc, 3)))
    pts = np.vstack(parts) + np.array([100.0, 50.0, 90.0])
    return pts[rng.permutation(M)].astype(np.float32)
