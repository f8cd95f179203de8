"""TEST REFERENCE of the point-to-plane refit (pcreg_model_refit_plane_f32's contract, include/pcreg.h).

The pairs come from tests/score_ref.py, as tests/refit_ref.py takes them: float64 transformed queries rounded once, the
brute-force fp32 nearest row, the `<= r2` filter.  The normals are an input.  The 28 sums are taken in numpy.longdouble (numpy's
pairwise summation, not the library's tree), the 6 x 6 scaled Cholesky by hand in longdouble, the Cayley rotation in longdouble
and rounded to double at the end.  The composition is refit_ref.compose.  The origin is the contract's: the middle of the model's
bounding box in fp32, 0.5f * lo + 0.5f * hi.

origin(model)                      -> [3] float64
plane_sums(model, normals, idx_b, tq_b, o) -> (sums [28] longdouble, n_plane); sums_of_pairs(m, p, n, o) the same of given pairs
fit(sums, n_plane, o)              -> (T_step [4, 4] float64 as quickTF uses it, or None when the contract says empty; the smallest
                                       pivot of the scaled matrix, NaN when the factorisation was not reached)
step(q, model, normals, T, r2)     -> refit_ref.step's dict plus n_plane [B], sum_res2 [B], pivot [B]
finish64(sums, n_plane, o)         -> the 16 doubles of T_step in the library's layout, or None: the float64 restatement of
                                       pcreg_amd/csrc/plane_fit.hpp in the header's order, operation by operation
scene()                            -> the GPU test's main scene, shared with the CPU premises in tests/test_plane_ref.py
"""
from __future__ import annotations

import math

import numpy as np

import refit_ref
import score_ref

LD = np.longdouble
MIN_PIVOT = 2.0 ** -26
MIN_PAIRS = 6


def origin(model):
    m = np.asarray(model, np.float32).reshape(-1, 3)
    if len(m) == 0:
        return np.zeros(3)
    lo, hi = m.min(axis=0), m.max(axis=0)
    return (np.float32(0.5) * lo + np.float32(0.5) * hi).astype(np.float64)


def tri(i, j):
    """the place of A_ij (i <= j) among the sums: the upper triangle row-major"""
    return i * 6 - i * (i - 1) // 2 + (j - i)


def plane_pairs(model, normals, idx_b, tq_b):
    """-> (m, p, n) [n_plane, 3] float64 each: the pairs of one transform whose row has a finite normal, in ascending query order"""
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    hit = np.flatnonzero(np.asarray(idx_b) >= 0)
    rows = np.asarray(idx_b)[hit]
    ok = np.isfinite(nrm[rows]).all(axis=1) if len(hit) else np.zeros(0, bool)
    hit, rows = hit[ok], rows[ok]
    return (np.asarray(model, np.float32).reshape(-1, 3)[rows].astype(np.float64), np.asarray(tq_b, np.float32)[hit].astype(np.float64),
            nrm[rows].astype(np.float64))


def plane_sums(model, normals, idx_b, tq_b, o):
    return sums_of_pairs(*plane_pairs(model, normals, idx_b, tq_b), o)


def sums_of_pairs(m, p, n, o):
    """the 28 sums of given plane pairs (model rows m, moved points p, normals n: [n_plane, 3] float64 each) -> (sums, n_plane)"""
    m, p, n = (np.asarray(a, np.float64).reshape(-1, 3).astype(LD) for a in (m, p, n))
    o = np.asarray(o, np.float64).astype(LD)
    sums = np.zeros(28, LD)
    if len(m) == 0:
        return sums, 0
    r = ((p - m) * n).sum(axis=1)
    J = np.concatenate([np.cross(p - o, n), n], axis=1)
    for i in range(6):
        for j in range(i, 6):
            sums[tri(i, j)] = (J[:, i] * J[:, j]).sum()
        sums[21 + i] = (J[:, i] * r).sum()
    sums[27] = (r * r).sum()
    return sums, len(m)


def fit(sums, n_plane, o):
    sums = np.asarray(sums, LD)
    o = np.asarray(o, np.float64).astype(LD)
    nan = float("nan")
    if n_plane < MIN_PAIRS:
        return None, nan
    diag = np.array([sums[tri(i, i)] for i in range(6)], LD)
    if not (np.isfinite(diag).all() and (diag > 0).all()):
        return None, nan
    s = np.sqrt(diag)
    Cm = np.ones((6, 6), LD)
    for i in range(6):
        for j in range(i + 1, 6):
            Cm[i, j] = Cm[j, i] = sums[tri(i, j)] / (s[i] * s[j])
    L = np.zeros((6, 6), LD)
    pivot = LD(np.inf)
    for i in range(6):
        for j in range(i):
            L[i, j] = (Cm[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
        p = Cm[i, i] - (L[i, :i] * L[i, :i]).sum()
        pivot = min(pivot, p) if p == p else LD(np.nan)
        if not p > MIN_PIVOT:
            return None, float(pivot)
        L[i, i] = np.sqrt(p)
    b = -sums[21:27] / s
    y = np.zeros(6, LD)
    for i in range(6):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    z = np.zeros(6, LD)
    for i in range(5, -1, -1):
        z[i] = (y[i] - (L[i + 1:, i] * z[i + 1:]).sum()) / L[i, i]
    x = z / s
    if not np.isfinite(x).all():
        return None, float(pivot)
    h = x[:3] / 2
    S = np.sqrt(1 + (h * h).sum())
    a, bq, c, d = LD(1) / S, h[0] / S, h[1] / S, h[2] / S
    R = np.array([[1 - 2 * (c * c + d * d), 2 * (bq * c - a * d), 2 * (bq * d + a * c)],
                  [2 * (bq * c + a * d), 1 - 2 * (bq * bq + d * d), 2 * (c * d - a * bq)],
                  [2 * (bq * d - a * c), 2 * (c * d + a * bq), 1 - 2 * (bq * bq + c * c)]], LD)
    T = np.zeros((4, 4), LD)
    T[:3, :3] = R.T                                          # [p, 1] @ T: the row-vector form of p -> R (p - o) + o + t
    T[3, :3] = o + x[3:] - R @ o
    T[3, 3] = 1
    T = T.astype(np.float64)
    if not np.isfinite(T).all():
        return None, float(pivot)
    return T, float(pivot)


def step(q, model, normals, T, r2, threads=None):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tq = score_ref.transformed(q, T)
    B, Q = tq.shape[:2]
    if len(model) and Q:
        idx, dist = score_ref.within(*score_ref.nearest(tq.reshape(-1, 3), model, threads=threads), r2)
    else:
        idx, dist = np.full(B * Q, -1, np.int32), np.full(B * Q, np.inf, np.float32)
    idx, dist = idx.reshape(B, Q), dist.reshape(B, Q)
    n_close, sum_d2 = score_ref.sums(idx, dist)
    o = origin(model)
    T_step, T_out, empty = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.ones(B, bool)
    n_plane, sum_res2, pivot = np.zeros(B, np.int32), np.zeros(B), np.full(B, np.nan)
    for b in range(B):
        sums, n_plane[b] = plane_sums(model, normals, idx[b], tq[b], o)
        sum_res2[b] = float(sums[27])
        S, pivot[b] = fit(sums, n_plane[b], o) if T[b].any() else (None, np.nan)
        if S is not None:
            T_step[b], T_out[b], empty[b] = S, refit_ref.compose(T[b], S), False
    return dict(T_step=T_step, T_out=T_out, empty=empty, hit=idx >= 0, idx=idx, tq=tq, n_close=n_close, sum_d2=sum_d2, n_plane=n_plane,
                sum_res2=sum_res2, pivot=pivot)


def finish64(sums, n_plane, o):
    """plane_fit.hpp in float64, one operation per operation (Python floats are IEEE doubles, never contracted)"""
    A = [float(v) for v in sums]
    o = [float(v) for v in o]
    fin = lambda v: v - v == 0.0
    if n_plane < MIN_PAIRS:
        return None
    s = [0.0] * 6
    for i in range(6):
        a = A[tri(i, i)]
        if not a > 0.0 or not fin(a):
            return None
        s[i] = math.sqrt(a)
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i):
            v = A[tri(j, i)] / (s[j] * s[i])
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
        p = 1.0
        for k in range(i):
            p = p - L[i][k] * L[i][k]
        if not p > MIN_PIVOT:
            return None
        L[i][i] = math.sqrt(p)
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = -A[21 + i] / s[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    for i in range(6):
        x[i] = x[i] / s[i]
        if not fin(x[i]):
            return None
    hx, hy, hz = x[0] / 2.0, x[1] / 2.0, x[2] / 2.0
    S = math.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    a, b, c, d = 1.0 / S, hx / S, hy / S, hz / S
    R = [[1.0 - 2.0 * (c * c + d * d), 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
         [2.0 * (b * c + a * d), 1.0 - 2.0 * (b * b + d * d), 2.0 * (c * d - a * b)],
         [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), 1.0 - 2.0 * (b * b + c * c)]]
    out = [0.0] * 16
    for j in range(3):
        for i in range(3):
            out[4 * j + i] = R[j][i]
        out[4 * j + 3] = (o[j] + x[3 + j]) - ((R[j][0] * o[0] + R[j][1] * o[1]) + R[j][2] * o[2])
    out[15] = 1.0
    if not all(fin(v) for v in out[:12]):
        return None
    return np.array(out, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the main scene
def rigid(eul, shift):
    from oracle.pcreg_oracle import eul2rotm
    T = np.eye(4)
    T[:3, :3] = eul2rotm(eul)
    T[3, :3] = shift
    return T


def about(P, c):
    """the rigid P applied about the point c: shift c to the origin, apply P, shift back ([p, 1] @ result)"""
    A, B = np.eye(4), np.eye(4)
    A[3, :3], B[3, :3] = -np.asarray(c, np.float64), np.asarray(c, np.float64)
    return A @ P @ B


def sheet_samples(n, seed, lo=4.0, hi=36.0):
    """n other samples of normals_ref's sheet (the same surface and noise), with (u, v) inside [lo, hi]^2: the interior"""
    import normals_ref
    rng = np.random.default_rng(seed)
    u = rng.uniform(lo, hi, (n, 2))
    z = 3 * np.sin(u[:, 0] / 5) * np.cos(u[:, 1] / 7) + rng.normal(0, 0.05, n)
    return np.column_stack([u, z]) + normals_ref.OFFSET


PERTURBATIONS = ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]), ([0.004, -0.003, 0.005], [0.05, -0.04, 0.03]), ([0.01, 0.008, -0.012], [0.15, 0.1, -0.12]), \
    ([0.03, -0.02, 0.025], [0.4, -0.3, 0.35])                    # tests/test_gpu_refit.py's four
K_NORMALS = 8
_SCENE = {}


def scene():
    """model: normals_ref.family("sheet", 4096), 8 tiles.  cloud: 2500 other samples of the sheet's interior (two chunks, five query
    blocks), in the model's frame -- the surface's TRUE PLACE.  surf: the cloud moved by the rigid G, fp32.  T: invertTF(G) times
    the four perturbations, each applied about the cloud's centroid (the sheet lies 170 units from the coordinate origin, where a
    rotation about the origin would be a large shift), then the empty transform and one with a NaN entry.  normals: normals_ref
    at k = 8 with the contract's sign, rounded to fp32."""
    if _SCENE:
        return _SCENE
    import normals_ref
    from oracle.pcreg_oracle import invertTF
    model = normals_ref.family("sheet", 4096)
    cloud = sheet_samples(2500, 11)
    G = rigid([0.3, -0.2, 0.5], [4, -3, 2])
    surf = (cloud @ G[:3, :3] + G[3, :3]).astype(np.float32)
    back = invertTF(G)
    c = cloud.mean(axis=0)
    T = np.stack([back @ about(rigid(*p), c) for p in PERTURBATIONS] + [np.zeros((4, 4)), back.copy()])
    T[5, 1, 2] = np.nan
    normals = normals_ref.oriented(normals_ref.normals(model, K_NORMALS), model).astype(np.float32)
    _SCENE.update(model=model, cloud=cloud, surf=surf, T=T, normals=normals, ref={})
    return _SCENE


def scene_ref(r2, threads=None):
    sc = scene()
    key = float(r2)
    if key not in sc["ref"]:
        sc["ref"][key] = step(sc["surf"], sc["model"], sc["normals"], sc["T"], r2, threads=threads)
    return sc["ref"][key]


def rms_to_truth(surf, T, cloud):
    """the RMS distance of the surface moved by T ([p, 1] @ T, float64) from its true place"""
    moved = np.asarray(surf, np.float64) @ T[:3, :3] + T[3, :3]
    return float(np.sqrt(((moved - cloud) ** 2).sum(axis=1).mean()))
