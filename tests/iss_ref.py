"""TEST REFERENCE for the ISS keypoints of a prepared model (pcreg_model_iss_f32's contract in include/pcreg.h).

Brute force.  The neighbourhood is the fp32 predicate fmaf(dz, dz, fmaf(dy, dy, dx*dx)) <= r2 on every pair (each fmaf exactly: the
product and the sum in float64, rounded to odd, then once to float32).  iss() takes the contract's integers q as Python integers:
n, S1, S2 and N = n S2 - S1 S1^T are exact, each entry of N is rounded once to double, its eigenvalues come from
numpy.linalg.eigvalsh (nothing here restates the library's Jacobi; a coordinate whose row of N is zero is split off first, so an
exact zero stays one), and every decision -- the ratio tests, the saliency order, the ties -- is made in numpy.longdouble.
iss(..., quantised=False) is the UNQUANTISED variant: the differences in longdouble, the covariance about the mean, for the
quantisation bound of tests/test_iss_ref.py.

iss(model, r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors) -> dict with, per row,
  n [M]  mu [M, 3] longdouble, descending, in N's units (NaN for a non-finite row)   lam [M, 3] longdouble, the reported eigenvalues
  N [M, 6] float64 (xx, xy, xz, yy, yz, zz)   normN [M] its Frobenius norm   cand [M] bool   s [M] longdouble
  key [M] bool and keypoints (ascending rows)   sensitive [M], excluded [M] bool   e, the contract's exponent
A row is SENSITIVE if n >= min_neighbors and one of the candidate tests (mu2 < g21 mu1, mu3 < g32 mu2, mu3 > 0) lies within
TOL mu1 of equality, or a nonmax neighbour that is also a candidate has |s_i - s_j| <= TOL max(s_i, s_j) -- unless the two have
identical (n, N), an exact tie in any arithmetic; a zero that the split made exact is not sensitive either.  A row is EXCLUDED if
it is sensitive or has a sensitive nonmax neighbour."""
from __future__ import annotations

import math

import numpy as np

import normals_ref

L = np.longdouble
TOL = 1e-9
EXCLUDED_CAP = 0.01
M_FAMILY = 2048
RADII = ((3.0, 2.0), (2.0, 2.0), (4.0, 3.0))          # (salient, nonmax)
GAMMA21 = GAMMA32 = 0.975
MIN_NEIGHBORS = 5
EPS = float(np.finfo(np.float64).eps)


def r2_of(radius) -> np.float32:
    """the wrappers' rule: the radius squared in double, the square rounded once to float32"""
    return np.float32(float(radius) * float(radius))


def _fmaf(a, c):
    """fmaf(a, a, c) for float32 arrays, exactly: a*a is exact in float64; the sum is rounded to odd in float64 (TwoSum's
    residual says on which side the exact sum lies), so the second rounding, to float32, is the only one that counts"""
    p = a.astype(np.float64) * a.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def d2_matrix(model) -> np.ndarray:
    """[M, M] float32: the chain distance from row i (axis 0) to row j (axis 1), dx = m_j - m_i"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = m[None, :, 0] - m[:, None, 0]
        dy = m[None, :, 1] - m[:, None, 1]
        dz = m[None, :, 2] - m[:, None, 2]
        t = (dx.astype(np.float64) * dx.astype(np.float64)).astype(np.float32)
        return _fmaf(dz, _fmaf(dy, t))


def adjacency(model, r2) -> np.ndarray:
    """[M, M] bool: j is in the neighbourhood of i (i itself included); a non-finite row is in none and has none"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    fin = np.isfinite(m).all(axis=1)
    with np.errstate(invalid="ignore"):
        adj = d2_matrix(m) <= np.float32(r2)
    adj &= fin[:, None] & fin[None, :]
    return adj


def exponent(r2_salient) -> int:
    _f, e2 = math.frexp(float(np.float32(r2_salient)))
    return -((-e2) // 2)                                # ceil(e2 / 2)


def _eig_desc(N6):
    """eigenvalues of the symmetric 3 x 3 matrix (xx, xy, xz, yy, yz, zz) in float64, descending; a coordinate whose row is all
    zero contributes an exact 0 and is split off.  -> (mu [3], exact_zero: the number of split coordinates)"""
    A = np.array([[N6[0], N6[1], N6[2]], [N6[1], N6[3], N6[4]], [N6[2], N6[4], N6[5]]], np.float64)
    keep = [c for c in range(3) if A[c].any()]
    ev = list(np.linalg.eigvalsh(A[np.ix_(keep, keep)])) if keep else []
    ev += [0.0] * (3 - len(keep))
    return np.sort(np.array(ev, np.float64))[::-1], 3 - len(keep)


def iss(model, r2_salient, r2_nonmax, gamma21=GAMMA21, gamma32=GAMMA32, min_neighbors=MIN_NEIGHBORS, quantised=True) -> dict:
    m = np.asarray(model, np.float32).reshape(-1, 3)
    M = len(m)
    e = exponent(r2_salient)
    scale = 2.0 ** (18 - e)
    back = L(4.0) ** L(-(18 - e))
    adj_s = adjacency(m, r2_salient) if M else np.zeros((0, 0), bool)
    adj_n = adjacency(m, r2_nonmax) if M else np.zeros((0, 0), bool)
    g21, g32 = L(gamma21), L(gamma32)
    n = adj_s.sum(axis=1).astype(np.int64)
    mu = np.full((M, 3), np.nan, L)
    lam = np.full((M, 3), np.nan, L)
    N = np.zeros((M, 6), np.float64)
    Nint = [None] * M
    zeros = np.zeros(M, np.int64)
    for i in range(M):
        if n[i] == 0:
            continue
        nb = np.flatnonzero(adj_s[i])
        if quantised:
            d = (m[nb] - m[i]).astype(np.float64) * scale                  # fp32 differences, scaled exactly
            q = np.rint(d).astype(np.int64)
            q = [[int(v) for v in row] for row in q]
            ni = len(q)
            S1 = [sum(r[a] for r in q) for a in range(3)]
            pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            Ni = tuple(ni * sum(r[a] * r[b] for r in q) - S1[a] * S1[b] for a, b in pairs)
            Nint[i] = (ni, Ni)
            N[i] = [float(v) for v in Ni]                                   # one rounding each (int -> float is correctly rounded)
            ev, zeros[i] = _eig_desc(N[i])
            mu[i] = ev.astype(L)
            lam[i] = (mu[i] / L(ni * ni)) * back
        else:
            d = m[nb].astype(L) - m[i].astype(L)
            c = d - d.mean(axis=0)
            Cm = (c[:, :, None] * c[:, None, :]).sum(axis=0) / L(len(nb))
            C6 = np.array([Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]], np.float64)
            N[i] = C6
            ev, zeros[i] = _eig_desc(C6)
            lam[i] = ev.astype(L)
            mu[i] = lam[i] * L(int(n[i]) ** 2) / back
    with np.errstate(invalid="ignore"):
        cand = (n >= min_neighbors) & (mu[:, 1] < g21 * mu[:, 0]) & (mu[:, 2] < g32 * mu[:, 1]) & (mu[:, 2] > 0)
    s = np.where(cand, lam[:, 2], L(0))
    key = np.zeros(M, bool)
    sensitive = np.zeros(M, bool)
    tol = L(TOL)
    for i in range(M):
        if n[i] < min_neighbors:
            continue
        m1, m2, m3 = mu[i]
        if zeros[i] == 3:                                # N = 0 (coincident rows): no candidate in any arithmetic
            pass
        elif abs(m2 - g21 * m1) <= tol * m1 or (abs(m3 - g32 * m2) <= tol * m1 and zeros[i] < 2) or (abs(m3) <= tol * m1 and zeros[i] < 1):
            sensitive[i] = True
        nbr = np.flatnonzero(adj_n[i])
        nbr = nbr[nbr != i]
        if cand[i]:
            sj = s[nbr]
            key[i] = not ((sj > s[i]) | ((sj == s[i]) & (nbr < i))).any()
            for j in nbr[cand[nbr]]:
                if abs(s[i] - s[j]) <= tol * max(s[i], s[j]) and not (quantised and Nint[i] == Nint[j]):
                    sensitive[i] = True
    excluded = sensitive | (adj_n & sensitive[None, :]).any(axis=1) if M else sensitive
    normN = np.sqrt((N[:, [0, 3, 5]] ** 2).sum(axis=1) + 2 * (N[:, [1, 2, 4]] ** 2).sum(axis=1))
    return dict(n=n, mu=mu, lam=lam, N=N, normN=normN, cand=cand, s=s, key=key, keypoints=np.flatnonzero(key).astype(np.int32),
                sensitive=sensitive, excluded=excluded, e=e, adj_nonmax=adj_n)


def keypoints_of(model, saliency, r2_nonmax) -> np.ndarray:
    """the contract's keypoint rule restated on RETURNED saliencies (float64) and the fp32 predicate: ascending int32 rows"""
    s = np.asarray(saliency, np.float64)
    adj = adjacency(model, r2_nonmax)
    out = []
    for i in np.flatnonzero(s > 0):
        nbr = np.flatnonzero(adj[i])
        nbr = nbr[nbr != i]
        if not ((s[nbr] > s[i]) | ((s[nbr] == s[i]) & (nbr < i))).any():
            out.append(i)
    return np.array(out, np.int32)


def family(name: str, M: int = M_FAMILY) -> np.ndarray:
    return normals_ref.family(name, M)


def cases():
    return [(name, rs, rn) for name in ("sheet", "volume") for rs, rn in RADII]


def case(name: str, rs: float, rn: float, quantised=True) -> dict:
    return iss(family(name), r2_of(rs), r2_of(rn), quantised=quantised)


def quantisation_bound(r2_salient) -> float:
    """|lambda - lambda_unq| <= (4 sqrt(3) 2^-17 + 3 2^-34) r2_salient: Weyl, from a rounding of at most 1/2 per component in scaled
    units and |x - mean| <= 2 * 2^18 there"""
    return (4 * math.sqrt(3) * 2.0 ** -17 + 3 * 2.0 ** -34) * float(np.float32(r2_salient))


def hand_case():
    """eight rows worked by hand (tests/test_iss_ref.py): seven on the axes about the first, one far away"""
    pts = np.array([[0, 0, 0], [1.5, 0, 0], [-1.5, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5], [0, 0, -0.5], [10, 10, 10]], np.float64)
    return (pts + np.array([8.0, 16.0, 4.0])).astype(np.float32)


def lattice_plane():
    g = np.arange(32, dtype=np.float32)
    return np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])


def lattice_cube(shuffle_seed=3):
    """9 x 9 x 9 integer lattice, rows in a fixed shuffled order -> (points [729, 3] float32, interior [729] bool)"""
    g = np.arange(9, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = pts[np.random.default_rng(shuffle_seed).permutation(len(pts))]
    interior = ((pts >= 1) & (pts <= 7)).all(axis=1)
    return pts + np.float32(20), interior
