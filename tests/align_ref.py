"""Independent extended-precision reference for AlignPoints_KNN (AlignPoints_KNN.m:17-59), the scenes that drive every branch of
pcreg_amd/csrc/align.hip, and the a-priori bounds at which a fp64 implementation is compared with it.  Standard library and
numpy only; shares no code with oracle/.

align(X, C1, C2)            the reference for ONE support X [n, 3] of fp64 values
conditioning(X, C1, C2)     the exact quantities that decide what may be compared, and how tightly
tolerances(X, C1, C2)       the bounds for centroid, coeff and aligned points, derived from conditioning() alone
selection_model(X)          align.hip step 2 restated literally in fp64 numpy: which branch of the selection a support reaches
compare(...)                the comparison the CPU and the GPU tests share: everything the support determines, nothing else
SCENES                      deterministic supports, each with its premises recorded as data (tests/test_align_ref.py checks them)

ARITHMETIC OF THE REFERENCE.  Every fp64 input is a dyadic rational; the support is scaled by a power of two to Python integers
I (X = I 2^-e), and everything up to the moments is integer arithmetic, hence exact:
  centroid          c = S / (n 2^e), S = sum I                                 rounded to fp64 once
  K                 round(0.85 n) half away from zero = (17 n + 10) // 20
  distances         n^2 4^e |x_i - c|^2 = |n I_i - S|^2 as integers; the K nearest by (distance^2, row): ties by ascending row
  moments           of the kept rows about their mean (pca, :33) or about c (C1, 'Centered' off, :31), divided by K - 1 or K
The six moments are rounded to np.longdouble (64-bit significand here; the module refuses a narrower one).  The 3 x 3 symmetric
eigenproblem is a cyclic Jacobi in np.longdouble run until the off-diagonal is below 2^-62 of the diagonal; eigenvalues descending,
stable; pca's sign convention (the largest-magnitude entry of each column positive, the first of equals); the votes (:45-46) are
2 pos >= n, pos counted over all rows of the raw support with C2 and over the kept, centred rows otherwise -- compared with n in
both cases, as the reference does (:37); y's sign from the determinant (:53).

THE BOUNDS.  u = 2^-53, gamma_k = k u / (1 - k u).  hat = what a fp64 implementation computes with sums in ANY order.
 1. centroid, per coordinate k:   |c^_k - c_k| <= gamma_(n+1) (sum_i |X_ik|) / n  =: dc_k
    (Higham, Accuracy and Stability, (4.4): n - 1 additions in any order, one division, one rounding of the reference.)
 2. deviations of the kept rows: x^_i = fl(fl(X_i - c^) - m^).  With rho = the largest |X_ik - c_k| over the kept rows plus max dc,
    each coordinate of a computed deviation carries  eta = 2 u (2 rho)  of rounding (two subtractions of numbers <= 2 rho), and
      without C1  nothing else to first order: c^ - c is a translation the centring removes, and an error dm in the mean enters
                  as K dm_a dm_b (the cross terms vanish), dm <= gamma_K 2 rho;
      with C1     the translation stays: sum (x_i - d)(y_i - d') - sum x_i y_i = -d' sum x_i - d sum y_i + K d d', d = c^ - c.
 3. second moments M_ab = sum x_ia x_ib over the kept rows, with A_a = sum_i |x_ia| and P_ab = sum_i |x_ia x_ib|:
      |M^_ab - M_ab| <= eta (A_a + A_b) + K eta^2 + u P_ab            products of perturbed factors, one rounding each
                        + gamma_(K-1) (P_ab + eta (A_a + A_b) + K eta^2)   K - 1 additions in any order
                        + [C1] dc_b |sum x_a| + dc_a |sum x_b| + K dc_a dc_b     or   [not C1] K dm^2
    and the covariance entry C_ab = M_ab / dof adds u |C_ab|.  E_ab is this bound; |E| its Frobenius norm over the full 3 x 3.
 4. eigenvectors.  The Jacobi is backward stable: its output is exact for a matrix within kJacobi u |C|_F of its input, kJacobi = 256
    (at most ~8 sweeps of 3 rotations here, each a handful of roundings on entries bounded by |C|_F, the reciprocal square root one
    ulp).  Davis-Kahan (in the form of Yu, Wang, Samworth 2015, and 2 sin(t / 2) <= sqrt 2 sin t): for column j with
    gap_j = min_(k != j) |lambda_j - lambda_k| and F = |E| + kJacobi u |C|_F,
      |coeff^_j - coeff_j|_2 <= sqrt 2 F / (gap_j - F) + 16 u          (16 u: normalisation of V and the determinant's y sign)
    A column whose gap_j is below 1 % of the trace is declared undetermined, not compared at a wide bound.
 5. aligned points, row i:  |aligned^_i - aligned_i| <= |X_i|_1 (max_j dcoeff_j + 4 u)      (3 u for the dot product, u for ours)
    and against X coeff^ with the implementation's OWN coeff, evaluated in fp64 (always asserted, also where coeff is undetermined):
    |X_i|_1 8 u  (gamma_3 for the implementation's dot product, gamma_3 for the fp64 evaluation it is compared with, 2 u to spare).
 6. orthonormality of coeff^: 256 u in general (the rotations' accumulated rounding), 8 u where the covariance is exactly diagonal
    (no rotation is applied: coeff is a signed permutation).
 7. signs and counts are exact.  A vote is determined when no admissible rounding can change it: projections with
    |p_i| <= 4 (|v_i|_1 (dcoeff + 4 u) + 3 (eta + [C1] max dc + [not C1] dm)) are counted as free, and the decision must be the
    same with all of them positive and all of them negative.  An undetermined x (z) vote frees the joint sign of columns 0, 1
    (1, 2); nothing else.
Nothing above is tuned to what the kernel or the oracles give.  What they do give, measured by tests/test_align_ref.py
(test_oracles_fall_inside_the_bounds prints it; largest error / bound over all scenes and flag pairs, informational):
    oracle_c    centroid 2.0e-02    coeff 4.7e-03    aligned 2.4e-03
    oracle_py   centroid 2.0e-02    coeff 1.2e-02    aligned 7.6e-03
"""
from __future__ import annotations

import functools
import itertools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs a long double with a 64-bit significand"
K_JACOBI = 256.0
GAP_FRAC = 0.01                      # a column is determined when its eigen-gap is at least this fraction of the trace
ORTHO_TOL = 256 * U
FLAGS = ((False, False), (True, False), (False, True), (True, True))
INSTANTIATIONS = ((4, 256), (4, 512), (12, 256), (8, 512), (16, 512))      # (PT, NT) of align.hip's launcher, by max_n
RULES = dict(ties="row", k_delta=0, vote_cmp=">=", vote_den="n", eig_order="desc", sign_rule="largest")


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def round_k(n: int) -> int:
    """round(0.85 n), half away from zero, exactly"""
    return (17 * n + 10) // 20


# ---- exact integers ---------------------------------------------------------------------------------------------------------
def _to_ints(X):
    """I [n][3] Python ints and e with X = I 2^-e exactly"""
    ratios = [[float(v).as_integer_ratio() for v in row] for row in X]
    e = max(d.bit_length() - 1 for row in ratios for _, d in row)
    return [[num << (e - (den.bit_length() - 1)) for num, den in row] for row in ratios], e


def _ld(fr: Fraction):
    """a Fraction rounded to long double (two fp64 pieces: 106 bits before the one rounding)"""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


def _exact(X):
    """the integer core shared by align() and conditioning(): rows scaled by n 2^e relative to the centroid, squared distances"""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    assert len(X) >= 2 and np.isfinite(X).all()
    n = len(X)
    I, e = _to_ints(X)
    S = [sum(r[k] for r in I) for k in range(3)]
    rel = [[n * r[k] - S[k] for k in range(3)] for r in I]                 # (x_i - c) n 2^e
    d2 = [r[0] * r[0] + r[1] * r[1] + r[2] * r[2] for r in rel]
    return X, n, e, S, rel, d2


def _tie_order(n, ties):
    """the rank of each row among equal distances.  "row": ascending row (the stable sort of :24); "highest": descending row;
    ("thread", NT): thread-major, the order a kernel that keeps point i in thread i % NT would give by mistake"""
    if ties == "row":
        return list(range(n))
    if ties == "highest":
        return [n - 1 - i for i in range(n)]
    NT = ties[1]
    order = sorted(range(n), key=lambda i: (i % NT, i // NT))
    rank = [0] * n
    for r, i in enumerate(order):
        rank[i] = r
    return rank


def jacobi_ld(C):
    """eigenvalues [3] and eigenvectors (columns) of a symmetric 3 x 3 long double matrix: cyclic Jacobi"""
    A = np.array(C, dtype=LD)
    V = np.eye(3, dtype=LD)
    for _ in range(100):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off == 0 or off <= LD(2.0 ** -62) * (abs(A[0, 0]) + abs(A[1, 1]) + abs(A[2, 2])):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0:
                continue
            theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
            t = (LD(1) if theta >= 0 else LD(-1)) / (abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = c * t
            J = np.eye(3, dtype=LD)
            J[p, p] = c; J[q, q] = c; J[p, q] = s; J[q, p] = -s
            A = J.T @ A @ J
            A[p, q] = A[q, p] = 0
            V = V @ J
    return np.array([A[0, 0], A[1, 1], A[2, 2]]), V


def align(X, C1=False, C2=False, rules=None) -> dict:
    """AlignPoints_KNN.m:17-59 for one support.  rules: RULES with entries replaced -- the deliberately wrong variants that
    tests/test_align_ref.py uses to show the bounds are not loose (a "flags" entry names the flag pairs a variant shows under and
    is ignored here); None is the reference.
    Returns c [3], coeff [3, 3] (coeff[:, j] = column j), aligned [n, 3], kept (sorted rows), K, eigenvalues [3] descending,
    votes (posx, posz), n_votes, min_abs_proj, proj [n_votes, 2] (columns 0 and 2), dev (the kept rows' deviations), coeff_pca."""
    R = dict(RULES, **{k: v for k, v in (rules or {}).items() if k != "flags"})
    X, n, e, S, rel, d2 = _exact(X)
    scale = n << e
    c = np.array([float(Fraction(S[k], scale)) for k in range(3)])
    K = min(max(round_k(n) + R["k_delta"], 1), n)
    tr = _tie_order(n, R["ties"])
    order = sorted(range(n), key=lambda i: (d2[i], tr[i]))
    kept = sorted(order[:K])
    # moments of the kept rows, exact: about their mean (dof K - 1) or about the centroid (C1: dof K)
    s1 = [sum(rel[i][k] for i in kept) for k in range(3)]
    dof = K if C1 else max(K - 1, 1)
    Cm = np.zeros((3, 3), dtype=LD)
    for a in range(3):
        for b in range(a, 3):
            s2 = sum(rel[i][a] * rel[i][b] for i in kept)
            num = Fraction(s2) if C1 else Fraction(K * s2 - s1[a] * s1[b], K)
            Cm[a, b] = Cm[b, a] = _ld(num / (dof * scale * scale))
    ev, V = jacobi_ld(Cm)
    idx = sorted(range(3), key=lambda j: -ev[j]) if R["eig_order"] == "desc" else sorted(range(3), key=lambda j: ev[j])
    ev, V = ev[idx], V[:, idx]
    for j in range(3):
        big = 0 if R["sign_rule"] == "first" else int(np.argmax(np.abs(V[:, j])))        # argmax: the first of equals
        if V[big, j] < 0:
            V[:, j] = -V[:, j]
    coeff_pca = V.copy()
    # the votes
    mean = [Fraction(0)] * 3 if C1 else [Fraction(s1[k], K) for k in range(3)]
    dev = np.array([[_ld((rel[i][k] - mean[k]) / scale) for k in range(3)] for i in kept], dtype=LD).reshape(-1, 3)
    voters = X.astype(LD) if C2 else dev
    proj = voters @ V[:, [0, 2]]
    pos = (proj > 0).sum(axis=0)
    den = n if R["vote_den"] == "n" else K
    win = (lambda p: 2 * p >= den) if R["vote_cmp"] == ">=" else (lambda p: 2 * p > den)
    xs, zs = (1 if win(int(pos[0])) else -1), (1 if win(int(pos[1])) else -1)
    M = V * np.array([xs, 1, zs], dtype=LD)
    ys = 1 if np.linalg.det(M.astype(np.float64)) > 0 else -1
    cu = V * np.array([xs, ys, zs], dtype=LD)
    aligned = X.astype(LD) @ cu
    return dict(c=c, coeff=cu.astype(np.float64), aligned=aligned.astype(np.float64), kept=np.array(kept), K=K, n=n,
                eigenvalues=ev.astype(np.float64), votes=(int(pos[0]), int(pos[1])), n_votes=len(voters),
                min_abs_proj=float(np.abs(proj).min()), proj=proj.astype(np.float64), dev=dev.astype(np.float64),
                voters_l1=np.abs(voters).sum(axis=1).astype(np.float64), coeff_pca=coeff_pca.astype(np.float64), signs=(xs, ys, zs))


@functools.lru_cache(maxsize=None)
def _scene_ref(name, C1, C2):
    return align(SCENES[name].X, C1, C2)


def scene_ref(name, C1, C2):
    """align() of a scene, computed once"""
    return _scene_ref(name, bool(C1), bool(C2))


@functools.lru_cache(maxsize=None)
def _scene_tol(name, C1, C2):
    s, r = SCENES[name], _scene_ref(name, C1, C2)
    return tolerances(s.X, C1, C2, r, conditioning(s.X, C1, C2, r))


def scene_tol(name, C1, C2):
    """tolerances() of a scene, computed once"""
    return _scene_tol(name, bool(C1), bool(C2))


# ---- conditioning and tolerances ----------------------------------------------------------------------------------------------
def conditioning(X, C1=False, C2=False, ref=None) -> dict:
    ref = ref or align(X, C1, C2)
    X, n, e, S, rel, d2 = _exact(X)
    K = ref["K"]
    sd = sorted(d2)
    # integer coordinates below 2^25 with an integer centroid: sums, differences, squares and their sums are exact in fp64
    exact_arith = bool((X == np.round(X)).all() and all(s % (n << e) == 0 for s in S) and np.abs(X).max() < 2.0 ** 25)
    if K < n:
        kth_equal = sd[K - 1] == sd[K]
        kth_rel_gap = 0.0 if kth_equal else float(Fraction(sd[K] - sd[K - 1], 2 * sd[K]))       # of the distances, first order
    else:
        kth_equal, kth_rel_gap = False, math.inf
    kth_distance = math.sqrt(float(Fraction(sd[K - 1], (n << e) ** 2)))
    ev = ref["eigenvalues"]
    trace = float(ev.sum())
    mags = np.sort(np.abs(ref["coeff_pca"]), axis=0)
    dev = ref["dev"]
    Xc = X - ref["c"]
    return dict(n=n, K=K, dof=(K if C1 else max(K - 1, 1)), exact_arith=exact_arith,
                kth_bit_equal=bool(kth_equal and exact_arith), kth_exactly_equal=bool(kth_equal), kth_rel_gap=kth_rel_gap, kth_distance=kth_distance,
                eigenvalues=ev, eigen_gaps=(float(ev[0] - ev[1]), float(ev[1] - ev[2])), trace=trace,
                col_gaps=(float(ev[0] - ev[1]), float(min(ev[0] - ev[1], ev[1] - ev[2])), float(ev[1] - ev[2])),
                column_sign_margins=tuple(float(v) for v in (mags[2] - mags[1])),
                votes=ref["votes"], vote_margins=tuple(abs(2 * p - n) for p in ref["votes"]), n_votes=ref["n_votes"],
                min_abs_proj=ref["min_abs_proj"],
                extent=float(np.sqrt((Xc * Xc).sum(axis=1)).max()), max_abs=float(np.abs(X).max()),
                sum_abs=np.abs(X).sum(axis=0), rho_kept=float(np.abs(Xc[ref["kept"]]).max()),
                A=np.abs(dev).sum(axis=0), P=np.abs(dev).T @ np.abs(dev), s1=dev.sum(axis=0), C_fro=float(np.sqrt((ev * ev).sum())))


def tolerances(X, C1=False, C2=False, ref=None, cond=None) -> dict:
    """c [3], coeff [3] (per column; inf where the column is undetermined), coeff_max, aligned [n], aligned_self [n], ortho,
    determined (three booleans), votes_determined (x, z), free_signs: the diagonal sign matrices the votes leave open."""
    ref = ref or align(X, C1, C2)
    q = cond or conditioning(X, C1, C2, ref)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n, K, dof = q["n"], q["K"], q["dof"]
    safe = 1.0 + 1e-9                                            # the fp64 evaluation of the exact quantities themselves
    dc = gamma(n + 1) * q["sum_abs"] / n * safe
    rho = q["rho_kept"] + dc.max()
    eta = 2 * U * (2 * rho)
    dm = 0.0 if C1 else gamma(K) * 2 * rho
    A, P, s1 = q["A"], q["P"], np.abs(q["s1"])
    E = np.zeros((3, 3))
    Cabs = np.abs((ref["coeff_pca"] * ref["eigenvalues"]) @ ref["coeff_pca"].T)
    for a in range(3):
        for b in range(3):
            pert = eta * (A[a] + A[b]) + K * eta * eta
            t = pert + U * P[a, b] + gamma(max(K - 1, 1)) * (P[a, b] + pert)
            t += (dc[b] * s1[a] + dc[a] * s1[b] + K * dc[a] * dc[b]) if C1 else K * dm * dm
            E[a, b] = t / dof + U * Cabs[a, b]
    F = (np.sqrt((E * E).sum()) + K_JACOBI * U * q["C_fro"]) * safe
    tol_co = np.full(3, np.inf)
    determined = [False] * 3
    for j in range(3):
        g = q["col_gaps"][j]
        if q["trace"] > 0 and g >= GAP_FRAC * q["trace"] and g > 2 * F:
            tol_co[j] = math.sqrt(2.0) * F / (g - F) + 16 * U
            determined[j] = True
    co_max = float(tol_co[np.isfinite(tol_co)].max()) if any(determined) else math.inf
    l1 = np.abs(X).sum(axis=1)
    diagonal = bool(np.all(np.sort(np.abs(ref["coeff_pca"]), axis=0)[:2] == 0))
    # the votes: which can no admissible rounding change
    votes_det = []
    for col, j in ((0, 0), (1, 2)):
        if not determined[j]:
            votes_det.append(False)
            continue
        eps = 4 * (ref["voters_l1"] * (tol_co[j] + 4 * U) + (0.0 if C2 else 3 * (eta + (dc.max() if C1 else dm))))
        p = ref["proj"][:, col]
        free = np.abs(p) <= eps
        lo, hi = int((p[~free] > 0).sum()), int((p[~free] > 0).sum() + free.sum())
        votes_det.append((2 * lo >= n) == (2 * hi >= n))
    free_signs = [np.array([sx, sx * sz, sz], dtype=np.float64) for sx in ((1,) if votes_det[0] else (1, -1))
                  for sz in ((1,) if votes_det[1] else (1, -1))]
    return dict(c=dc, coeff=tol_co, coeff_max=co_max, aligned=l1 * (co_max + 4 * U), aligned_self=l1 * 8 * U,
                ortho=8 * U if diagonal else ORTHO_TOL, determined=tuple(determined), votes_determined=tuple(votes_det),
                free_signs=free_signs)


def compare(X, ref, tol, c, coeff, aligned) -> dict:
    """Everything the support determines, asserted; returns the largest error / bound per quantity (for the record).
    c [3], coeff [3, 3] with columns as columns, aligned [n, 3]: the implementation's outputs."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    c, coeff, aligned = np.asarray(c, np.float64).ravel(), np.asarray(coeff, np.float64).reshape(3, 3), np.asarray(aligned, np.float64).reshape(-1, 3)
    assert np.isfinite(c).all() and np.isfinite(coeff).all() and np.isfinite(aligned).all(), "non-finite output"
    ratios = {}
    ec = np.abs(c - ref["c"])
    ok = ec <= tol["c"]
    assert ok.all(), ("centroid", ec, tol["c"])
    ratios["c"] = float(np.max(ec[tol["c"] > 0] / tol["c"][tol["c"] > 0])) if (tol["c"] > 0).any() else 0.0
    eo = np.abs(coeff.T @ coeff - np.eye(3)).max()
    assert eo <= tol["ortho"], ("orthonormality", eo, tol["ortho"])
    es = np.abs(aligned - X @ coeff).max(axis=1)
    assert (es <= tol["aligned_self"]).all(), ("aligned vs the implementation's own coeff", es.max())
    det = np.array(tol["determined"])
    if det.any():
        best = None
        for s in tol["free_signs"]:                               # the one frame, or the few the votes leave open
            eco = np.abs(coeff - ref["coeff"] * s).max(axis=0)
            eal = np.abs(aligned - ref["aligned"] * s)
            r_co = float(np.max(eco[det] / tol["coeff"][det]))
            live = tol["aligned"] > 0
            r_al = float(np.max((eal[:, det].max(axis=1)[live]) / tol["aligned"][live])) if live.any() else 0.0
            if (eal[:, det].max(axis=1) > tol["aligned"]).any():
                r_al = max(r_al, math.inf)
            if best is None or max(r_co, r_al) < max(best):
                best = (r_co, r_al)
        ratios["coeff"], ratios["aligned"] = best
        assert best[0] <= 1.0, ("coeff", best[0], tol["coeff"])
        assert best[1] <= 1.0, ("aligned", best[1])
    return ratios


# ---- align.hip step 2, literally --------------------------------------------------------------------------------------------
K_SMALL = 256


def selection_model(X) -> dict:
    """align.hip:123-190 in fp64 numpy, one operation per rounding, in the kernel's order.  The centroid is numpy's sum: the model
    is a statement about the kernel only where `robust` is True -- the arithmetic up to the square root is exact (integer
    coordinates, integer centroid), or m is at least 2 x away from kSmall and no distance lies within 2^-40 relative of an
    edge of the K-th's bin."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    c = X.sum(axis=0) / n                                         # :114-117
    K = int(math.floor(n * 0.85 + 0.5))                           # :124
    x, y, z = X[:, 0] - c[0], X[:, 1] - c[1], X[:, 2] - c[2]      # :129
    D = np.sqrt(x * x + y * y + z * z)                            # :130
    dlo, dhi = float(D.min()), float(D.max())                     # :131-140
    scale = 256.0 / (dhi - dlo) if dhi > dlo else 0.0             # :142
    pos = (D - dlo) * scale
    bins = np.minimum(pos.astype(np.int64), 255)                  # :143
    hist = np.bincount(bins, minlength=256)                       # :144
    cum = np.cumsum(hist)
    bstar = int(np.searchsorted(cum, K))                          # :155: before < K <= before + count
    below = int(cum[bstar] - hist[bstar])
    m = int(hist[bstar])                                          # :163-165
    keys = np.sort(D[bins == bstar])
    vK = float(keys[K - below - 1])                               # :167-189, either way the Kp-th smallest key of the bin
    n_less = below + int((keys < vK).sum())
    n_eq = int((D == vK).sum())
    take_eq = K - n_less                                          # :190
    exact = bool((X == np.round(X)).all() and (c == np.round(c)).all() and np.abs(X).max() < 2.0 ** 25
                 and (X.sum(axis=0) == np.round(c) * n).all())
    edges = [e for e in ((bstar,) if bstar > 0 else ()) + ((bstar + 1,) if bstar < 255 else ())]
    edge_margin = min([float(np.abs(pos - e).min()) / 256.0 for e in edges], default=math.inf) if scale > 0 else math.inf
    margin_m = m <= K_SMALL // 2 or m >= 2 * K_SMALL
    return dict(n=n, K=K, flat=not (dhi > dlo), bstar=bstar, below=below, m=m, branch="small" if m <= K_SMALL else "bisect",
                n_less=n_less, n_eq=n_eq, take_eq=take_eq, split=n_eq != take_eq, exact=exact, edge_margin=edge_margin,
                robust=bool(exact or (margin_m and edge_margin >= 2.0 ** -40)), vK=vK,
                tied_rows=np.flatnonzero(D == vK))


# ---- scenes -------------------------------------------------------------------------------------------------------------------
class Scene:
    """X [n, 3] (read-only), the flag pairs it is defined for, and its premises as data: `expect` holds what
    selection_model / conditioning must say (branch, split, flat, determined, votes, ...), `mutants` the wrong rules that must
    land far outside the bounds on this scene, `about_degeneracy` exempts it from the eigen-gap premise."""

    def __init__(self, name, X, flags=FLAGS, expect=None, mutants=(), about_degeneracy=False, note=""):
        self.name, self.flags, self.expect, self.mutants = name, tuple(flags), dict(expect or {}), tuple(mutants)
        self.about_degeneracy, self.note = about_degeneracy, note
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.X.setflags(write=False)
        self.n = len(self.X)

    def holds(self, pt, nt):
        return self.n <= pt * nt


def _rot(seed):
    """a fixed proper rotation"""
    Q = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))[0]
    return Q * np.sign(np.linalg.det(Q))


def _plain(n, seed, shift=(11.0, -7.0, 23.0), half=(6.0, 3.0, 1.2)):
    """a uniform anisotropic box, rotated: bounded extent, healthy eigen-gaps"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 3)) * np.array(half)) @ _rot(seed + 1) + np.array(shift)


def _symmetric_lattice(pairs, half, seed, shift, exclude=None):
    """`pairs` random integer points of the box +-half (none at the origin) and their negatives, shuffled, translated by integers"""
    rng = np.random.default_rng(seed)
    P = np.zeros((0, 3), dtype=np.int64)
    while len(P) < pairs:
        cand = rng.integers(-np.array(half), np.array(half) + 1, (pairs, 3))
        cand = cand[(cand != 0).any(axis=1)]
        if exclude is not None:
            cand = cand[exclude(cand)]
        P = np.concatenate([P, cand])[:pairs]
    X = np.concatenate([P, -P])
    return X[rng.permutation(len(X))].astype(np.float64) + np.array(shift, dtype=np.float64)


def _orbit(triple):
    """the 48 sign changes and permutations of an integer triple with distinct non-zero magnitudes"""
    return np.array(sorted({tuple(s * t for s, t in zip(sg, pm)) for pm in itertools.permutations(triple)
                            for sg in itertools.product((1, -1), repeat=3)}), dtype=np.int64)


def _crowded_split(rep, n_inner_pairs, n_outer_pairs, order, seed=11, shift=(40, -12, 7)):
    """A shell of rep x 48 points at one distance (21: the orbit of (6, 9, 18)), anisotropic inner points, outer points; all
    centrally symmetric integers, so centroid and distances are exact.  Among the tied rows the order is by descending x y:
    the lowest rows (the stable sort's choice) and the highest differ in their xy moment, so another choice of ties turns the
    frame.  order: where the tied rows stand among the others -- "first", "last" or "interleaved" (evenly spread)."""
    rng = np.random.default_rng(seed)
    shell = np.repeat(_orbit((6, 9, 18)), rep, axis=0)
    shell = shell[np.argsort(-(shell[:, 0] * shell[:, 1]), kind="stable")]
    inner = _symmetric_lattice(n_inner_pairs, (14, 7, 2), seed + 1, (0, 0, 0)).astype(np.int64)
    outer = _symmetric_lattice(n_outer_pairs, (40, 30, 26), seed + 2, (0, 0, 0), exclude=lambda p: (p * p).sum(axis=1) > 600).astype(np.int64)
    others = np.concatenate([inner, outer])
    others = others[rng.permutation(len(others))]
    if order == "first":
        X = np.concatenate([shell, others])
    elif order == "last":
        X = np.concatenate([others, shell])
    else:
        n = len(shell) + len(others)
        slots = np.zeros(n, dtype=bool)
        slots[np.unique(np.floor(np.arange(len(shell)) * n / len(shell)).astype(np.int64))] = True
        assert slots.sum() == len(shell)
        X = np.empty((n, 3), dtype=np.int64)
        X[slots], X[~slots] = shell, others
    return X.astype(np.float64) + np.array(shift, dtype=np.float64)


def _sphere(N, limit=40):
    g = np.arange(-limit, limit + 1)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    keep = (x * x + y * y + z * z) == N
    return np.column_stack([x[keep], y[keep], z[keep]]).astype(np.int64)


def _equal_distances(N, shift=(17, -5, 9)):
    """every integer point of the sphere |p|^2 = N (centrally symmetric: the centroid is the integer shift).  Rows are ordered
    so that the 15 % the stable tie rule drops (the last rows) crowd around two oblique axes, 10 % and 5 %: the kept rows then
    have three well separated variances along oblique axes."""
    P = _sphere(N)
    n = len(P)
    q1, q2 = np.array([6.0, 2.0, 3.0]) / 7.0, np.array([2.0, 3.0, -6.0]) / 7.0
    s1 = np.abs(P @ q1)
    d1 = np.argsort(-s1, kind="stable")[: int(round(0.10 * n))]
    rest = np.setdiff1d(np.arange(n), d1)
    d2 = rest[np.argsort(-np.abs(P[rest] @ q2), kind="stable")[: n - round_k(n) - len(d1) + 4]]
    head = np.setdiff1d(rest, d2)
    rng = np.random.default_rng(N)
    order = np.concatenate([head[rng.permutation(len(head))], np.concatenate([d1, d2])[rng.permutation(len(d1) + len(d2))]])
    return P[order].astype(np.float64) + np.array(shift, dtype=np.float64)


def _outlier(n, seed):
    """a Gaussian support and one far outlier: every other distance falls into bin 0 of the 256"""
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(n, 3)) * np.array([2.0, 1.0, 0.4])) @ _rot(seed + 1) + np.array([5.0, 3.0, -2.0])
    X[n // 3] = np.array([5.0, 3.0, -2.0]) + np.array([3600.0, 2800.0, 1600.0])
    return X


def _vote_tie(pairs, seed):
    """centrally symmetric about the origin, integer coordinates of a rotated anisotropic box: with C2 both votes are n / 2"""
    rng = np.random.default_rng(seed)
    P = np.round((rng.uniform(-1, 1, (pairs, 3)) * np.array([3000.0, 1500.0, 400.0])) @ _rot(seed + 1))
    X = np.concatenate([P, -P])
    return X[rng.permutation(len(X))]


def _skewed(n, seed):
    """52 % of the rows near +1 and 48 % near -1.083 along the main axis (mean 0; the far cluster loses more rows to the 15 %
    cut): over the kept rows more than half of the projections are positive, but fewer than n / 2"""
    rng = np.random.default_rng(seed)
    na = int(round(0.52 * n))
    x = np.concatenate([1.0 + rng.uniform(-0.3, 0.3, na), -(na / (n - na)) + rng.uniform(-0.3, 0.3, n - na)])
    X = np.column_stack([x, rng.uniform(-1.2, 1.2, n), rng.uniform(-0.4, 0.4, n)])
    return X[rng.permutation(n)] @ _rot(seed + 1) + np.array([3.0, -8.0, 5.0])


def _box(perm, seed=5):
    """20 octant representatives with distinct norms and all their sign changes (n = 160, K = 136 = 17 orbits of 8): every
    off-diagonal moment of the kept rows is exactly zero, the frame is a signed permutation.  perm: the order of the variances."""
    rng = np.random.default_rng(seed)
    reps, norms = [], set()
    while len(reps) < 20:
        p = rng.integers(1, np.array([25, 12, 5]))
        if int(p @ p) not in norms:
            norms.add(int(p @ p)); reps.append(p)
    X = np.array([p * np.array(s) for p in reps for s in itertools.product((1, -1), repeat=3)], dtype=np.float64)
    return X[rng.permutation(len(X))][:, list(perm)]


def _tiny(n, seed):
    return np.round(np.random.default_rng(seed).normal(size=(n, 3)) * np.array([4.0, 2.0, 1.0]) @ _rot(seed + 1) * 64) / 64 + np.array([2.0, -1.0, 0.5])


def _far(n, seed):
    """a symmetric support on a 2^-16 grid about an exactly representable far centre (the descriptor tests' translation)"""
    rng = np.random.default_rng(seed)
    P = np.round((rng.uniform(-1, 1, (n // 2, 3)) * np.array([5.0, 2.5, 1.0])) @ _rot(seed + 1) * 65536) / 65536
    X = np.concatenate([P, -P])
    return X[rng.permutation(len(X))] + np.array([4.2e6, -3.9e6, 5.1e5])


FILLER_SIZES = (1024, 2048, 3072, 4096, 8192)
_TIE_MUTANTS = ({"ties": "highest"}, {"ties": ("thread", 256)}, {"ties": ("thread", 512)})
# (the pca sign convention cancels in the final frame wherever all n rows vote, C2: a flipped column flips its vote too)
_GENERAL_MUTANTS = ({"k_delta": 1}, {"k_delta": -1}, {"eig_order": "asc"}, {"sign_rule": "first", "flags": ((False, False), (True, False))})


def _build():
    S = []
    add = lambda *a, **k: S.append(Scene(*a, **k))
    add("split_tie_small", _symmetric_lattice(200, (6, 4, 2), 1, (17, -5, 9)),
        expect=dict(branch="small", split=True, exact=True), mutants=({"ties": "highest"}, {"ties": ("thread", 256)}))
    for order in ("first", "last", "interleaved"):
        add(f"crowded_split_{order}", _crowded_split(10, 150, 35, order),          # (tied rows first: all in thread row 0 of NT = 512)
            expect=dict(branch="bisect", split=True, exact=True, m=480, n_eq=480), mutants=_TIE_MUTANTS[:2] if order == "first" else _TIE_MUTANTS)
    add("crowded_split_large", _crowded_split(40, 460, 110, "interleaved", seed=13),
        expect=dict(branch="bisect", split=True, exact=True, m=1920, n_eq=1920), mutants=_TIE_MUTANTS)
    add("crowded_distinct", _outlier(1000, 21), expect=dict(branch="bisect", split=False, exact=False, m=999, n_eq=1, take_eq=1, bstar=0))
    add("equal_distances_240", _equal_distances(194), expect=dict(branch="small", split=True, flat=True, exact=True, m=240),
        mutants=({"ties": "highest"},))
    add("equal_distances_720", _equal_distances(1361), expect=dict(branch="bisect", split=True, flat=True, exact=True, m=720),
        mutants=({"ties": "highest"}, {"ties": ("thread", 256)}, {"ties": ("thread", 512)}))
    for n in (100, 300):
        add(f"identical_{n}", np.tile(np.array([[3.0, -7.0, 11.0]]), (n, 1)), about_degeneracy=True,
            expect=dict(branch="small" if n <= 256 else "bisect", split=True, flat=True, determined=(False, False, False)))
    tie = _vote_tie(500, 31)
    ref = align(tie, False, True)
    both_pos = np.flatnonzero((ref["proj"] > 0).all(axis=1))[0]
    both_neg = np.flatnonzero((ref["proj"] < 0).all(axis=1))[0]
    vote_flags = ((False, True), (True, True))
    add("vote_tie", tie, flags=vote_flags, expect=dict(votes=(500, 500), signs_xz=(1, 1)), mutants=({"vote_cmp": ">"},))
    add("vote_tie_minus_half", np.delete(tie, both_pos, axis=0), flags=vote_flags, expect=dict(votes=(499, 499), signs_xz=(-1, -1)))
    add("vote_tie_plus_half", np.delete(tie, both_neg, axis=0), flags=vote_flags, expect=dict(votes=(500, 500), signs_xz=(1, 1)))
    add("votes_over_kept", _skewed(400, 41), flags=((False, False), (True, False)),
        expect=dict(kept_majority_below_half_n=True, signs_xz=(-1, -1)), mutants=({"vote_den": "K"},))
    for perm in itertools.permutations(range(3)):
        add("box_" + "".join("xyz"[p] for p in perm), _box(perm), expect=dict(exact=True, split=False, permutation=True),
            mutants=({"eig_order": "asc"},))
    for n, seed in ((2, 50), (3, 50), (4, 50), (5, 50), (6, 50), (7, 50)):
        add(f"tiny_{n}", _tiny(n, seed), about_degeneracy=n <= 4, expect=dict(K={2: 2, 3: 3, 4: 3, 5: 4, 6: 5, 7: 6}[n]))
    add("far", _far(400, 61), expect=dict(branch="small"))
    add("plain_500", _plain(500, 71), expect=dict(branch="small"), mutants=_GENERAL_MUTANTS)
    for n in FILLER_SIZES:
        add(f"filler_{n}", _plain(n, 80 + n), expect=dict(branch="small"), mutants=_GENERAL_MUTANTS if n == 1024 else ())
    return {s.name: s for s in S}


SCENES = _build()
