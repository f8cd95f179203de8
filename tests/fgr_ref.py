"""Reference of fast global registration (pcreg_fgr_batched's contract, include/pcreg.h) -- numpy only, no GPU.

  kept_mask   the tuple test in float64: every compare is an exact restatement, so the mask is exact
  run_ld      the contract in numpy.longdouble (the mask, o, mu0 and the mu schedule are float64 by definition and enter as they are)
  run64       the contract restated in float64, one operation per operation of csrc/fgr_pair.hpp, with SEQUENTIAL sums
  run_tree    run64 with the device's sum order (tree_sum): what the kernels compute, bit for bit
  tree_sum    the contract's sum order of one value per kept pair: chunks of 2048, thread t adds t, t + 256, ...; the wave butterfly;
              ((w0 + w1) + w2) + w3; the chunks ascending
  scene       extent 100, noise sigma 0.05, uniformly random outliers, a rotation of a given angle about a random axis

E_method = |run64 - run_ld| per output is the yardstick tests/test_gpu_fgr.py holds the device to (method_error)."""
import numpy as np

import plane_ref
from oracle.pcreg_oracle import sample_table

LD = np.longdouble
CHUNK, BLOCK = 2048, 256
DEFAULTS = dict(iterations=128, decrease_every=4, division_factor=1.4, mu0=0.0, n_tuples=0, tuple_scale=0.95, seed=0)
E_FLOOR = 2.0 ** -49                       # tests/cpd_ref.py's: what the doubles themselves cost
DELTA = 1.0
CASES = ((256, 0.5, 1.0), (512, 0.7, 2.5), (1000, 0.8, 2.0))        # (n, outlier share, angle)


def options(**kw):
    o = dict(DEFAULTS, delta2=DELTA * DELTA)
    o.update(kw)
    return o


# ------------------------------------------------------------------------------------------------------------------- the scenes
def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene(n, share, angle, seed):
    """-> dict(p1, p2 [n, 3] float64, inliers [n] bool (the planted set), T [4, 4] with [p2, 1] @ T = [p1, 1] on the inliers)"""
    rng = np.random.default_rng(seed)
    p2 = rng.random((n, 3)) * 100.0
    R = rotation(rng.normal(size=3), angle)
    t = rng.uniform(-20.0, 20.0, 3)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.T, t
    p1 = p2 @ R.T + t + rng.normal(0.0, 0.05, (n, 3))
    out = rng.permutation(n)[:int(round(share * n))]
    lo = (np.array([[0.0, 0, 0], [100.0, 0, 0], [0, 100.0, 0], [0, 0, 100.0], [100.0, 100.0, 100.0]]) @ R.T + t).min(axis=0)
    p1[out] = lo + rng.random((len(out), 3)) * 140.0                # uniform over a box that holds the moved cloud
    inl = np.ones(n, bool)
    inl[out] = False
    return dict(p1=p1, p2=p2, inliers=inl, T=T)


_SCENES = {}


def scenes():
    """the three cases of the issue, generated once"""
    if not _SCENES:
        for k, (n, share, angle) in enumerate(CASES):
            _SCENES[k] = scene(n, share, angle, 1000 + k)
    return [_SCENES[k] for k in range(len(CASES))]


# -------------------------------------------------------------------------------------------------------------- the tuple test
def triples(n, opts, b=0, tuple_idx=None):
    """0-based [n_tuples, 3], clamped as pcreg_ransac clamps its table"""
    if tuple_idx is not None:
        t = np.asarray(tuple_idx, np.int64).reshape(-1, 3) - 1
    else:
        t = sample_table(n, int(opts["n_tuples"]), 3, int(opts["seed"]) + b).astype(np.int64) - 1
    return np.clip(t, 0, n - 1)


def _d2(A, i, j):
    d = A[i] - A[j]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def kept_mask(p1, p2, opts, b=0, tuple_idx=None):
    p1, p2 = np.asarray(p1, np.float64).reshape(-1, 3), np.asarray(p2, np.float64).reshape(-1, 3)
    n = len(p1)
    live = np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)
    if int(opts["n_tuples"]) == 0:
        return live
    kept = np.zeros(n, bool)
    if n < 3:
        return kept
    t = triples(n, opts, b, tuple_idx)
    s2 = float(opts["tuple_scale"]) * float(opts["tuple_scale"])
    ok = live[t].all(axis=1)
    with np.errstate(all="ignore"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            a, bb = _d2(p1, t[:, i], t[:, j]), _d2(p2, t[:, i], t[:, j])
            ok &= (s2 * a < bb) & (s2 * bb < a)
    kept[t[ok].ravel()] = True
    return kept


# ------------------------------------------------------------------------------------------------------------------ the sums
def tree_sum(x):
    """the contract's order for one float64 value per kept pair (0.0 where a pair adds nothing: x + 0.0 has x's bits)"""
    x = np.asarray(x, np.float64)
    total = 0.0
    lanes = np.arange(64)
    for c in range(0, len(x), CHUNK):
        blk = np.zeros(CHUNK)
        part = x[c:c + CHUNK]
        blk[:len(part)] = part
        a = np.zeros(BLOCK)
        for u in range(CHUNK // BLOCK):
            a = a + blk[u * BLOCK:(u + 1) * BLOCK]
        w = a.reshape(BLOCK // 64, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lanes ^ o]
        total = total + (((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    return float(total)


def _seq_sum(x):
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def _ld_sum(x):
    return np.asarray(x, LD).sum()


def _moved(P2, T):
    return np.stack([((P2[:, 0] * T[0, j] + P2[:, 1] * T[1, j]) + P2[:, 2] * T[2, j]) + T[3, j] for j in range(3)], axis=1)


def _residuals(P1, P2, T):
    q = _moved(P2, T)
    r = q - P1
    return q, r, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]


def pair_terms(q, r, rr, o, mu):
    """{sum index: [n_kept] terms w * v} of csrc/fgr_pair.hpp's fgr_pair_add, in the dtype of q"""
    t = mu / (mu + rr)
    w = t * t
    u0, u1, u2 = q[:, 0] - o[0], q[:, 1] - o[1], q[:, 2] - o[2]
    tri = plane_ref.tri
    one = w
    return {tri(0, 0): w * (u1 * u1 + u2 * u2), tri(0, 1): w * (-(u0 * u1)), tri(0, 2): w * (-(u0 * u2)), tri(0, 4): w * (-u2), tri(0, 5): w * u1,
            tri(1, 1): w * (u0 * u0 + u2 * u2), tri(1, 2): w * (-(u1 * u2)), tri(1, 3): w * u2, tri(1, 5): w * (-u0),
            tri(2, 2): w * (u0 * u0 + u1 * u1), tri(2, 3): w * (-u1), tri(2, 4): w * u0, tri(3, 3): one, tri(4, 4): one, tri(5, 5): one,
            21: w * (u1 * r[:, 2] - u2 * r[:, 1]), 22: w * (u2 * r[:, 0] - u0 * r[:, 2]), 23: w * (u0 * r[:, 1] - u1 * r[:, 0]),
            24: w * r[:, 0], 25: w * r[:, 1], 26: w * r[:, 2], 27: w * rr}


def sums28(P1, P2, T, o, mu, summer, dt=np.float64):
    q, r, rr = _residuals(P1, P2, T)
    s = np.zeros(28, dt)
    for k, v in pair_terms(q, r, rr, o, mu).items():
        s[k] = summer(v)
    return s


def compose(T, S):
    """T @ S, every entry ((T(r,0) S(0,c) + T(r,1) S(1,c)) + T(r,2) S(2,c)) + T(r,3) S(3,c)"""
    out = np.zeros((4, 4), T.dtype)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((T[r, 0] * S[0, c] + T[r, 1] * S[1, c]) + T[r, 2] * S[2, c]) + T[r, 3] * S[3, c]
    return out


def box_values(P1, P2, opts):
    """o and mu0 of the kept rows, in float64 as the contract defines them"""
    lo1, hi1, lo2, hi2 = P1.min(axis=0), P1.max(axis=0), P2.min(axis=0), P2.max(axis=0)
    o = 0.5 * lo1 + 0.5 * hi1
    d1, d2 = hi1 - lo1, hi2 - lo2
    a, b = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2], (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2]
    mu0 = float(opts["mu0"]) if float(opts["mu0"]) != 0.0 else float(max(a, b))
    return o, mu0


def _failed(n, n_live, n_kept, kept):
    return dict(T=np.zeros((4, 4)), failed=True, n=n, n_live=n_live, n_kept=n_kept, kept=kept, mu0=0.0, mu_final=0.0, cost=0.0, n_inliers=0,
                sum_d2=0.0, inlier_idx=np.zeros(0, np.int32))


def _run(p1, p2, opts, b, tuple_idx, T0, dt, summer):
    p1, p2 = np.asarray(p1, np.float64).reshape(-1, 3), np.asarray(p2, np.float64).reshape(-1, 3)
    n = len(p1)
    live = np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)
    kept = kept_mask(p1, p2, opts, b, tuple_idx)
    rows = np.flatnonzero(kept)
    if len(rows) < 3:
        return _failed(n, int(live.sum()), len(rows), kept)
    o, mu0 = box_values(p1[rows], p2[rows], opts)
    P1, P2, od = p1[rows].astype(dt), p2[rows].astype(dt), o.astype(dt)
    T = np.eye(4, dtype=dt) if T0 is None else np.asarray(T0, np.float64).astype(dt)
    mu, d2, f = mu0, float(opts["delta2"]), float(opts["division_factor"])
    for it in range(int(opts["iterations"])):
        if it > 0 and it % int(opts["decrease_every"]) == 0:
            m = mu / f
            mu = m if m > d2 else d2
        with np.errstate(all="ignore"):
            s = sums28(P1, P2, T, od, dt(mu), summer, dt)
            if dt is LD:
                S = plane_ref.fit(s, 3 * len(rows), o)[0]
            else:
                S = plane_ref.finish64(s, 3 * len(rows), o)
                S = None if S is None else S.reshape(4, 4, order="F")
        if S is None:
            return _failed(n, int(live.sum()), len(rows), kept)
        T = compose(T, S.astype(dt))
    _q, _r, rr = _residuals(P1, P2, T)
    t = dt(mu) / (dt(mu) + rr)
    inl = rr <= d2
    return dict(T=T.astype(np.float64), failed=False, n=n, n_live=int(live.sum()), n_kept=len(rows), kept=kept, mu0=mu0, mu_final=mu,
                cost=float(summer((t * t) * rr)), n_inliers=int(inl.sum()), sum_d2=float(summer(np.where(inl, rr, dt(0.0)))),
                inlier_idx=(rows[inl] + 1).astype(np.int32))


def run_ld(p1, p2, opts, b=0, tuple_idx=None, T0=None):
    return _run(p1, p2, opts, b, tuple_idx, T0, LD, _ld_sum)


def run64(p1, p2, opts, b=0, tuple_idx=None, T0=None):
    return _run(p1, p2, opts, b, tuple_idx, T0, np.float64, _seq_sum)


def run_tree(p1, p2, opts, b=0, tuple_idx=None, T0=None):
    return _run(p1, p2, opts, b, tuple_idx, T0, np.float64, tree_sum)


def tail64(p1, p2, kept, T, mu, delta2):
    """the counts of a given T in float64 and the device's sum order -> n_inliers, inlier_idx (1-based), sum_d2, cost"""
    rows = np.flatnonzero(kept)
    _q, _r, rr = _residuals(np.asarray(p1, np.float64)[rows], np.asarray(p2, np.float64)[rows], np.asarray(T, np.float64))
    t = mu / (mu + rr)
    inl = rr <= delta2
    return int(inl.sum()), (rows[inl] + 1).astype(np.int32), tree_sum(np.where(inl, rr, 0.0)), tree_sum((t * t) * rr)


def method_error(lds, r64s):
    """per OUTPUT |run64 - run_ld| over the registrations of one call that both computations fit: T in Frobenius norm, cost relative,
    each the WORST over them and never below E_FLOOR (tests/cpd_ref.py: method_error says why) -> dict"""
    both = [(a, c) for a, c in zip(lds, r64s) if not a["failed"] and not c["failed"]]
    if not both:
        return dict(T=float("nan"), cost=float("nan"))
    return dict(T=max(max(float(np.linalg.norm(a["T"] - c["T"])) for a, c in both), E_FLOOR),
                cost=max(max(abs(a["cost"] - c["cost"]) / abs(a["cost"]) for a, c in both), E_FLOOR))
