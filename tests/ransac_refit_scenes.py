"""Scenes for the refit tests (test_gpu_ransac_refit.py), built and judged on the host with the oracle alone.

Every scene starts from conftest.rigid_case(n, seed, noise=0.0, outlier_frac=0.3) and gets KNIFE-EDGE rows: every other
inlier row of p1 is moved by a vector v of squared length thDist (1 + s delta), s = +-1, delta log-uniform in
[dlo, 1e-4] (dlo = 1e-9; 1e-7 in the georef scenes, see scene()), thDist = 0.05.  A hypothesis from three untouched inlier rows
reproduces the scene's motion to rounding, so its first pass keeps the untouched rows and the rows with s = -1.

The vectors of the s = -1 rows are BALANCED: sum v = 0 and sum (m - cm) v^T = 0 over them (m their p2 rows, cm the centroid
of the whole first-pass inlier set).  The refit of that inlier set is then the scene's motion again, to rounding -- the
moved rows add nothing to the centroid or to H -- and every knife-edge row is as close to the threshold in the SECOND
pass as it was in the first.  Without the balance the refit would shift by ~|v| / sqrt(K) ~ 4e-3 and no row would stay
within 1e-6 of the threshold: the refined count would not see a refit that is wrong in the ninth digit.  With it, a
relative error of delta * thDist / (2 |v| |x|) in T moves a row across.

A scene variant derives from the base scene of its n by an exact or nearly exact map (one row replaced, a translation,
a scaling), which keeps the balance.  Each has eight hypotheses (a sample table of eight rows, one call each).

prepare(scene) returns the scene with the oracle's answer per hypothesis, the reference refit T_x, which hypotheses are
usable, and asserts the conditions that keep the test honest:
  * usable = the oracle's refined inlier set is the same for T_oracle and for T_x (the reference can decide it); at most
    2 of 8 may be unusable;
  * the scene bites: for some usable hypothesis at least 20 knife-edge rows with delta < 1e-6 lie within 1e-6 (relative)
    of thDist on EACH side of it under the oracle's refit.
"""
from __future__ import annotations

import functools

import numpy as np

from conftest import rigid_case
from ransac_refit_ref import refit_reference

TH = 0.05
BOX = np.array([30.0, 20.0, 25.0])
CENTRE = np.array([40.0, 25.0, 50.0])
EXTENT = 2.0 * float(np.linalg.norm(BOX))          # diameter of the inlier box
N_HYP = 8

# the window of the chunk_edge scenes: the refit sums run in chunks of kMomSlots = 44 slots of 64 rows = 2816 rows
CHUNK = 2816
WINDOW = np.arange(CHUNK - 40, CHUNK + 41)


def _balanced(rng, m, cm, lens):
    """k vectors of the given lengths with sum v = 0 and sum (m - cm) v^T = 0: alternate the projection onto the twelve
    linear constraints with the rescaling to the lengths (which ends the loop, so the lengths are exact)."""
    v = rng.normal(size=(len(m), 3))
    v *= (lens / np.linalg.norm(v, axis=1))[:, None]
    B = np.hstack([np.ones((len(m), 1)), m - cm])
    for _ in range(200):
        v -= B @ np.linalg.lstsq(B, v, rcond=None)[0]
        v *= (lens / np.linalg.norm(v, axis=1))[:, None]
        if np.abs(B.T @ v).max() < 1e-11:
            break
    assert np.abs(B.T @ v).max() < 1e-9, "the knife-edge vectors did not balance"
    return v


def _triples(rng, rows, p2, count):
    """`count` distinct triples of `rows` with large triangles (a well-conditioned three-point fit), 1-based."""
    cand = np.stack([rng.choice(rows, 3, replace=False) for _ in range(max(40 * count, 84))])
    cand = np.unique(np.sort(cand, axis=1), axis=0)
    a, b, c = p2[cand[:, 0]], p2[cand[:, 1]], p2[cand[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return (cand[np.argsort(-area)[:count]] + 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _base(n, dlo=1e-9, window=False):
    """The base scene of size n.  window: the chunk_edge variant -- rows WINDOW follow a second motion B; nine of them stay
    untouched (the samples come from those), the other 72 are knife-edge rows of B with delta in [dlo, 1e-6] (81 rows
    cannot hold 20 rows below 1e-6 on each side at the full range), half on each side, the inner ones balanced."""
    from oracle import pcreg_oracle as o
    p1, p2, T = rigid_case(n, 7000 + n, noise=0.0, outlier_frac=0.3)
    p1 = p1.copy(); p2 = p2.copy()
    rng = np.random.default_rng(n + 1)
    for r in (0, n // 2):                               # rows 0 and n // 2 are outliers in every scene
        p1[r] = CENTRE + rng.uniform(-1, 1, 3) * BOX * 1.5
    R, t = T[:3, :3], T[3, :3]
    inl = np.flatnonzero(np.linalg.norm(p1 - (p2 @ R + t), axis=1) < 1e-9)
    plain, knife = inl[1::2], inl[::2]
    k = len(knife)
    sign = rng.choice([-1.0, 1.0], k)
    delta = 10.0 ** rng.uniform(np.log10(dlo), -4.0, k)
    lens = np.sqrt(TH * (1.0 + sign * delta))
    v = rng.normal(size=(k, 3)); v *= (lens / np.linalg.norm(v, axis=1))[:, None]
    inner = sign < 0
    first = np.concatenate([plain, knife[inner]])
    v[inner] = _balanced(rng, p2[knife[inner]], p2[first].mean(axis=0), lens[inner])
    p1[knife] += v
    sample_rows = plain
    if window:
        RB = o.eul2rotm(rng.uniform(-1, 1, 3)); tB = rng.uniform(-5, 5, 3)
        p1[WINDOW] = p2[WINDOW] @ RB + tB
        T = np.eye(4); T[:3, :3] = RB; T[3, :3] = tB
        pick = rng.permutation(len(WINDOW))
        sample_rows, knife = WINDOW[np.sort(pick[:9])], WINDOW[np.sort(pick[9:])]
        k = len(knife)
        sign = np.where(rng.permutation(k) % 2 == 0, -1.0, 1.0)
        delta = 10.0 ** rng.uniform(np.log10(dlo), -6.0, k)
        lens = np.sqrt(TH * (1.0 + sign * delta))
        v = rng.normal(size=(k, 3)); v *= (lens / np.linalg.norm(v, axis=1))[:, None]
        inner = sign < 0
        first = np.concatenate([sample_rows, knife[inner]])
        v[inner] = _balanced(rng, p2[knife[inner]], p2[first].mean(axis=0), lens[inner])
        p1[knife] += v
    table = _triples(rng, sample_rows, p2, N_HYP)
    for a in (p1, p2, knife, delta, table):
        a.setflags(write=False)
    outl = np.setdiff1d(np.arange(1, n), np.concatenate([inl, WINDOW if window else inl[:0], np.array([n // 2])]))
    for a in (plain, outl):
        a.setflags(write=False)
    return dict(p1=p1, p2=p2, th=TH, knife=knife, delta=delta, table=table, ratio=0.004 if window else 0.2, T=T, plain=plain, outliers=outl)


def _far_point(f, salt):
    u = np.random.default_rng(salt).normal(size=3)
    return CENTRE + u / np.linalg.norm(u) * f * EXTENT


_FAR = ["%s-%s-%s" % (k, w, f) for k in ("far_row0", "far_other") for w in ("p1", "p2", "both") for f in ("1e2", "1e4", "1e6")]
STAGED_N = 5633                  # 2 x 44 x 64 + 1: the third chunk of the refit sums holds one correspondence
# rows beyond the reach of the staged chain's record grid (16 median distances from the origin) that ARE inliers: 5 of them in
# different 32-row steps of the digit table (listed by several lanes; the refit must leave the matrix-core sums), and 40 inliers
# + 30 outliers (more than the list holds: every refit leaves them)
_OFF_GRID = ["far_inliers-5", "far_many-40-30"]
STAGED_SCENES = [(name, STAGED_N) for name in ["base"] + _FAR + _OFF_GRID + ["georef", "georef_zero", "scaled-1e-4", "scaled-1e4"]] \
    + [("chunk_edge", n) for n in (4096, 2 * CHUNK, 2 * CHUNK + 1)]
# the scenes that move the origin (row 0), at the sizes of the kernels the host tier runs: the LDS-resident kernel (1500), the
# fp64 kernel on the raw coordinates (2500: a registration above the resident classes) and the tiled kernel (3500)
HOST_SCENES = [(name, n) for n in (1500, 2500, 3500) for name in [s for s in _FAR if s.startswith("far_row0")] + ["georef", "georef_zero"]]
ALL_SCENES = STAGED_SCENES + HOST_SCENES

FAR_F = 30.0                     # the reach is 16 median distances of ~0.5 extents each: 30 extents lie well beyond it
GEO1 = np.array([4.2e6, -3.9e6, 5.1e5])
GEO2 = np.array([-3.7e6, 4.4e6, 6.3e5])


def scene(name, n):
    """name: base | far_row0-<p1|p2|both>-<f> | far_other-<..>-<f> | far_inliers-<k> | far_many-<inliers>-<outliers> | georef |
    georef_zero | scaled-<s> | chunk_edge."""
    kind, _, rest = name.partition("-")
    arg = rest.split("-", 1)
    if kind == "chunk_edge":
        return dict(_base(n, window=True), name=name, n=n)
    # georef: the lower delta is raised to 1e-7, the first rung of the ladder tried on the host (1e-9, 1e-8, 3e-8, 1e-7) at which
    # no more than 2 of 8 hypotheses drop -- none does, at n = 1500, 2500, 3500 and 5633.  Coordinates of 4e6 carry an absolute
    # rounding of ~1e-9 and the oracle's own refit there is off by e_ref ~ 2e-8.  With delta from 1e-9 the first pass no longer
    # reproduces the planned inlier set (the balance breaks and no row stays within 1e-6 of the threshold); from 1e-8 the reference
    # cannot decide 3 of the 8 hypotheses; from 3e-8 it cannot decide any of the 8 (about 50 rows differ in each).
    s = dict(_base(n, dlo=1e-7 if kind.startswith("georef") else 1e-9), name=name, n=n)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    if kind in ("far_row0", "far_other"):
        row = 0 if kind == "far_row0" else n // 2
        f = float(arg[1])
        if arg[0] in ("p1", "both"):
            p1[row] = _far_point(f, 1)
        if arg[0] in ("p2", "both"):
            p2[row] = _far_point(f, 2)
    elif kind in ("far_inliers", "far_many"):
        # true inliers FAR_F inlier extents from the centre, in all directions: p1 = p2 R + t there too, so they sit in the first-pass
        # mask and in the refit (exact rows leave the balance of the knife-edge rows alone); far outliers in p1 beside them
        rng = np.random.default_rng(len(name))
        R, t = s["T"][:3, :3], s["T"][3, :3]
        cand = s["plain"][~np.isin(s["plain"], s["table"] - 1)]
        rows = cand[np.linspace(0, len(cand) - 1, int(arg[0])).astype(int)]
        assert len(np.unique(rows // 32)) == len(rows)                     # each in a digit step of its own
        u = rng.normal(size=(len(rows), 3)); u /= np.linalg.norm(u, axis=1)[:, None]
        p2[rows] = CENTRE + u * FAR_F * EXTENT
        p1[rows] = p2[rows] @ R + t
        if kind == "far_many":
            out = s["outliers"][np.linspace(0, len(s["outliers"]) - 1, int(arg[1])).astype(int)]
            u = rng.normal(size=(len(out), 3)); u /= np.linalg.norm(u, axis=1)[:, None]
            p1[out] = CENTRE + u * FAR_F * EXTENT
        s["far_inliers"] = rows
    elif kind in ("georef", "georef_zero"):
        p1 += GEO1; p2 += GEO2
        if kind == "georef_zero":
            p1[0] = 0.0; p2[0] = 0.0
    elif kind == "scaled":
        f = float(rest)
        p1 *= f; p2 *= f; s["th"] = TH * f * f
    else:
        assert kind == "base", name
    s["p1"], s["p2"] = p1, p2
    return s


def off_grid_rows(p1, p2):
    """Host mirror of the staged chain's grid (ransac.hip: ransac_origin, kGridReach = 16): the origin is, of 31 evenly spread
    rows, the one at the median distance from row 0; a row is off the grid when it lies further than 16 times the median distance
    of those 31 rows from the origin, in either point set.  Used to assert that a scene reaches the branches it is built for."""
    n = len(p1)
    rows = (np.arange(31) * (n - 1)) // 30
    q = np.hstack([p1[rows], p2[rows]])
    key = ((q - np.hstack([p1[0], p2[0]])) ** 2).sum(axis=1)
    o = q[np.lexsort((np.arange(31), key))[15]]
    g1 = 256.0 * np.sort(((q[:, :3] - o[:3]) ** 2).sum(axis=1))[15]; g2 = 256.0 * np.sort(((q[:, 3:] - o[3:]) ** 2).sum(axis=1))[15]
    return np.flatnonzero((((p1 - o[:3]) ** 2).sum(axis=1) > g1) | (((p2 - o[3:]) ** 2).sum(axis=1) > g2))


def coef_of(s, refine=True):
    return dict(minPtNum=3, iterNum=1, thDist=s["th"], thInlrRatio=s["ratio"], REFINE=refine, VERBOSE=0)


@functools.lru_cache(maxsize=None)
def prepare(name, n):
    """The scene with, per hypothesis, the oracle's answers (refined run `ref`, first pass `ref1`), the reference refit Tx
    on the oracle's first-pass inlier rows, e_ref and `usable`; asserts the honesty conditions of the module docstring."""
    from oracle import c_oracle
    c_oracle.build()
    s = scene(name, n)
    p1, p2, th = s["p1"], s["p2"], s["th"]
    small = np.zeros(n, bool); small[s["knife"][s["delta"] < 1e-6]] = True
    hyps, cache, bites = [], {}, False
    for row in s["table"]:
        tab = row[None, :]
        far_rows = [0] if name == "chunk_edge" else [0, n // 2]          # (the window of chunk_edge may hold row n // 2)
        assert not np.isin(far_rows, row - 1).any()
        ref = c_oracle.ransac(p1, p2, coef_of(s), sample_idx=tab)
        ref1 = c_oracle.ransac(p1, p2, coef_of(s, refine=False), sample_idx=tab)
        assert not ref["failed"] and not ref1["failed"] and ref["numSuccess"] == 1, name
        rows = ref1["inlierIdx"] - 1
        assert len(rows) == ref["inlrNum"][0] and ref["maxInliers"] == ref["inlrNum_refined"][0]
        assert not np.isin(far_rows, rows).any(), "rows 0 and n // 2 must be outliers"
        if "far_inliers" in s:                              # the off-grid branches: listed rows inside the mask; the list overflowing
            off = off_grid_rows(p1, p2)
            assert np.isin(s["far_inliers"], rows).all() and np.isin(s["far_inliers"], off).all()
            assert (len(off) == 5) if name.startswith("far_inliers") else (len(off) == 70 > 62), len(off)
        key = rows.tobytes()
        if key not in cache:
            cache[key] = refit_reference(p1, p2, rows)
        Tx = cache[key]
        d_or = c_oracle.calcDists(ref["T"], p1, p2); d_x = c_oracle.calcDists(Tx, p1, p2)
        np.testing.assert_array_equal(np.flatnonzero(d_or < th) + 1, ref["inlierIdx"])
        usable = bool(np.array_equal(d_or < th, d_x < th))
        near = small & (np.abs(d_or / th - 1.0) < 1e-6)
        bite = (int((near & (d_or < th)).sum()), int((near & (d_or >= th)).sum()))
        bites |= usable and min(bite) >= 20
        hyps.append(dict(table=tab, ref=ref, ref1=ref1, Tx=Tx, e_ref=float(np.linalg.norm(ref["T"] - Tx)), usable=usable, bite=bite))
    s["hyps"] = hyps
    s["n_unusable"] = sum(not h["usable"] for h in hyps)
    assert s["n_unusable"] <= 2, (name, n, "the reference cannot decide", s["n_unusable"], "of", len(hyps))
    assert bites, (name, n, "no usable hypothesis has 20 knife-edge rows within 1e-6 on each side", [h["bite"] for h in hyps])
    return s
