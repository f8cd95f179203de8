"""Host-side mirror of the reference's MATLAB interface for the hot path.

Same function names, argument meaning and failure behaviour as the reference .m files
(LCJebe/PCReg); the arithmetic happens in libpcreg_hip.so on an MI355X through the
C ABI of include/pcreg.h (host tier).  Differences forced by the host language only:
MATLAB structs are dicts, ``[]`` is an empty (0, 0) array, indices stay 1-based.

    estimateTransform(pts1, pts2)                          estimateTransform.m:2
    calcDists(T, pts1, pts2)                               getInliersRANSAC.m:46
    ransac(pts1, pts2, ransacCoef, funcFindTransf, funcDist)   ransac.m:1
    getInliersRANSAC(loc1M, loc1S)                         getInliersRANSAC.m:12-42
    getMatches(descSurface, descModel, par)                getMatches.m:1
    AlignPoints_KNN(pts, C1, C2)                           AlignPoints_KNN.m:1
    quickTF(pts, TF) / invertTF(TF)                        quickTF.m:1 / invertTF.m:1
"""
from __future__ import annotations

import ctypes as C

import math

import numpy as np

from . import _lib
from ._lib import KNN_MAX_K, DescOpts, MatchOpts, RansacOpts, check, lib

EMPTY = np.zeros((0, 0))
"""MATLAB's ``[]`` (what estimateTransform / ransac return on failure)."""


def _fcol(a, dtype=np.float64) -> np.ndarray:
    a = np.asarray(a, dtype=dtype)
    if a.ndim != 2:
        raise ValueError("expected a 2-D array")
    return np.asfortranarray(a)


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


def _pts3(a, name: str) -> np.ndarray:
    a = _fcol(a)
    if a.shape[1] != 3:
        raise ValueError(f"{name} must be N x 3")
    return a


# ------------------------------------------------------------------ estimateTransform
def estimateTransform(pts1, pts2) -> np.ndarray:
    """T = estimateTransform(pts1, pts2) with [pts2, 1] * T = [pts1, 1]
    (estimateTransform.m:2-71).  Returns ``EMPTY`` where the reference returns []."""
    p1, p2 = _pts3(pts1, "pts1"), _pts3(pts2, "pts2")
    if p1.shape != p2.shape:
        raise ValueError("pts1 and pts2 must have the same size")
    n = p1.shape[0]
    T = np.zeros(16)
    empty = C.c_int(1)
    check(lib().pcreg_estimate_transform(_ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(n), C.c_int(n),
                                         _ptr(T, C.c_double), C.byref(empty)))
    return EMPTY.copy() if empty.value else T.reshape(4, 4, order="F").copy()


def calcDists(T, pts1, pts2) -> np.ndarray:
    """d = calcDists(T, pts1, pts2): squared distance of pts1 to [pts2,1]*T
    (getInliersRANSAC.m:46-54).  Like the reference it raises on an empty T."""
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("calcDists: T must be 4 x 4 (the reference errors on [] as well, ransac.m:77-79)")
    p1, p2 = _pts3(pts1, "pts1"), _pts3(pts2, "pts2")
    n = p1.shape[0]
    d = np.zeros(n)
    Tf = T.reshape(-1, order="F").copy()
    check(lib().pcreg_calc_dists(_ptr(Tf, C.c_double), _ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(n),
                                 C.c_int(n), _ptr(d, C.c_double)))
    return d


# ------------------------------------------------------------------------------ ransac
def _ransac_opts(coef: dict, seed: int = 0) -> RansacOpts:
    for k in ("minPtNum", "iterNum", "thInlrRatio", "thDist", "REFINE"):     # ransac.m:23-29
        if k not in coef:
            raise KeyError(f"ransacCoef.{k} is required (ransac.m:23-29)")
    return RansacOpts(int(coef["minPtNum"]), int(coef["iterNum"]), float(coef["thDist"]),
                      float(coef["thInlrRatio"]), int(bool(coef["REFINE"])),
                      int(bool(coef.get("VERBOSE", 1))), int(seed) & ((1 << 64) - 1))


def _matlab_round(x: float) -> int:
    return int(np.floor(abs(x) + 0.5) * (1 if x >= 0 else -1))


def ransac(pts1, pts2, ransacCoef: dict, funcFindTransf=None, funcDist=None, *, sample_idx=None,
           seed: int = 0, return_iter_counts: bool = False):
    """[T, inlierIdx, numSuccess, maxInliers, ratio] = ransac(pts1, pts2, ransacCoef,
    @estimateTransform, @calcDists)   (ransac.m:1-118).

    With the handles every caller of the reference passes (``estimateTransform`` and
    ``calcDists`` of this module, or None) the whole loop runs on the GPU.  Any other
    pair of handles runs the reference's generic loop on the host, calling the handles.

    sample_idx (iterNum x minPtNum, 1-based) replaces ``randperm(ptNum)(1:minPtNum)``
    (ransac.m:42-43); None selects the built-in counter-based sampler seeded by `seed`.
    Failure mirrors ransac.m:77-89: T = EMPTY, inlierIdx empty, numSuccess = maxInliers = 0.
    """
    fit_is_ours = funcFindTransf is None or funcFindTransf is estimateTransform
    dist_is_ours = funcDist is None or funcDist is calcDists
    if not (fit_is_ours and dist_is_ours):
        return _ransac_generic(pts1, pts2, ransacCoef, funcFindTransf or estimateTransform,
                               funcDist or calcDists, sample_idx, seed)
    p1, p2 = _pts3(pts1, "pts1"), _pts3(pts2, "pts2")
    if p1.shape != p2.shape:
        raise ValueError("pts1 and pts2 must have the same size")
    n = p1.shape[0]
    o = _ransac_opts(ransacCoef, seed)
    si_ptr = None
    if sample_idx is not None:
        si = np.ascontiguousarray(sample_idx, dtype=np.int32)
        if si.shape != (o.iterNum, o.minPtNum):
            raise ValueError("sample_idx must be iterNum x minPtNum")
        if n and (si.min() < 1 or si.max() > n):
            raise ValueError("sample_idx entries must lie in 1..ptNum")
        si_ptr = _ptr(si, C.c_int32)
    T = np.zeros(16)
    inl = np.zeros(max(n, 1), dtype=np.int32)
    ni, ns, mi, fl = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(1)
    it1 = np.zeros(o.iterNum, dtype=np.int32) if return_iter_counts else None
    it2 = np.zeros(o.iterNum, dtype=np.int32) if return_iter_counts else None
    check(lib().pcreg_ransac(_ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(n), C.c_int(n), C.byref(o), si_ptr,
                             _ptr(T, C.c_double), _ptr(inl, C.c_int32), C.byref(ni), C.byref(ns), C.byref(mi),
                             C.byref(fl), _ptr(it1, C.c_int32) if it1 is not None else None,
                             _ptr(it2, C.c_int32) if it2 is not None else None))
    if fl.value:
        if o.VERBOSE:
            print("RANSAC could not find an appropriate transformation")                 # ransac.m:82
        out = (EMPTY.copy(), np.zeros(0), 0, 0, 0.0)
    else:
        if o.VERBOSE:                                                                     # ransac.m:100
            print("RANSAC succeeded %d times with a maximum of %d Inliers (%0.2f %%)"
                  % (ns.value, mi.value, 100.0 * mi.value / n))
        out = (T.reshape(4, 4, order="F").copy(), inl[:ni.value].astype(np.float64), ns.value, mi.value,
               100.0 * mi.value / n)
    if return_iter_counts:
        return out + (it1, it2)
    return out


def _ransac_generic(pts1, pts2, coef, fit, dist, sample_idx, seed):
    """ransac.m:21-116 for arbitrary function handles (host loop; the handles do the math)."""
    pts1 = np.asarray(pts1, dtype=np.float64)
    pts2 = np.asarray(pts2, dtype=np.float64)
    minPtNum, iterNum = int(coef["minPtNum"]), int(coef["iterNum"])
    thDist, ptNum = float(coef["thDist"]), pts1.shape[0]
    thInlr = _matlab_round(float(coef["thInlrRatio"]) * ptNum)
    REFINE, VERBOSE = bool(coef["REFINE"]), bool(coef.get("VERBOSE", 1))
    rng = np.random.default_rng(seed)
    inlrNum = np.zeros(iterNum, dtype=np.int64)
    inlrNum_refined = np.zeros(iterNum, dtype=np.int64)
    TForms = [None] * iterNum

    def _empty(f):
        return f is None or (isinstance(f, np.ndarray) and f.size == 0)

    for p in range(iterNum):
        s = (np.asarray(sample_idx[p]) - 1) if sample_idx is not None else rng.permutation(ptNum)[:minPtNum]
        f1 = fit(pts1[s], pts2[s])
        d = dist(f1, pts1, pts2)        # like ransac.m:48 this raises if f1 is empty
        inl = np.nonzero(np.asarray(d) < thDist)[0]
        inlrNum[p] = inl.size
        if inl.size >= thInlr:
            if REFINE:
                f2 = fit(pts1[inl], pts2[inl])
                d = dist(f2, pts1, pts2)
                inlrNum_refined[p] = int(np.sum(np.asarray(d) < thDist))
                if inlrNum_refined[p] >= thInlr:
                    TForms[p] = f2
            else:
                TForms[p] = f1
    counts = inlrNum_refined if REFINE else inlrNum
    idx = int(np.argmax(counts)) if iterNum else 0
    T = TForms[idx] if iterNum else None
    try:
        if _empty(T):
            raise ValueError("empty transform")
        d = dist(T, pts1, pts2)
    except Exception:
        if VERBOSE:
            print("RANSAC could not find an appropriate transformation")
        return EMPTY.copy(), np.zeros(0), 0, 0, 0.0
    inlierIdx = (np.nonzero(np.asarray(d) < thDist)[0] + 1).astype(np.float64)
    numSuccess, maxInliers = int(np.sum(counts >= thInlr)), int(counts[idx])
    if VERBOSE:
        print("RANSAC succeeded %d times with a maximum of %d Inliers (%0.2f %%)"
              % (numSuccess, maxInliers, 100.0 * maxInliers / ptNum))
    return T, inlierIdx, numSuccess, maxInliers, 100.0 * maxInliers / ptNum


def ransac_batched(pts1_list, pts2_list, ransacCoef: dict, *, sample_idx=None, seed: int = 0):
    """B independent registrations in one launch (the parfor of
    completeExperimentFast.m:201-225).  Returns a list of ransac() 5-tuples."""
    B = len(pts1_list)
    if B == 0:
        return []
    sizes = [np.asarray(p).shape[0] for p in pts1_list]
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    total = int(offsets[-1])
    p1 = _pts3(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in pts1_list], axis=0), "pts1")
    p2 = _pts3(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in pts2_list], axis=0), "pts2")
    o = _ransac_opts(ransacCoef, seed)
    si_ptr = None
    if sample_idx is not None:
        si = np.ascontiguousarray(sample_idx, dtype=np.int32)
        if si.shape != (B, o.iterNum, o.minPtNum):
            raise ValueError("sample_idx must be B x iterNum x minPtNum")
        si_ptr = _ptr(si, C.c_int32)
    T = np.zeros(16 * B)
    inl = np.zeros(max(total, 1), dtype=np.int32)
    ni = np.zeros(B, dtype=np.int32); ns = np.zeros(B, dtype=np.int32)
    mi = np.zeros(B, dtype=np.int32); fl = np.zeros(B, dtype=np.int32)
    check(lib().pcreg_ransac_batched(_ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(total), C.c_int(total),
                                     _ptr(offsets, C.c_int32), C.c_int(B), C.byref(o), si_ptr, _ptr(T, C.c_double),
                                     _ptr(inl, C.c_int32), _ptr(ni, C.c_int32), _ptr(ns, C.c_int32),
                                     _ptr(mi, C.c_int32), _ptr(fl, C.c_int32)))
    out = []
    for b in range(B):
        if fl[b]:
            out.append((EMPTY.copy(), np.zeros(0), 0, 0, 0.0))
        else:
            a = int(offsets[b])
            out.append((T[16 * b:16 * b + 16].reshape(4, 4, order="F").copy(),
                        inl[a:a + int(ni[b])].astype(np.float64), int(ns[b]), int(mi[b]),
                        100.0 * int(mi[b]) / max(sizes[b], 1)))
    return out


# ------------------------------------------------------------- fast global registration
FGR_DEFAULTS = dict(iterations=128, decrease_every=4, division_factor=1.4, mu0=0.0, n_tuples=0, tuple_scale=0.95, seed=0)
"""What fgr / fgr_batched take where `opts` leaves a key out; delta2 has no default."""


def _fgr_opts(opts: dict):
    from ._lib import FgrOpts
    if "delta2" not in opts:
        raise KeyError("opts['delta2'] is required: the SQUARED distance at which a pair stops counting")
    unknown = set(opts) - set(FGR_DEFAULTS) - {"delta2"}
    if unknown:
        raise KeyError(f"unknown fast-global-registration options {sorted(unknown)}")
    o = {**FGR_DEFAULTS, **opts}
    return FgrOpts(float(o["delta2"]), int(o["iterations"]), int(o["decrease_every"]), float(o["division_factor"]), float(o["mu0"]),
                   int(o["n_tuples"]), 0, float(o["tuple_scale"]), int(o["seed"]) & ((1 << 64) - 1))


def fgr_batched(pts1_list, pts2_list, opts: dict, tuple_idx=None, *, T0=None):
    """Fast global registration (MATLAB's pcregisterfgr on matched pairs; pcreg_fgr_batched's contract, include/pcreg.h) of B
    independent sets of matched pairs in one call: [pts2, 1] * T = [pts1, 1].  opts: delta2 (required) and any of FGR_DEFAULTS'
    keys.  tuple_idx: B x n_tuples x 3 1-based triples for the tuple test in place of the built-in ones (seed + b); T0: B x 4 x 4
    start transforms.  Returns one dict per registration: T (4 x 4, EMPTY when failed), failed, n_live, n_kept, mu0, mu_final,
    cost, n_inliers, sum_d2, inlier_idx (1-based, ascending, int32) and kept (bool per pair).  Deterministic: no samples, no
    hypotheses, every sum in one fixed order."""
    from ._lib import FgrResult
    B = len(pts1_list)
    if B == 0:
        return []
    if len(pts2_list) != B:
        raise ValueError("pts1_list and pts2_list differ in length")
    sizes = [np.asarray(p).reshape(-1, 3).shape[0] for p in pts1_list]
    if sizes != [np.asarray(p).reshape(-1, 3).shape[0] for p in pts2_list]:
        raise ValueError("a registration's pts1 and pts2 differ in size")
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    total = int(offsets[-1])
    p1 = _pts3(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in pts1_list], axis=0), "pts1")
    p2 = _pts3(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in pts2_list], axis=0), "pts2")
    o = _fgr_opts(opts)
    ti = None
    if tuple_idx is not None:
        ti = np.ascontiguousarray(tuple_idx, dtype=np.int32)
        if ti.shape != (B, o.n_tuples, 3):
            raise ValueError("tuple_idx must be B x n_tuples x 3")
    t0 = None
    if T0 is not None:
        t0 = np.asarray(T0, dtype=np.float64)
        if t0.shape != (B, 4, 4):
            raise ValueError("T0 must be B x 4 x 4")
        t0 = np.ascontiguousarray(t0.transpose(0, 2, 1))                         # (each 4 x 4 column-major)
    res = (FgrResult * B)()
    inl = np.zeros(max(total, 1), dtype=np.int32)
    kept = np.zeros(max(total, 1), dtype=np.uint8)
    ld = max(total, 1)
    check(lib().pcreg_fgr_batched(p1.ctypes.data, p2.ctypes.data, total, ld, offsets.ctypes.data, B, C.addressof(o),
                                  None if t0 is None else t0.ctypes.data, None if ti is None else ti.ctypes.data, C.addressof(res),
                                  inl.ctypes.data, kept.ctypes.data))
    out = []
    for b in range(B):
        r, a = res[b], int(offsets[b])
        out.append(dict(T=EMPTY.copy() if r.failed else np.array(r.T[:]).reshape(4, 4, order="F"), failed=bool(r.failed), n_live=r.n_live,
                        n_kept=r.n_kept, mu0=r.mu0, mu_final=r.mu_final, cost=r.cost, n_inliers=r.n_inliers, sum_d2=r.sum_d2,
                        inlier_idx=inl[a:a + r.n_inliers].copy(), kept=kept[a:a + sizes[b]].astype(bool)))
    return out


def fgr(pts1, pts2, opts: dict, tuple_idx=None, *, T0=None):
    """fgr_batched for one set of matched pairs: its dict."""
    return fgr_batched([pts1], [pts2], opts, None if tuple_idx is None else np.asarray(tuple_idx)[None],
                       T0=None if T0 is None else np.asarray(T0, dtype=np.float64)[None])[0]


REGISTER_FGR_MATCH = dict(UNNORMALIZE=False, CHANGE_METRIC=False, Method="Exhaustive", MatchThreshold=100.0, MaxRatio=1.0, Metric="SSD",
                          Unique=True, VERBOSE=0)
"""register_fgr's getMatches parameters: every nearest descriptor, kept when the choice is mutual."""


def register_fgr(moving, fixed, grid_step: float, *, max_distance=None, k: int = 16, opts=None, match=None) -> dict:
    """The composition a pcregisterfgr(moving, fixed, gridStep) user expects, over this package's own calls: pcdownsample of both
    clouds at grid_step, point_normals and point_fpfh (k neighbours) on both, getMatches (REGISTER_FGR_MATCH, Unique) of the moving
    descriptors against the fixed ones, then fgr on the matched points with delta2 = max_distance^2 (default grid_step^2):
    [moving, 1] * T = [fixed, 1].  Returns fgr's dict with `matches` (P x 2, 1-based rows of the two downsampled clouds) and the
    clouds `moving_down` / `fixed_down` added."""
    md = pcdownsample(moving, grid_step)[0]
    fd = pcdownsample(fixed, grid_step)[0]
    dm = point_fpfh(md, k, normals=point_normals(md, k))
    df = point_fpfh(fd, k, normals=point_normals(fd, k))
    matches = getMatches(dm, df, {**REGISTER_FGR_MATCH, **(match or {})})
    d = float(grid_step if max_distance is None else max_distance)
    r = fgr(fd[matches[:, 1].astype(np.int64) - 1].astype(np.float64), md[matches[:, 0].astype(np.int64) - 1].astype(np.float64),
            {"delta2": d * d, **(opts or {})})
    r.update(matches=matches, moving_down=md, fixed_down=fd)
    return r


GETINLIERS_COEFF = dict(minPtNum=3, iterNum=int(2e4), thDist=0.5, thInlrRatio=0.1, REFINE=True)
"""coeff of getInliersRANSAC.m:17-31."""


def getInliersRANSAC(loc1M, loc1S, *, sample_idx=None, seed: int = 0, VERBOSE: int = 1) -> dict:
    """The script getInliersRANSAC.m as a function of its two workspace inputs; returns the
    variables it leaves in the workspace (T, inlierPtIdx, pts1_aligned)."""
    pts1 = np.asarray(loc1M, dtype=np.float64)                                  # :12
    pts2 = np.asarray(loc1S, dtype=np.float64)                                  # :13
    coeff = dict(GETINLIERS_COEFF, VERBOSE=VERBOSE)                             # :17-31
    T, inlierPtIdx, *_ = ransac(pts1, pts2, coeff, estimateTransform, calcDists,
                                sample_idx=sample_idx, seed=seed)               # :34
    ws = dict(T=T, inlierPtIdx=inlierPtIdx, coeff=coeff, pts1=pts1, pts2=pts2)
    if T.size:                                                                  # :39
        ws["pts1_aligned"] = quickTF(pts1, T)                                   # :40-41
    return ws


# -------------------------------------------------------------------------- getMatches
def _match_opts(par: dict) -> MatchOpts:
    metric = str(par.get("Metric", "SSD")).upper()
    if metric not in ("SAD", "SSD"):
        raise ValueError("par.Metric must be 'SAD' or 'SSD'")
    method = str(par.get("Method", "Exhaustive"))
    if method not in ("Exhaustive", "Approximate"):
        raise ValueError("par.Method must be 'Exhaustive' or 'Approximate'")
    # 'Approximate' (randomised kd-trees in MATLAB) is answered with the exact search
    return MatchOpts(_lib.METRIC_SAD if metric == "SAD" else _lib.METRIC_SSD,
                     float(par.get("MatchThreshold", 10.0 if metric == "SAD" else 1.0)),
                     float(par.get("MaxRatio", 0.6)), int(bool(par.get("Unique", False))),
                     int(bool(par.get("Prenormalized", False))), int(bool(par.get("UNNORMALIZE", False))),
                     float(par.get("norm_factor", 0.0)), int(bool(par.get("CHANGE_METRIC", False))),
                     float(par.get("metric_factor", 1.0)))


def getLocalPoints(pts, R, c, min_points, max_points):
    """[pts_sphere, dists] = getLocalPoints(pts, R, c, min_points, max_points)  (getLocalPoints.m:1-35): the points within R of c,
    RELATIVE to c, or two empty arrays where MATLAB returns [].  A float32 cloud or centre selects MATLAB's single arithmetic
    (the result is float32 then, as in MATLAB)."""
    p_single = isinstance(pts, np.ndarray) and pts.dtype == np.float32
    c_single = isinstance(c, np.ndarray) and c.dtype == np.float32
    mode = 1 if c_single else (2 if p_single else 0)
    P = _fcol(pts)
    if P.shape[1] != 3:
        raise ValueError("pts must be N x 3")
    N = P.shape[0]
    cc = (C.c_double * 3)(*[float(v) for v in np.asarray(c, dtype=np.float64).ravel()[:3]])
    out = np.zeros((max(N, 1), 3), dtype=np.float64, order="F")
    dists = np.zeros(max(N, 1), dtype=np.float64)
    n = C.c_int(0)
    check(lib().pcreg_get_local_points(_ptr(P, C.c_double), N, max(N, 1), C.c_double(float(R)), cc, C.c_double(float(min_points)),
                                       C.c_double(float(max_points)), mode, _ptr(out, C.c_double), _ptr(dists, C.c_double), C.byref(n)))
    k = n.value
    res = np.ascontiguousarray(out.ravel(order="F")[:3 * k].reshape(k, 3, order="F")), dists[:k].copy()
    if mode:
        return res[0].astype(np.float32), res[1].astype(np.float32)
    return res


class DescSet:
    """A descriptor set resident on the GPU (pcreg_desc_set_create): uploaded once, matched many times -- the surface set and
    the model set of completeExperimentFast.m:101-150.  `with DescSet(desc) as h:` or call close()."""

    def __init__(self, desc):
        d = _fcol(desc)
        self.n, self.D = d.shape
        self._h = C.c_void_p()
        check(lib().pcreg_desc_set_create(_ptr(d, C.c_double), self.n, max(self.n, 1), self.D, C.byref(self._h)))

    def close(self) -> None:
        if self._h:
            lib().pcreg_desc_set_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def getMatchesOnSet(hSurface: DescSet, hModel: DescSet, rows, par: dict) -> np.ndarray:
    """getMatches(descSurface, descModel[rows], par) on resident sets (pcreg_get_matches_on_sets): the same pairs, bit for bit,
    without uploading either matrix again.  rows: 0-based ascending row numbers of the model set, or None for all of it."""
    o = _match_opts(par)
    Q = hSurface.n
    pairs = np.zeros((max(Q, 1), 2), dtype=np.uint32)
    P = C.c_int(0)
    if rows is None:
        rp, nr = None, 0
    else:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).ravel())
        if r.size == 0:
            return np.zeros((0, 2), dtype=np.uint32)
        rp, nr = _ptr(r, C.c_int32), int(r.size)
    check(lib().pcreg_get_matches_on_sets(hSurface._h, hModel._h, rp, nr, C.byref(o), _ptr(pairs, C.c_uint32), None, C.byref(P)))
    return pairs[:P.value].copy()


def getMatchesSegmented(descSurface, descModel, rows_list, par: dict) -> list:
    """[getMatches(descSurface, descModel[rows], par) for rows in rows_list] in ONE library call (pcreg_get_matches_segmented):
    the per-sphere calls of completeExperimentFast.m:131-149.  rows: 0-based ascending row numbers of descModel."""
    dS, dM = _fcol(descSurface), _fcol(descModel)
    if dS.shape[1] != dM.shape[1]:
        raise ValueError("descriptor lengths differ")
    Q, D = dS.shape
    VM = dM.shape[0]
    S = len(rows_list)
    off = np.zeros(S + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows_list])
    rows = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32).ravel() for r in rows_list] + [np.zeros(0, np.int32)]))
    o = _match_opts(par)
    pairs = np.zeros((max(S, 1), max(Q, 1), 2), dtype=np.uint32)
    n_pairs = np.zeros(max(S, 1), dtype=np.int32)
    check(lib().pcreg_get_matches_segmented(_ptr(dS, C.c_double), Q, max(Q, 1), _ptr(dM, C.c_double), VM, max(VM, 1), D,
                                            _ptr(rows, C.c_int32) if rows.size else None, _ptr(off, C.c_int32), S, C.byref(o),
                                            _ptr(pairs, C.c_uint32), _ptr(n_pairs, C.c_int32)))
    return [pairs[z, :n_pairs[z]].copy() for z in range(S)]


def getMatchesSegmentedOnSet(hSurface: DescSet, hModel: DescSet, rows_list, par: dict) -> list:
    """getMatchesSegmented on resident sets (pcreg_get_matches_segmented_on_sets): every sphere of completeExperimentFast.m:131-149
    in one call with only the row lists going up and the pairs coming down."""
    if hSurface.D != hModel.D:
        raise ValueError("descriptor lengths differ")
    Q, S = hSurface.n, len(rows_list)
    off = np.zeros(S + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows_list])
    rows = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32).ravel() for r in rows_list] + [np.zeros(0, np.int32)]))
    o = _match_opts(par)
    pairs = np.zeros((max(S, 1), max(Q, 1), 2), dtype=np.uint32)
    n_pairs = np.zeros(max(S, 1), dtype=np.int32)
    check(lib().pcreg_get_matches_segmented_on_sets(hSurface._h, hModel._h, _ptr(rows, C.c_int32) if rows.size else None, _ptr(off, C.c_int32), S,
                                                    C.byref(o), _ptr(pairs, C.c_uint32), _ptr(n_pairs, C.c_int32)))
    return [pairs[z, :n_pairs[z]].copy() for z in range(S)]


def sphereCounts(featModel, centres, R: float) -> np.ndarray:
    """counts(i) = nnz(vecnorm(featModel - centres(i, :), 2, 2) < R)  (completeExperimentFast.m:52-64, pcreg_sphere_counts)."""
    f, c = _fcol(featModel), _fcol(centres)
    VM, S = f.shape[0], c.shape[0]
    counts = np.zeros(max(S, 1), dtype=np.int32)
    check(lib().pcreg_sphere_counts(_ptr(f, C.c_double), VM, max(VM, 1), _ptr(c, C.c_double), S, max(S, 1), C.c_double(R), _ptr(counts, C.c_int32)))
    return counts[:S].astype(np.int64)


def sphereSweep(hSurface: DescSet, hModel: DescSet, featSurface, featModel, centres, num_desc, R_desc: float, par: dict, putative_thresh: int,
                ransacCoef: dict, seed: int = 0) -> dict:
    """completeExperimentFast.m:101-224 for the spheres `centres` (already filtered by their counts `num_desc` = sphereCounts) in one
    library call on resident descriptor sets (pcreg_sphere_sweep): per-sphere row lists and matches, the spheres above the putative
    threshold and their ransac results.  Keys as pcreg_amd.sweep.SphereSweep.run's."""
    fS, fM, c = _fcol(featSurface), _fcol(featModel), _fcol(centres)
    S = c.shape[0]
    nd = np.ascontiguousarray(num_desc, dtype=np.int32)
    Q = hSurface.n
    tot = int(nd.sum())
    rows = np.zeros(max(tot, 1), dtype=np.int32)
    pairs = np.zeros((max(S, 1), max(Q, 1), 2), dtype=np.uint32)
    n_pairs = np.zeros(max(S, 1), dtype=np.int32)
    trial = np.zeros(max(S, 1), dtype=np.int32)
    nt = C.c_int(0)
    T = np.zeros((max(S, 1), 16)); ns = np.zeros(max(S, 1), dtype=np.int32); mi = np.zeros(max(S, 1), dtype=np.int32); fl = np.zeros(max(S, 1), dtype=np.int32)
    o, rc = _match_opts(par), _ransac_opts(ransacCoef, seed)
    check(lib().pcreg_sphere_sweep(hSurface._h, hModel._h, _ptr(fS, C.c_double), max(fS.shape[0], 1), _ptr(fM, C.c_double), max(fM.shape[0], 1),
                                   _ptr(c, C.c_double), S, max(S, 1), _ptr(nd, C.c_int32), C.c_double(R_desc), C.byref(o), int(putative_thresh), C.byref(rc),
                                   _ptr(rows, C.c_int32), _ptr(pairs, C.c_uint32), _ptr(n_pairs, C.c_int32), _ptr(trial, C.c_int32), C.byref(nt),
                                   _ptr(T, C.c_double), _ptr(ns, C.c_int32), _ptr(mi, C.c_int32), _ptr(fl, C.c_int32)))
    n = nt.value
    off = np.zeros(S + 1, dtype=np.int64); off[1:] = np.cumsum(nd)
    npr = n_pairs[:S].astype(np.int64)
    tr = trial[:n].astype(np.int64)
    return dict(centres=np.asarray(centres, dtype=np.float64), num_desc=nd.astype(np.int64), num_putative=npr,
                matches=[pairs[i, :npr[i]].copy() for i in range(S)], model_rows=[rows[off[i]:off[i + 1]].astype(np.int64) for i in range(S)], trial=tr,
                statsPutative=npr[tr], statsSuccess=ns[:n].astype(np.int64), statsInliers=mi[:n].astype(np.int64),
                statsRatio=np.array([100.0 * mi[t] / npr[tr[t]] if not fl[t] else 0.0 for t in range(n)], dtype=np.float64),
                transforms=[None if fl[t] else T[t].reshape(4, 4, order="F").copy() for t in range(n)])


class SphereModel:
    """What the sphere sweep makes of the MODEL alone (pcreg_sphere_model_create): the kept spheres' row lists and keypoints, the model
    descriptor set restricted to the union of those rows, its powered rows per getMatches options -- one model, many surfaces.
    centres / num_desc: the spheres kept after sphereCounts.  `with SphereModel(...) as sm:` or call close()."""

    def __init__(self, hModel: DescSet, featModel, centres, num_desc, R_desc: float):
        fM, c = _fcol(featModel), _fcol(centres)
        self.S = c.shape[0]
        self.centres = np.asarray(centres, dtype=np.float64).reshape(self.S, 3)
        self.num_desc = np.ascontiguousarray(num_desc, dtype=np.int32)
        tot = int(self.num_desc.sum())
        rows = np.zeros(max(tot, 1), dtype=np.int32)
        self._h = C.c_void_p()
        check(lib().pcreg_sphere_model_create(hModel._h, _ptr(fM, C.c_double), max(fM.shape[0], 1), _ptr(c, C.c_double), self.S, max(self.S, 1),
                                              _ptr(self.num_desc, C.c_int32), C.c_double(R_desc), _ptr(rows, C.c_int32), C.byref(self._h)))
        off = np.zeros(self.S + 1, dtype=np.int64); off[1:] = np.cumsum(self.num_desc)
        self.model_rows = [rows[off[i]:off[i + 1]].astype(np.int64) for i in range(self.S)]

    def close(self) -> None:
        if self._h:
            lib().pcreg_sphere_model_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sphereSweepOnModel(sm: SphereModel, hSurface: DescSet, featSurface, par: dict, putative_thresh: int, ransacCoef: dict, seed: int = 0) -> dict:
    """sphereSweep for one more surface against a prepared SphereModel (pcreg_sphere_sweep_on_model): the same results, without redoing
    what belongs to the model."""
    fS = _fcol(featSurface)
    S, Q = sm.S, hSurface.n
    pairs = np.zeros((max(S, 1), max(Q, 1), 2), dtype=np.uint32)
    n_pairs = np.zeros(max(S, 1), dtype=np.int32)
    trial = np.zeros(max(S, 1), dtype=np.int32)
    nt = C.c_int(0)
    T = np.zeros((max(S, 1), 16)); ns = np.zeros(max(S, 1), dtype=np.int32); mi = np.zeros(max(S, 1), dtype=np.int32); fl = np.zeros(max(S, 1), dtype=np.int32)
    o, rc = _match_opts(par), _ransac_opts(ransacCoef, seed)
    check(lib().pcreg_sphere_sweep_on_model(sm._h, hSurface._h, _ptr(fS, C.c_double), max(fS.shape[0], 1), C.byref(o), int(putative_thresh), C.byref(rc),
                                            _ptr(pairs, C.c_uint32), _ptr(n_pairs, C.c_int32), _ptr(trial, C.c_int32), C.byref(nt), _ptr(T, C.c_double),
                                            _ptr(ns, C.c_int32), _ptr(mi, C.c_int32), _ptr(fl, C.c_int32)))
    n = nt.value
    npr = n_pairs[:S].astype(np.int64)
    tr = trial[:n].astype(np.int64)
    return dict(centres=sm.centres, num_desc=sm.num_desc.astype(np.int64), num_putative=npr,
                matches=[pairs[i, :npr[i]].copy() for i in range(S)], model_rows=sm.model_rows, trial=tr,
                statsPutative=npr[tr], statsSuccess=ns[:n].astype(np.int64), statsInliers=mi[:n].astype(np.int64),
                statsRatio=np.array([100.0 * mi[t] / npr[tr[t]] if not fl[t] else 0.0 for t in range(n)], dtype=np.float64),
                transforms=[None if fl[t] else T[t].reshape(4, 4, order="F").copy() for t in range(n)])


def _moving_transforms(transforms) -> np.ndarray:
    """[K, 16]: invertTF(transCur_k) (:291) column-major, cluster after cluster -- the host arithmetic of FinalStage.run."""
    return np.ascontiguousarray([invertTF(np.asarray(T, dtype=np.float64)).ravel(order="F") for T in transforms], dtype=np.float64).reshape(-1, 16)


def finalStageLimits(pts, transforms) -> np.ndarray:
    """[K, 6] (xmin xmax ymin ymax zmin zmax) of quickTF(pts, invertTF(transCur_k)) for every transCur_k of `transforms`, as the
    library moves the surface (pcreg_final_stage_limits): the box and count of pcRandomUniformSamples (:418-432) for cluster k."""
    P = _pts3(pts, "pts")
    Tm = _moving_transforms(transforms)
    K = Tm.shape[0]
    lim = np.zeros((max(K, 1), 6))
    check(lib().pcreg_final_stage_limits(_ptr(P, C.c_double), P.shape[0], max(P.shape[0], 1), _ptr(Tm, C.c_double), K, _ptr(lim, C.c_double)))
    return lim[:K].copy()


def finalStage(hModel: DescSet, featModel, pts, clusters, sample_pts, descOpt: dict, par: dict, R_desc: float, maxDist: float = 1.5,
               return_matches: bool = True) -> dict:
    """completeExperimentFast.m:280-394 after clusterPoints in ONE library call (pcreg_final_stage) -- pcreg_amd.sweep.FinalStage.run
    at the host tier.  hModel: the no-LRF model descriptors (DescSet); featModel: their keypoints; pts: the surface N x 3;
    clusters = [(locCur, transCur)]; sample_pts[i]: the keypoints drawn for cluster i (S_i x 3, see finalStageLimits).
    Keys as FinalStage.run's, without pts_tform (the moved copies stay in the library) and model_rows; pts_final is N x 3 here."""
    K = len(clusters)
    fM, P = _pts3(featModel, "featModel"), _pts3(pts, "pts")
    locs = _fcol(np.asarray([np.asarray(c[0], dtype=np.float64).ravel()[:3] for c in clusters], dtype=np.float64).reshape(-1, 3))
    Tm = _moving_transforms([c[1] for c in clusters])
    kps = [np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in sample_pts]
    if len(kps) != K:
        raise ValueError(f"{len(kps)} keypoint sets for {K} clusters")
    kp_off = np.zeros(K + 1, dtype=np.int32); kp_off[1:] = np.cumsum([k.shape[0] for k in kps])
    kp = _fcol(np.vstack(kps) if K and kp_off[-1] else np.zeros((0, 3)))
    tot, N = int(kp_off[-1]), P.shape[0]
    i32 = lambda: np.zeros(max(K, 1), dtype=np.int32)
    nk, nd, nm, nc = i32(), i32(), i32(), i32()
    prec = np.zeros(max(K, 1))
    best, empty = C.c_int32(0), C.c_int32(1)
    T = np.zeros(16)
    out = np.zeros((max(N, 1), 3), order="F")
    pairs = np.zeros((max(tot, 1), 2), dtype=np.uint32)
    do, mo = _desc_opts(dict(descOpt, ALIGN_POINTS=False)), _match_opts(par)
    check(lib().pcreg_final_stage(hModel._h, _ptr(fM, C.c_double), max(fM.shape[0], 1), _ptr(P, C.c_double), N, max(N, 1), _ptr(locs, C.c_double),
                                  _ptr(Tm, C.c_double), K, _ptr(kp, C.c_double), _ptr(kp_off, C.c_int32), C.byref(do), C.byref(mo), C.c_double(R_desc),
                                  C.c_double(maxDist), _ptr(nk, C.c_int32), _ptr(nd, C.c_int32), _ptr(nm, C.c_int32), _ptr(nc, C.c_int32),
                                  _ptr(prec, C.c_double), C.byref(best), _ptr(T, C.c_double), C.byref(empty), _ptr(out, C.c_double),
                                  _ptr(pairs, C.c_uint32) if return_matches else None))
    npr = nm[:K].astype(np.int64)
    res = dict(num_keypoints=nk[:K].astype(np.int64), num_desc=nd[:K].astype(np.int64), num_matches=npr, num_close=nc[:K].astype(np.int64),
               precisions=prec[:K].copy(), best=int(best.value), T_refine=None if empty.value else T.reshape(4, 4, order="F").copy(),
               pts_final=np.ascontiguousarray(out[:N]))
    if return_matches:
        res["matches"] = [pairs[kp_off[i]:kp_off[i] + npr[i]].copy() for i in range(K)]
    return res


def getMatches(descSurface, descModel, par: dict) -> np.ndarray:
    """matches = getMatches(descSurface, descModel, par)  (getMatches.m:1-59):
    P x 2 uint32, 1-based [surfaceIdx, modelIdx], ascending in the first column."""
    for k in ("UNNORMALIZE", "CHANGE_METRIC", "Method", "MatchThreshold", "MaxRatio", "Metric", "Unique"):
        if k not in par:
            raise KeyError(f"par.{k} is required (getMatches.m:22-56)")
    import time
    t0 = time.time()                                                            # :12 tic
    dS, dM = _fcol(descSurface), _fcol(descModel)
    if dS.shape[1] != dM.shape[1]:
        raise ValueError("descriptor lengths differ")
    Q, D = dS.shape
    M = dM.shape[0]
    o = _match_opts(par)
    pairs = np.zeros((max(Q, 1), 2), dtype=np.uint32)
    P = C.c_int(0)
    check(lib().pcreg_get_matches(_ptr(dS, C.c_double), C.c_int(Q), C.c_int(Q), _ptr(dM, C.c_double), C.c_int(M),
                                  C.c_int(M), C.c_int(D), C.byref(o), _ptr(pairs, C.c_uint32), None, C.byref(P)))
    if par.get("VERBOSE", 1):
        print("Calculated matches in %0.1f seconds..." % (time.time() - t0))    # :58
    return pairs[:P.value].copy()


def matchFeatures(features1, features2, **kw):
    """The subset of MathWorks matchFeatures that getMatches uses (getMatches.m:51-56):
    returns (indexPairs P x 2 uint32, matchMetric P)."""
    par = dict(Method=kw.get("Method", "Exhaustive"), MatchThreshold=kw.get("MatchThreshold", 10.0),
               MaxRatio=kw.get("MaxRatio", 0.6), Metric=kw.get("Metric", "SSD"), Unique=kw.get("Unique", False),
               Prenormalized=kw.get("Prenormalized", False))
    f1, f2 = _fcol(features1), _fcol(features2)
    Q, D = f1.shape
    M = f2.shape[0]
    o = _match_opts(par)
    pairs = np.zeros((max(Q, 1), 2), dtype=np.uint32)
    met = np.zeros(max(Q, 1))
    P = C.c_int(0)
    check(lib().pcreg_match_features(_ptr(f1, C.c_double), C.c_int(Q), C.c_int(Q), _ptr(f2, C.c_double), C.c_int(M),
                                     C.c_int(M), C.c_int(D), C.byref(o), _ptr(pairs, C.c_uint32),
                                     _ptr(met, C.c_double), C.byref(P)))
    return pairs[:P.value].copy(), met[:P.value].copy()


# ------------------------------------------------------------------------ point search
def knn2_points(query, model):
    """Two nearest model points per query (fp32): (idx [Q,2] 0-based, dist [Q,2] squared)."""
    q, m = _fcol(query, np.float32), _fcol(model, np.float32)
    Q, M = q.shape[0], m.shape[0]
    idx = np.zeros((max(Q, 1), 2), dtype=np.int32)
    dist = np.zeros((max(Q, 1), 2), dtype=np.float32)
    check(lib().pcreg_knn2_points_f32(_ptr(q, C.c_float), C.c_int(Q), C.c_int(Q), _ptr(m, C.c_float), C.c_int(M),
                                      C.c_int(M), _ptr(idx, C.c_int32), _ptr(dist, C.c_float)))
    return idx[:Q], dist[:Q]


def _knn_k(k) -> int:
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must lie in [1, {KNN_MAX_K}], got {k}")
    return k


def knn_points(query, model, k: int):
    """knnsearch(model, query, 'K', k) in fp32: (idx [Q,k] 0-based int32, -1 past M; dist [Q,k] squared float32, +inf past M),
    ordered by (distance, row).  The model is prepared for this call only: keep a Model for repeated searches."""
    k = _knn_k(k)
    q, m = _fcol(query, np.float32), _fcol(model, np.float32)
    Q, M = q.shape[0], m.shape[0]
    idx = np.zeros((max(Q, 1), k), dtype=np.int32)
    dist = np.zeros((max(Q, 1), k), dtype=np.float32)
    check(lib().pcreg_knn_points_f32(_ptr(q, C.c_float), C.c_int(Q), C.c_int(max(Q, 1)), _ptr(m, C.c_float), C.c_int(M),
                                     C.c_int(max(M, 1)), C.c_int(k), _ptr(idx, C.c_int32), _ptr(dist, C.c_float)))
    return idx[:Q], dist[:Q]


def _range_r2(r2) -> float:
    r2 = float(np.float32(r2))
    if not r2 >= 0.0:
        raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
    return r2


def _range_call(call, Q: int):
    """capacity 0 sizes the result, the second call fills it (the library counts again: the host tier keeps no state)"""
    seg_off = np.zeros(Q + 1, dtype=np.int64)
    call(0, seg_off, None, None)
    total = int(seg_off[Q])
    idx = np.zeros(total, dtype=np.int32)
    dist = np.zeros(total, dtype=np.float32)
    if total:
        call(total, seg_off, idx.ctypes.data, dist.ctypes.data)
    return seg_off, idx, dist


def rangesearch_points(query, model, r2: float):
    """rangesearch(model, query, r) in fp32 with r2 = r^2: (seg_off [Q + 1] int64, idx [total] 0-based int32, dist [total]
    squared float32); query i's rows are seg_off[i] .. seg_off[i + 1], every row with distance <= r2, ordered by (distance,
    row).  The model is prepared for this call only: keep a Model for repeated searches."""
    r2 = _range_r2(r2)
    q, m = _fcol(query, np.float32), _fcol(model, np.float32)
    Q, M = q.shape[0], m.shape[0]
    return _range_call(lambda cap, so, i, d: check(lib().pcreg_range_points_f32(q.ctypes.data, Q, max(Q, 1), m.ctypes.data, M, max(M, 1), r2, cap,
                                                                                so.ctypes.data, i, d)), Q)


def _cluster_call(call, M: int):
    label = np.zeros(max(M, 1), dtype=np.int32)
    cl_off = np.zeros(M + 1, dtype=np.int32)
    members = np.zeros(max(M, 1), dtype=np.int32)
    nc = C.c_int32(0)
    call(label.ctypes.data, C.byref(nc), cl_off.ctypes.data, members.ctypes.data)
    return label[:M], cl_off[:nc.value + 1].copy(), members[:M]


def cluster_points(pts, r2: float):
    """clusterPoints(pts, r) in fp32 with r2 = r^2: (label [M] int32, cl_off [C + 1] int32, members [M] int32), 0-based.  The
    clusters are the connected components of the graph "squared distance <= r2" over the rows, numbered in ascending order of
    their smallest row; cluster c is members[cl_off[c] .. cl_off[c + 1]), ascending; a row with a non-finite coordinate is a
    cluster of its own.  The cloud is prepared for this call only: keep a Model for repeated calls."""
    r2 = _range_r2(r2)
    m = _fcol(pts, np.float32)
    M = m.shape[0]
    return _cluster_call(lambda lab, nc, off, mem: check(lib().pcreg_cluster_points_f32(m.ctypes.data, M, max(M, 1), r2, lab, nc, off, mem)), M)


def _dbscan_minpts(minpts) -> int:
    if int(minpts) != minpts or int(minpts) < 1:
        raise ValueError(f"minpts must be a whole number >= 1, got {minpts}")
    return int(minpts)


def _dbscan_call(call, M: int):
    label = np.zeros(max(M, 1), dtype=np.int32)
    core = np.zeros(max(M, 1), dtype=np.uint8)
    cl_off = np.zeros(M + 1, dtype=np.int32)
    members = np.zeros(max(M, 1), dtype=np.int32)
    nc = C.c_int32(0)
    call(label.ctypes.data, C.byref(nc), core.ctypes.data, cl_off.ctypes.data, members.ctypes.data)
    return label[:M], core[:M] != 0, cl_off[:nc.value + 1].copy(), members[:cl_off[nc.value]].copy()


def dbscan_points(pts, r2: float, minpts: int):
    """DBSCAN of the rows of pts in fp32 with r2 = epsilon^2 (MATLAB's dbscan(X, epsilon, minpts), scikit-learn's
    DBSCAN(eps, min_samples=minpts)): (label [M] int32, 0-based, -1 for noise; core [M] bool; cl_off [C + 1] int32; members int32).
    A row is a core row when at least minpts rows, itself included, lie within the radius (squared distance <= r2, inclusive);
    the clusters are the connected components of the core rows, numbered in ascending order of their smallest core row; a
    border row joins the smallest-numbered cluster among its core neighbours; cluster c is members[cl_off[c] .. cl_off[c + 1]),
    ascending, border rows included, noise rows in no cluster.  A row with a non-finite coordinate is noise.  The cloud is
    prepared for this call only: keep a Model for repeated calls."""
    r2, minpts = _range_r2(r2), _dbscan_minpts(minpts)
    m = _fcol(pts, np.float32)
    M = m.shape[0]
    return _dbscan_call(lambda lab, nc, core, off, mem: check(lib().pcreg_dbscan_points_f32(m.ctypes.data, M, max(M, 1), r2, minpts, lab, nc, core,
                                                                                          None, off, mem)), M)


def _normals_args(k, viewpoint):
    k = int(k)
    if not 3 <= k <= KNN_MAX_K:
        raise ValueError(f"k must lie in [3, {KNN_MAX_K}], got {k}")
    vp = None
    if viewpoint is not None:
        vp = np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).ravel())
        if vp.shape != (3,):
            raise ValueError("viewpoint is three numbers or None")
    return k, vp


def _normals_call(call, M: int, vp, variation: bool):
    nrm = np.zeros((max(M, 1), 3), dtype=np.float32, order="F")
    var = np.zeros(max(M, 1), dtype=np.float32) if variation else None
    call(vp.ctypes.data if vp is not None else None, nrm.ctypes.data, max(M, 1), var.ctypes.data if variation else None)
    return (nrm[:M], var[:M]) if variation else nrm[:M]


def point_normals(pts, k: int, viewpoint=None, variation: bool = False):
    """pcnormals(pts, k) in this library's rule (pcreg_model_normals_f32's contract): the normal of every row [M, 3] float32,
    the eigenvector of the smallest eigenvalue of the scatter of the row's k nearest rows (3 <= k <= 32, the row itself among
    them), taken in double.  viewpoint (three numbers): the normal points towards it; None: its component of largest magnitude
    is non-negative.  variation=True also returns lambda_min / (lambda_0 + lambda_1 + lambda_2) [M] float32.  NaN for a
    non-finite row, fewer than three finite rows, coincident neighbours.  The cloud is prepared for this call only: keep a Model
    for repeated calls."""
    k, vp = _normals_args(k, viewpoint)
    m = _fcol(pts, np.float32)
    M = m.shape[0]
    return _normals_call(lambda v, n, ldn, va: check(lib().pcreg_point_normals_f32(m.ctypes.data, M, max(M, 1), k, v, n, ldn, va)), M, vp, variation)


def _fpfh_args(M: int, k, normals, k_normals, viewpoint):
    k = int(k)
    if not 3 <= k <= KNN_MAX_K:
        raise ValueError(f"k (NumNeighbors) must lie in [3, {KNN_MAX_K}], got {k}")
    if normals is not None:
        nrm = _fcol(normals, np.float32)
        if nrm.ndim != 2 or nrm.shape != (M, 3):
            raise ValueError(f"normals are [M, 3] with M = {M} rows, got {nrm.shape}")
        return k, nrm, k, None                  # (k_normals is ignored with normals given; M = 0 has no address to pass)
    kn, vp = _normals_args(k if k_normals is None else k_normals, viewpoint)
    return k, None, kn, vp


def _fpfh_call(call, M: int, nrm, vp, spfh: bool):
    out = np.zeros((max(M, 1), 33), dtype=np.float64, order="F")
    cnt = np.zeros((max(M, 1), 33), dtype=np.uint8) if spfh else None
    call(nrm.ctypes.data if nrm is not None and M else None, max(M, 1), vp.ctypes.data if vp is not None else None, out.ctypes.data, max(M, 1),
         cnt.ctypes.data if spfh else None)
    return (out[:M], cnt[:M]) if spfh else out[:M]


def point_fpfh(pts, k: int, normals=None, k_normals=None, viewpoint=None, spfh: bool = False):
    """extractFPFHFeatures(pts, 'NumNeighbors', k) in this library's rule (pcreg_model_fpfh_f32's contract): the 33-number FPFH
    descriptor of every row, [M, 33] float64, from its k nearest rows (3 <= k <= 32, the row itself among them) and a normal per
    row.  normals: [M, 3] float32 by row, as point_normals returns them -- their SIGN matters, orient them with a viewpoint; None:
    computed in the call from the k_normals nearest rows (default k) and the viewpoint.  Each of the three histograms of a row adds
    up to 100 (or is all zero); a non-finite row is NaN.  spfh=True also returns the SPFH counts [M, 33] uint8.  The cloud is
    prepared for this call only: keep a Model for repeated calls."""
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    k, nrm, kn, vp = _fpfh_args(M, k, normals, k_normals, viewpoint)
    return _fpfh_call(lambda n, ldn, v, o, ldf, c: check(lib().pcreg_point_fpfh_f32(m.ctypes.data, M, max(M, 1), k, n, ldn, kn, v, o, ldf, c)),
                      M, nrm, vp, spfh)


FPFH_RADIUS_MAX_ROWS = 4 << 20             # rows per radius-FPFH call: the radius search's queries per call, one batch


def _fpfh_radius_args(M: int, radius, max_neighbors, normals, k_normals, viewpoint):
    """-> (r2, max_neighbors, normals or None, k_normals, viewpoint): the radius squared in double and the square rounded once to
    float32 (a number >= 0; +inf allowed), the rest as the C tiers take them"""
    r = float(radius)
    if not r >= 0.0:
        raise ValueError(f"radius must be a number >= 0, got {r}")
    with np.errstate(over="ignore"):
        r2 = float(np.float32(r * r))
    n = int(max_neighbors)
    if n < 0:
        raise ValueError(f"max_neighbors must be >= 0 (0: every row within the radius), got {n}")
    if M > FPFH_RADIUS_MAX_ROWS:
        raise ValueError(f"the radius FPFH takes at most {FPFH_RADIUS_MAX_ROWS} rows a call, got {M}")
    if normals is not None:
        nrm = _fcol(normals, np.float32)
        if nrm.ndim != 2 or nrm.shape != (M, 3):
            raise ValueError(f"normals are [M, 3] with M = {M} rows, got {nrm.shape}")
        return r2, n, nrm, 3, None              # (k_normals is ignored with normals given)
    kn, vp = _normals_args(k_normals, viewpoint)
    return r2, n, None, kn, vp


def _fpfh_radius_call(call, M: int, nrm, vp, counts: bool, n_neighbors: bool):
    out = np.zeros((max(M, 1), 33), dtype=np.float64, order="F")
    cnt = np.zeros((max(M, 1), 33), dtype=np.uint32) if counts else None
    nn = np.zeros(max(M, 1), dtype=np.int32) if n_neighbors else None
    call(nrm.ctypes.data if nrm is not None and M else None, max(M, 1), vp.ctypes.data if vp is not None else None, out.ctypes.data, max(M, 1),
         cnt.ctypes.data if counts else None, nn.ctypes.data if n_neighbors else None)
    res = (out[:M],) + ((cnt[:M],) if counts else ()) + ((nn[:M],) if n_neighbors else ())
    return res if len(res) > 1 else res[0]


def point_fpfh_radius(pts, radius, normals=None, max_neighbors: int = 0, k_normals: int = 6, viewpoint=None, counts: bool = False,
                      n_neighbors: bool = False):
    """extractFPFHFeatures(pts, 'Radius', radius) in this library's rule (pcreg_model_fpfh_radius_f32's contract): the 33-number
    FPFH descriptor of every row, [M, 33] float64, from the rows within the radius (inclusive, fp32 distances) and a normal per
    row.  max_neighbors = n > 0 counts only the n nearest of them ('NumNeighbors' beyond the k-nearest form's 32: MATLAB's default
    of 50 is max_neighbors=50 with a radius wide enough; a row with fewer rows inside the radius uses what is there); 0 counts
    all.  normals: [M, 3] float32 by row, as point_normals returns them -- their SIGN matters; None: computed in the call from the
    k_normals nearest rows and the viewpoint.  counts=True also returns the SPFH counts [M, 33] uint32, n_neighbors=True the
    neighbours counted per row [M] int32, in that order.  The lists take 8 bytes per (row, neighbour) pair within the radius on
    the device; at most 4 Mi rows a call.  The cloud is prepared for this call only: keep a Model for repeated calls."""
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    r2, n, nrm, kn, vp = _fpfh_radius_args(M, radius, max_neighbors, normals, k_normals, viewpoint)
    return _fpfh_radius_call(lambda a, ldn, v, o, ldf, c, nn: check(lib().pcreg_point_fpfh_radius_f32(m.ctypes.data, M, max(M, 1), r2, n, a, ldn, kn, v,
                                                                                                      o, ldf, c, nn)), M, nrm, vp, counts, n_neighbors)


def iss_args(salient_radius, nonmax_radius, gamma21, gamma32, min_neighbors):
    """The ISS parameters as the C tiers take them: each radius squared in double and the square rounded once to float32 (the
    rule pcreg_model_iss_f32 states for wrappers that take radii), the thresholds as doubles, min_neighbors as an int."""
    r2 = []
    for name, r in (("salient_radius", salient_radius), ("nonmax_radius", nonmax_radius)):
        r = float(r)
        with np.errstate(over="ignore"):
            sq = np.float32(r * r) if math.isfinite(r) and r > 0.0 else np.float32(np.nan)
        if not (np.isfinite(sq) and sq >= np.finfo(np.float32).tiny):
            raise ValueError(f"{name} must be a finite number > 0 whose square is a normal float32, got {r}")
        r2.append(float(sq))
    g21, g32, mn = float(gamma21), float(gamma32), int(min_neighbors)
    for name, g in (("gamma21", g21), ("gamma32", g32)):
        if not (math.isfinite(g) and g > 0.0):
            raise ValueError(f"{name} must be a finite number > 0, got {g}")
    if mn < 1:
        raise ValueError(f"min_neighbors must be at least 1, got {mn}")
    return r2[0], r2[1], g21, g32, mn


def _iss_call(call, M: int) -> dict:
    nn = np.zeros(max(M, 1), dtype=np.int32)
    eig = np.zeros((max(M, 1), 3), dtype=np.float64)
    sal = np.zeros(max(M, 1), dtype=np.float64)
    kp = np.zeros(max(M, 1), dtype=np.int32)
    n = C.c_int32(0)
    call(nn.ctypes.data, eig.ctypes.data, sal.ctypes.data, kp.ctypes.data, C.byref(n))
    return dict(keypoints=kp[:n.value].copy(), n_neighbors=nn[:M], eig=eig[:M], saliency=sal[:M])


def point_iss(pts, salient_radius, nonmax_radius, gamma21: float = 0.975, gamma32: float = 0.975, min_neighbors: int = 5) -> dict:
    """detectISSFeatures(pts, 'SalientRadius', .., 'NonMaxRadius', .., 'Threshold21', .., 'Threshold32', .., 'MinNeighbors', ..) in
    this library's rule (pcreg_model_iss_f32's contract): a dict with keypoints, the 0-based rows of the ISS keypoints, ascending
    int32 (pts[keypoints] are the points); n_neighbors [M] int32, the rows within salient_radius of every row, itself included;
    eig [M, 3] float64, the eigenvalues of that neighbourhood's covariance, descending (NaN for a non-finite row); saliency [M]
    float64, the smallest eigenvalue of a row that passes the two ratio tests and has min_neighbors rows, else 0.  The radii are
    squared in double and rounded once to float32.  The cloud is prepared for this call only: keep a Model for repeated calls."""
    a = iss_args(salient_radius, nonmax_radius, gamma21, gamma32, min_neighbors)
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    return _iss_call(lambda nn, e, s, kp, n: check(lib().pcreg_point_iss_f32(m.ctypes.data, M, max(M, 1), *a, nn, e, s, kp, n)), M)


def planes_args(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed):
    """The plane extraction's parameters as the C tiers take them (pcreg_model_fit_planes_f32's rules): max_distance as a float32
    whose fp32 square is a normal number, ref_vec as three contiguous float64 or None, and the ranges of the counts."""
    t = np.float32(max_distance)
    tiny = np.finfo(np.float32).tiny
    with np.errstate(over="ignore", under="ignore"):
        t2 = t * t
    if not (np.isfinite(t) and t >= tiny and np.isfinite(t2) and t2 >= tiny):
        raise ValueError(f"max_distance must be a finite number > 0 whose float32 square is a normal number, got {max_distance}")
    rv = None
    ang = 0.0
    if ref_vec is not None:
        rv = np.ascontiguousarray(np.asarray(ref_vec, np.float64).reshape(-1))
        if rv.shape != (3,) or not np.isfinite(rv).all() or not rv.any() or not math.isfinite(float(rv @ rv)):
            raise ValueError("ref_vec must be three finite numbers, not all zero")
        ang = float(max_angle)
        if not (0.0 < ang <= math.pi / 2):
            raise ValueError(f"max_angle must lie in (0, pi/2] radians, got {max_angle}")
    P, B, mi = int(max_planes), int(n_trials), int(min_inliers)
    if not 1 <= P <= 64:
        raise ValueError(f"max_planes must lie in 1 .. 64, got {P}")
    if not 1 <= B <= 1 << 20:
        raise ValueError(f"n_trials must lie in 1 .. 2^20, got {B}")
    if mi < 3:
        raise ValueError(f"min_inliers must be at least 3, got {mi}")
    return float(t), rv, ang, P, B, mi, int(seed) & 0xFFFFFFFFFFFFFFFF


def _planes_samples(samples, P, B):
    if samples is None:
        return None
    smp = np.ascontiguousarray(np.asarray(samples, np.int32))
    if smp.shape != (P, B, 3):
        raise ValueError(f"samples must be [max_planes, n_trials, 3] = {(P, B, 3)}, got {smp.shape}")
    return smp


def _planes_call(call, M: int, P: int) -> dict:
    labels = np.zeros(max(M, 1), dtype=np.int32)
    planes = np.zeros((P, 4), dtype=np.float64)
    centres = np.zeros((P, 3), dtype=np.float64)
    counts = np.zeros(P, dtype=np.int32)
    rmse = np.zeros(P, dtype=np.float64)
    bt = np.zeros(P, dtype=np.int32)
    bc = np.zeros(P, dtype=np.int64)
    bn = np.zeros(P, dtype=np.int32)
    n = C.c_int32(0)
    call(labels.ctypes.data, planes.ctypes.data, centres.ctypes.data, counts.ctypes.data, rmse.ctypes.data, C.byref(n), bt.ctypes.data,
         bc.ctypes.data, bn.ctypes.data)
    return dict(n_planes=int(n.value), labels=labels[:M], planes=planes, centres=centres, counts=counts, rmse=rmse, best_trial=bt,
                best_cost=bc, best_count=bn)


def point_fit_planes(pts, max_distance, ref_vec=None, max_angle=math.pi / 2, max_planes: int = 1, n_trials: int = 1000,
                     min_inliers: int = 3, seed: int = 0, samples=None) -> dict:
    """pcfitplane(pts, maxDistance[, referenceVector, maxAngularDistance]) and the fit / remove / fit-again loop, up to max_planes
    times in one call, in this library's rule (pcreg_model_fit_planes_f32's contract): a dict with n_planes; labels [M] int32 (plane
    p's rows carry p + 1, 0 is no plane); planes [P, 4] float64 (nx, ny, nz, d); centres [P, 3]; counts [P]; rmse [P]; and the
    diagnostics best_trial / best_cost / best_count [P] of every round's winning MSAC trial.  max_angle is in RADIANS.  samples,
    int32 [max_planes, n_trials, 3], replaces the sampler with the caller's 1-BASED rows.  The cloud is prepared for this call only:
    keep a Model for repeated calls."""
    t, rv, ang, P, B, mi, sd = planes_args(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed)
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    smp = _planes_samples(samples, P, B)
    return _planes_call(lambda *o: check(lib().pcreg_point_fit_planes_f32(m.ctypes.data, M, max(M, 1), t, rv.ctypes.data if rv is not None else None,
                                                                          ang, P, B, mi, sd, smp.ctypes.data if smp is not None else None, *o)), M, P)


def fit_spheres_args(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed):
    """The sphere extraction's parameters as the C tiers take them (pcreg_model_fit_spheres_f32's rules): max_distance as a float32
    whose fp32 square is a normal number, the radius bounds as float32 with 0 <= min_radius <= max_radius (max_radius may be inf),
    and the ranges of the counts."""
    t = np.float32(max_distance)
    tiny = np.finfo(np.float32).tiny
    with np.errstate(over="ignore", under="ignore"):
        t2 = t * t
    if not (np.isfinite(t) and t >= tiny and np.isfinite(t2) and t2 >= tiny):
        raise ValueError(f"max_distance must be a finite number > 0 whose float32 square is a normal number, got {max_distance}")
    with np.errstate(over="ignore"):
        r0, r1 = np.float32(min_radius), np.float32(max_radius)
    if not (r0 >= 0 and r0 <= r1):
        raise ValueError(f"the radius bounds must satisfy 0 <= min_radius <= max_radius, got {min_radius}, {max_radius}")
    P, B, mi = int(max_spheres), int(n_trials), int(min_inliers)
    if not 1 <= P <= 64:
        raise ValueError(f"max_spheres must lie in 1 .. 64, got {P}")
    if not 1 <= B <= 1 << 20:
        raise ValueError(f"n_trials must lie in 1 .. 2^20, got {B}")
    if mi < 4:
        raise ValueError(f"min_inliers must be at least 4, got {mi}")
    return float(t), float(r0), float(r1), P, B, mi, int(seed) & 0xFFFFFFFFFFFFFFFF


def _fit_spheres_samples(samples, P, B):
    if samples is None:
        return None
    smp = np.ascontiguousarray(np.asarray(samples, np.int32))
    if smp.shape != (P, B, 4):
        raise ValueError(f"samples must be [max_spheres, n_trials, 4] = {(P, B, 4)}, got {smp.shape}")
    return smp


def _fit_spheres_call(call, M: int, P: int) -> dict:
    labels = np.zeros(max(M, 1), dtype=np.int32)
    spheres = np.zeros((P, 4), dtype=np.float64)
    counts = np.zeros(P, dtype=np.int32)
    rmse = np.zeros(P, dtype=np.float64)
    used = np.zeros(P, dtype=np.int32)
    bt = np.zeros(P, dtype=np.int32)
    bc = np.zeros(P, dtype=np.int64)
    bn = np.zeros(P, dtype=np.int32)
    n = C.c_int32(0)
    call(labels.ctypes.data, spheres.ctypes.data, counts.ctypes.data, rmse.ctypes.data, used.ctypes.data, C.byref(n), bt.ctypes.data,
         bc.ctypes.data, bn.ctypes.data)
    return dict(n_spheres=int(n.value), labels=labels[:M], spheres=spheres, counts=counts, rmse=rmse, refit_used=used, best_trial=bt,
                best_cost=bc, best_count=bn)


def point_fit_spheres(pts, max_distance, min_radius: float = 0.0, max_radius: float = math.inf, max_spheres: int = 1,
                      n_trials: int = 1000, min_inliers: int = 4, seed: int = 0, samples=None) -> dict:
    """pcfitsphere(pts, maxDistance) and the fit / remove / fit-again loop, up to max_spheres times in one call, in this library's
    rule (pcreg_model_fit_spheres_f32's contract): a dict with n_spheres; labels [M] int32 (sphere p's rows carry p + 1, 0 is no
    sphere); spheres [P, 4] float64 (cx, cy, cz, R); counts [P]; rmse [P]; refit_used [P] (0: the round kept its winning trial's own
    sphere); and the diagnostics best_trial / best_cost / best_count [P] of every round's winning MSAC trial.  Only trial spheres
    with min_radius <= R <= max_radius count.  samples, int32 [max_spheres, n_trials, 4], replaces the sampler with the caller's
    1-BASED rows.  The cloud is prepared for this call only: keep a Model for repeated calls."""
    t, r0, r1, P, B, mi, sd = fit_spheres_args(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed)
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    smp = _fit_spheres_samples(samples, P, B)
    return _fit_spheres_call(lambda *o: check(lib().pcreg_point_fit_spheres_f32(m.ctypes.data, M, max(M, 1), t, r0, r1, P, B, mi, sd,
                                                                                smp.ctypes.data if smp is not None else None, *o)), M, P)


def fit_cylinders_args(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers, seed):
    """The cylinder extraction's parameters as the C tiers take them (pcreg_model_fit_cylinders_f32's rules): fit_spheres_args' for
    the distance, the radius bounds and the counts, planes_args' for ref_vec (three contiguous float64 or None) and max_angle."""
    t, r0, r1, P, B, mi, sd = fit_spheres_args(max_distance, min_radius, max_radius, 1, n_trials, min_inliers, seed)
    _, rv, ang, _, _, _, _ = planes_args(max_distance, ref_vec, max_angle, 1, 1, 3, 0)
    P = int(max_cylinders)
    if not 1 <= P <= 64:
        raise ValueError(f"max_cylinders must lie in 1 .. 64, got {P}")
    return t, r0, r1, rv, ang, P, B, mi, sd


def _fit_cylinders_normals(M: int, normals, k_normals):
    """-> (normals [M, 3] float32 column-major or None, k_normals): given normals are used as they are"""
    if normals is not None:
        nrm = _fcol(normals, np.float32)
        if nrm.ndim != 2 or nrm.shape != (M, 3):
            raise ValueError(f"normals are [M, 3] with M = {M} rows, got {nrm.shape}")
        return nrm, 3
    kn = int(k_normals)
    if not 3 <= kn <= KNN_MAX_K:
        raise ValueError(f"k_normals must lie in [3, {KNN_MAX_K}], got {kn}")
    return None, kn


def _fit_cylinders_samples(samples, P, B):
    if samples is None:
        return None
    smp = np.ascontiguousarray(np.asarray(samples, np.int32))
    if smp.shape != (P, B, 2):
        raise ValueError(f"samples must be [max_cylinders, n_trials, 2] = {(P, B, 2)}, got {smp.shape}")
    return smp


def _fit_cylinders_call(call, M: int, P: int) -> dict:
    labels = np.zeros(max(M, 1), dtype=np.int32)
    cyl = np.zeros((P, 7), dtype=np.float64)
    ext = np.zeros((P, 2), dtype=np.float64)
    counts = np.zeros(P, dtype=np.int32)
    rmse = np.zeros(P, dtype=np.float64)
    used = np.zeros(P, dtype=np.int32)
    bt = np.zeros(P, dtype=np.int32)
    bc = np.zeros(P, dtype=np.int64)
    bn = np.zeros(P, dtype=np.int32)
    n = C.c_int32(0)
    call(labels.ctypes.data, cyl.ctypes.data, ext.ctypes.data, counts.ctypes.data, rmse.ctypes.data, used.ctypes.data, C.byref(n),
         bt.ctypes.data, bc.ctypes.data, bn.ctypes.data)
    return dict(n_cylinders=int(n.value), labels=labels[:M], cylinders=cyl, extents=ext, counts=counts, rmse=rmse, refit_used=used,
                best_trial=bt, best_cost=bc, best_count=bn)


def point_fit_cylinders(pts, max_distance, min_radius: float = 0.0, max_radius: float = math.inf, ref_vec=None, max_angle=math.pi / 2,
                        normals=None, k_normals: int = 12, max_cylinders: int = 1, n_trials: int = 1000, min_inliers: int = 4,
                        seed: int = 0, samples=None) -> dict:
    """pcfitcylinder(pts, maxDistance[, referenceVector, maxAngularDistance]) and the fit / remove / fit-again loop, up to
    max_cylinders times in one call, in this library's rule (pcreg_model_fit_cylinders_f32's contract): a dict with n_cylinders;
    labels [M] int32 (cylinder p's rows carry p + 1, 0 is no cylinder); cylinders [P, 7] float64 (cx, cy, cz, wx, wy, wz, R: a point
    of the axis, its unit direction, the radius); extents [P, 2] (h_lo, h_hi: the axis runs from c + h_lo w to c + h_hi w); counts
    [P]; rmse [P]; refit_used [P] (0: the round kept its winning trial's own cylinder); and the diagnostics best_trial / best_cost /
    best_count [P].  normals: [M, 3] float32 by row, used as given (their sign does not matter); None: computed in the call from
    the k_normals nearest rows.  ref_vec / max_angle (radians) bound the axis.  samples, int32 [max_cylinders, n_trials, 2],
    replaces the sampler with the caller's 1-BASED rows.  The cloud is prepared for this call only: keep a Model for repeated calls."""
    t, r0, r1, rv, ang, P, B, mi, sd = fit_cylinders_args(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials,
                                                          min_inliers, seed)
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    nrm, kn = _fit_cylinders_normals(M, normals, k_normals)
    smp = _fit_cylinders_samples(samples, P, B)
    return _fit_cylinders_call(lambda *o: check(lib().pcreg_point_fit_cylinders_f32(
        m.ctypes.data, M, max(M, 1), t, r0, r1, rv.ctypes.data if rv is not None else None, ang, nrm.ctypes.data if nrm is not None and M else None,
        max(M, 1), kn, P, B, mi, sd, smp.ctypes.data if smp is not None else None, *o)), M, P)


def _denoise_args(k, threshold):
    k, threshold = int(k), float(threshold)
    if not 1 <= k <= KNN_MAX_K - 1:
        raise ValueError(f"k (NumNeighbors) must lie in [1, {KNN_MAX_K - 1}], got {k}")
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise ValueError(f"threshold must be a finite number >= 0, got {threshold}")
    return k, threshold


def _denoise_call(call, M: int) -> dict:
    md = np.zeros(max(M, 1), dtype=np.float64)
    inl = np.zeros(max(M, 1), dtype=np.int32)
    n = C.c_int32(0)
    stats = np.zeros(4, dtype=np.float64)
    call(md.ctypes.data, inl.ctypes.data, C.byref(n), stats.ctypes.data)
    return dict(inliers=inl[:n.value].copy(), mean_dist=md[:M], thr=float(stats[0]), mean=float(stats[1]), std=float(stats[2]),
                n_finite=int(stats[3]))


def point_denoise(pts, k: int = 4, threshold: float = 1.0) -> dict:
    """pcdenoise(pts, 'NumNeighbors', k, 'Threshold', threshold) (pcreg_model_denoise_f32's contract): a dict with mean_dist [M]
    float64, the mean distance of every row to its k nearest other rows (1 <= k <= 31; NaN for a non-finite row and where fewer
    than two finite rows exist); mean, std and n_finite of the finite ones; thr = mean + threshold * std; inliers, the 0-based
    rows with mean_dist <= thr, ascending int32 (pts[inliers] is the denoised cloud).  The cloud is prepared for this call only:
    keep a Model for repeated calls."""
    k, threshold = _denoise_args(k, threshold)
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    return _denoise_call(lambda md, inl, n, st: check(lib().pcreg_point_denoise_f32(m.ctypes.data, M, max(M, 1), k, threshold, md, inl, n, st)), M)


FPS_MAX_ROWS = 1 << 21      # PCREG_FPS_MAX_ROWS (include/pcreg.h)


def _fps_args(M: int, K, start, stop_d2):
    K, start, stop_d2 = int(K), int(start), float(stop_d2)
    if K < 0:
        raise ValueError(f"K must be >= 0, got {K}")
    if M > FPS_MAX_ROWS:
        raise ValueError(f"farthest point sampling serves at most {FPS_MAX_ROWS} rows, got {M}")
    if M > 0 and not -1 <= start < M:
        raise ValueError(f"start must be -1 or a 0-based row below {M}, got {start}")
    if not stop_d2 >= 0.0:
        raise ValueError(f"stop_d2 must be >= 0 and not NaN, got {stop_d2}")
    return K, start, stop_d2


def _fps_call(call, M: int, K: int) -> dict:
    idx = np.zeros(max(K, 1), dtype=np.int32)
    dist = np.zeros(max(K, 1), dtype=np.float32)
    n = C.c_int32(0)
    cover = C.c_float(0.0)
    md = np.zeros(max(M, 1), dtype=np.float32)
    lab = np.zeros(max(M, 1), dtype=np.int32)
    call(idx.ctypes.data, dist.ctypes.data, C.byref(n), C.byref(cover), md.ctypes.data, lab.ctypes.data)
    return dict(idx=idx[:n.value].copy(), dist=dist[:n.value].copy(), n_out=int(n.value), cover_d2=np.float32(cover.value), min_dist=md[:M],
                label=lab[:M])


def point_farthest_points(pts, K: int, start: int = -1, stop_d2: float = 0.0) -> dict:
    """Farthest point sampling of pts (pcreg_model_fps_f32's contract): at most K rows, each the finite row farthest from all rows
    chosen before it, starting at the 0-based row `start` (-1: the lowest finite row) and stopping early once every finite row is
    within stop_d2 (a SQUARED distance) of a sample.  A dict of numpy arrays: idx [n_out] int32 0-based rows in selection order;
    dist [n_out] float32, the squared distance of each sample to the ones before it (dist[0] = inf, non-increasing after);
    n_out; cover_d2 (float32), the largest squared distance of a finite row to its nearest sample; min_dist [M] float32 and
    label [M] int32, per row that distance and the 1-based position in idx of the nearest sample (NaN / 0 for a non-finite row).
    The cloud is prepared for this call only: keep a Model for repeated calls."""
    m = _fcol(pts, np.float32)
    if m.ndim != 2 or m.shape[1] != 3:
        raise ValueError("pts must be M x 3")
    M = m.shape[0]
    K, start, stop_d2 = _fps_args(M, K, start, stop_d2)
    return _fps_call(lambda *o: check(lib().pcreg_point_fps_f32(m.ctypes.data, M, max(M, 1), K, start, stop_d2, *o)), M, K)


def unique_rows(A):
    """[C, ia] = unique(A, 'rows') for an n x 3 float64 array: (C [u, 3], ia [u] int32, 0-based).  Rows in lexicographic order by
    column 1, 2, 3 as numbers (-0 == +0); the first occurrence represents its run and C = A[ia] carries its bits.  A NaN anywhere
    is refused (PCREG_E_ARG)."""
    a = _pts3(A, "A")
    n = a.shape[0]
    ia = np.zeros(max(n, 1), dtype=np.int32)
    nu = C.c_int(0)
    check(lib().pcreg_unique_rows3(_ptr(a, C.c_double), C.c_int(n), C.c_int(max(n, 1)), _ptr(ia, C.c_int32), C.byref(nu)))
    ia = ia[:nu.value] - 1
    return np.ascontiguousarray(a[ia]), ia


def aggregate_matches(pts1, pts2):
    """completeExperiment.m:440-443 on stacked putative matches (n x 3 float64 each): unique over pts1, pts2 taken along, unique
    over that pts2, pts1 taken along -> (pts1u [u, 3], pts2u [u, 3], ia [u] int32, 0-based rows of the input), sorted by pts2u."""
    p1, p2 = _pts3(pts1, "pts1"), _pts3(pts2, "pts2")
    n = p1.shape[0]
    if p2.shape[0] != n:
        raise ValueError("pts1 and pts2 must have the same number of rows")
    ld = max(n, 1)
    o1 = np.zeros((ld, 3), dtype=np.float64, order="F"); o2 = np.zeros((ld, 3), dtype=np.float64, order="F")
    ia = np.zeros(ld, dtype=np.int32)
    no = C.c_int(0)
    check(lib().pcreg_aggregate_matches(_ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(n), C.c_int(ld), _ptr(o1, C.c_double),
                                        _ptr(o2, C.c_double), C.c_int(ld), _ptr(ia, C.c_int32), C.byref(no)))
    u = no.value
    return np.ascontiguousarray(o1[:u]), np.ascontiguousarray(o2[:u]), ia[:u] - 1


def pcdownsample(pts, step: float):
    """pcdownsample(pc, 'gridAverage', step) for an n x 3 float32 cloud (pcreg_downsample_grid_f32's contract): (out [n_out, 3]
    float32, count [n_out] int32, label [n] int32).  A voxel is a distinct cell floor((x - lo) / step) of the grid that starts at the
    minimum of the finite rows, taken in double; the output rows are the voxels in ascending (c0, c1, c2) order, each the mean of
    its rows, summed in double in ascending row order and rounded once; count their number of rows; label the 0-based output row
    of every input row, -1 for a row with a non-finite coordinate (it belongs to no voxel).  A cloud that spans 2^21 or more
    cells along an axis is refused (PCREG_E_ARG)."""
    step = float(step)
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"step must be a finite number > 0, got {step}")
    p = _fcol(pts, np.float32)
    if p.shape[1] != 3:
        raise ValueError("pts must be N x 3")
    n = p.shape[0]
    ld = max(n, 1)
    out = np.zeros((ld, 3), dtype=np.float32, order="F")
    count = np.zeros(ld, dtype=np.int32)
    label = np.zeros(ld, dtype=np.int32)
    no = C.c_int(0)
    check(lib().pcreg_downsample_grid_f32(p.ctypes.data, n, ld, step, out.ctypes.data, ld, count.ctypes.data, label.ctypes.data, C.byref(no)))
    u = no.value
    return np.ascontiguousarray(out[:u]), count[:u].copy(), label[:n] - 1


def _transforms16(T) -> np.ndarray:
    """[B, 16] float64, each transform column-major: from a [B, 4, 4] array, one 4 x 4 matrix, or a sequence of 4 x 4 matrices
    in which None (or an empty array: MATLAB's []) stands for the empty transform, sixteen zeros"""
    if isinstance(T, np.ndarray) and T.ndim == 2:
        T = T[None]
    mats = [np.zeros((4, 4)) if t is None or np.size(t) == 0 else np.asarray(t, dtype=np.float64) for t in T]
    if any(m.shape != (4, 4) for m in mats):
        raise ValueError("every transform is a 4 x 4 matrix (or None: the empty transform)")
    return np.ascontiguousarray([m.ravel(order="F") for m in mats], dtype=np.float64).reshape(-1, 16)


def score_summary(n_close, sum_d2, Q: int) -> dict:
    """the callers' arithmetic on a scoring call's counts and sums: fitness = n_close / Q (0 without queries), rmse =
    sqrt(sum_d2 / n_close) (NaN where nothing is close)"""
    n_close, sum_d2 = np.asarray(n_close, dtype=np.int32), np.asarray(sum_d2, dtype=np.float64)
    fitness = n_close / float(Q) if Q > 0 else np.zeros(len(n_close))
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.where(n_close > 0, np.sqrt(sum_d2 / np.maximum(n_close, 1)), np.nan)
    return dict(n_close=n_close, sum_d2=sum_d2, fitness=fitness, rmse=rmse)


class _Trim:
    """The keep_ratio of a Model method: false for None (the untrimmed entry); otherwise the checked ratio, the two
    [B] outputs the trimmed entry fills (`args`, its last two arguments), and into(), which adds them to the method's dict."""

    def __init__(self, keep_ratio, B: int):
        self.ratio = None
        if keep_ratio is None:
            return
        self.ratio = float(keep_ratio)
        if not 0.0 < self.ratio <= 1.0:
            raise ValueError(f"keep_ratio must lie in (0, 1], got {self.ratio}")
        self.B = B
        self.n_within = np.zeros(max(B, 1), dtype=np.int32)
        self.d2_cut = np.full(max(B, 1), np.inf, dtype=np.float32)
        self.args = (self.n_within.ctypes.data, self.d2_cut.ctypes.data)

    def __bool__(self):
        return self.ratio is not None

    def into(self, res: dict) -> dict:
        if self:
            res.update(n_within=self.n_within[:self.B], d2_cut=self.d2_cut[:self.B])
        return res


class Model:
    """A model cloud uploaded and prepared ONCE (pcreg_model_create), matched against any number of surfaces: the host-tier
    handle a MATLAB caller keeps across the sphere loop of completeExperimentFast.m:131-149.  Use as a context manager or
    call close()."""

    def __init__(self, model):
        m = _fcol(model, np.float32)
        self.M = m.shape[0]
        self._h = C.c_void_p()
        check(lib().pcreg_model_create(_ptr(m, C.c_float), C.c_int(self.M), C.c_int(max(self.M, 1)), C.byref(self._h)))

    def match_points(self, query, thr_abs: float, max_ratio: float, unique: bool = True) -> np.ndarray:
        if not self._h.value:
            raise ValueError("the model handle is closed")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        pairs = np.zeros((max(Q, 1), 2), dtype=np.uint32)
        P = C.c_int(0)
        check(lib().pcreg_model_match_points_f32(self._h, _ptr(q, C.c_float), C.c_int(Q), C.c_int(max(Q, 1)), C.c_float(thr_abs),
                                                 C.c_float(max_ratio), C.c_int(int(unique)), _ptr(pairs, C.c_uint32), C.byref(P)))
        return pairs[:P.value].copy()

    def knn(self, query, k: int):
        """knnsearch(model, query, 'K', k) against the prepared model: (idx [Q,k] 0-based int32, -1 past M; dist [Q,k]
        squared float32, +inf past M), ordered by (distance, row) -- the bits of a brute-force fp32 search."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        k = _knn_k(k)
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        idx = np.zeros((max(Q, 1), k), dtype=np.int32)
        dist = np.zeros((max(Q, 1), k), dtype=np.float32)
        check(lib().pcreg_model_knn_f32(self._h, _ptr(q, C.c_float), C.c_int(Q), C.c_int(max(Q, 1)), C.c_int(k), _ptr(idx, C.c_int32),
                                        _ptr(dist, C.c_float)))
        return idx[:Q], dist[:Q]

    def rangesearch(self, query, r2: float):
        """rangesearch(model, query, r) against the prepared model with r2 = r^2: (seg_off [Q + 1] int64, idx [total] 0-based
        int32, dist [total] squared float32), query i's rows at seg_off[i] .. seg_off[i + 1], ordered by (distance, row) -- the
        bits of a brute-force fp32 search."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        return _range_call(lambda cap, so, i, d: check(lib().pcreg_model_range_f32(self._h, q.ctypes.data, Q, max(Q, 1), r2, cap, so.ctypes.data, i, d)), Q)

    def score_transforms(self, query, T, r2: float, rows: bool = False, keep_ratio=None):
        """How well B transforms put `query` (Q x 3) on the prepared model (pcreg_model_score_f32).  T: a [B, 4, 4] array or a
        sequence of 4 x 4 matrices used as quickTF uses them, None or an all-zero matrix being the empty transform (it scores
        nothing); r2 the squared radius -> dict(n_close [B] int32, the queries with a model row within r2 of their
        transformed place; sum_d2 [B] float64, the sum of those squared distances; fitness = n_close / Q; rmse =
        sqrt(sum_d2 / n_close), NaN where nothing is close), and with rows=True also idx [B, Q] int32 (0-based, -1 for none)
        and dist [B, Q] float32 (squared, +inf for none) -- the bits of a brute-force fp32 search.
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_model_score_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query, and everything above
        is about the kept pairs -- and the dict gains n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B]
        float32, the largest kept squared distance (+inf where nothing is kept).  idx / dist hold -1 / +inf at trimmed slots."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        n_close = np.zeros(max(B, 1), dtype=np.int32)
        sum_d2 = np.zeros(max(B, 1), dtype=np.float64)
        idx = np.zeros((B, Q), dtype=np.int32) if rows else None
        dist = np.zeros((B, Q), dtype=np.float32) if rows else None
        trim = _Trim(keep_ratio, B)
        if trim:
            check(lib().pcreg_model_score_trimmed_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2,
                                                      trim.ratio, n_close.ctypes.data, sum_d2.ctypes.data, idx.ctypes.data if rows and B * Q else None,
                                                      dist.ctypes.data if rows and B * Q else None, *trim.args))
        else:
            check(lib().pcreg_model_score_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2,
                                              n_close.ctypes.data, sum_d2.ctypes.data, idx.ctypes.data if rows and B * Q else None,
                                              dist.ctypes.data if rows and B * Q else None))
        res = trim.into(score_summary(n_close[:B], sum_d2[:B], Q))
        if rows:
            res.update(idx=idx, dist=dist)
        return res

    def refit_transforms(self, query, T, r2: float, steps: int = 1, keep_ratio=None):
        """B transforms refitted on their close pairs against the prepared model, `steps` times over (pcreg_model_refit_f32): per
        step, T_step = estimateTransform(model rows, moved points) over the points of `query` (Q x 3) with a model row within
        r2 of their transformed place, and T <- T * T_step.  T as score_transforms takes it -> dict(T [B, 4, 4] float64, the
        refitted transforms, used as quickTF uses them, a zero matrix where there is no fit; empty [B] bool; n_close, sum_d2,
        fitness, rmse as score_transforms gives them for the transform that went INTO the last step).
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_model_refit_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query, and everything above
        is about the kept pairs -- and the dict gains n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B]
        float32, the largest kept squared distance (+inf where nothing is kept).  Every step trims anew."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        out = np.zeros((max(B, 1), 16), dtype=np.float64)
        n_close = np.zeros(max(B, 1), dtype=np.int32)
        sum_d2 = np.zeros(max(B, 1), dtype=np.float64)
        empty = np.zeros(max(B, 1), dtype=np.int32)
        trim = _Trim(keep_ratio, B)
        if trim:
            check(lib().pcreg_model_refit_trimmed_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2,
                                                      trim.ratio, steps, out.ctypes.data, n_close.ctypes.data, sum_d2.ctypes.data, empty.ctypes.data,
                                                      *trim.args))
        else:
            check(lib().pcreg_model_refit_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2, steps,
                                              out.ctypes.data, n_close.ctypes.data, sum_d2.ctypes.data, empty.ctypes.data))
        res = trim.into(score_summary(n_close[:B], sum_d2[:B], Q))
        res.update(T=np.ascontiguousarray(out[:B].reshape(B, 4, 4).transpose(0, 2, 1)), empty=empty[:B] != 0)
        return res

    def refit_plane(self, query, T, r2: float, steps: int = 1, normals=None, k: int = 6, keep_ratio=None):
        """B transforms refitted by the linearised point-to-plane step against the prepared model, `steps` times over
        (pcreg_model_refit_plane_f32, whose contract this is): the pairs are refit_transforms', the residual of a pair is its
        distance from the plane through the model row, and T <- T * T_step.  normals: [M, 3] float32 by original row, as
        Model.normals returns them (a row with a non-finite component offers no plane; the sign is immaterial), or None to
        compute them once on the device from the k nearest rows (6 is MATLAB's pcnormals default).  -> refit_transforms' dict
        plus n_plane [B] int32, the pairs with a plane; sum_res2 [B] float64, the sum of their squared plane residuals;
        plane_rmse = sqrt(sum_res2 / n_plane), NaN where there is none -- all for the transform that went INTO the last step.
        empty is also set where fewer than six planes, or planes that leave a direction free, give no fit.
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_model_refit_plane_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query, and everything above
        is about the kept pairs -- and the dict gains n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B]
        float32, the largest kept squared distance (+inf where nothing is kept).  Every step trims anew."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        nrm = None
        if normals is not None:
            nrm = _fcol(normals, np.float32)
            if nrm.shape[0] != self.M:
                raise ValueError(f"normals are [M, 3] with M = {self.M} rows, got {nrm.shape[0]}")
        else:
            k, _ = _normals_args(k, None)
        out = np.zeros((max(B, 1), 16), dtype=np.float64)
        n_close, n_plane, empty = (np.zeros(max(B, 1), dtype=np.int32) for _ in range(3))
        sum_d2, sum_res2 = (np.zeros(max(B, 1), dtype=np.float64) for _ in range(2))
        trim = _Trim(keep_ratio, B)
        if trim:
            check(lib().pcreg_model_refit_plane_trimmed_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2,
                                                            trim.ratio, steps, nrm.ctypes.data if nrm is not None else None, max(self.M, 1), int(k),
                                                            out.ctypes.data, n_close.ctypes.data, sum_d2.ctypes.data, n_plane.ctypes.data,
                                                            sum_res2.ctypes.data, empty.ctypes.data, *trim.args))
        else:
            check(lib().pcreg_model_refit_plane_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2, steps,
                                                    nrm.ctypes.data if nrm is not None else None, max(self.M, 1), int(k), out.ctypes.data,
                                                    n_close.ctypes.data, sum_d2.ctypes.data, n_plane.ctypes.data, sum_res2.ctypes.data,
                                                    empty.ctypes.data))
        res = trim.into(score_summary(n_close[:B], sum_d2[:B], Q))
        with np.errstate(divide="ignore", invalid="ignore"):
            plane_rmse = np.where(n_plane[:B] > 0, np.sqrt(sum_res2[:B] / n_plane[:B]), np.nan)
        res.update(T=np.ascontiguousarray(out[:B].reshape(B, 4, 4).transpose(0, 2, 1)), empty=empty[:B] != 0, n_plane=n_plane[:B],
                   sum_res2=sum_res2[:B], plane_rmse=plane_rmse)
        return res

    def refit_gicp(self, query, T, r2: float, steps: int = 1, normals=None, query_normals=None, k: int = 6, epsilon: float = 1e-3,
                   keep_ratio=None):
        """B transforms refitted by the plane-to-plane (generalized ICP) step against the prepared model, `steps` times over
        (pcreg_model_refit_gicp_f32, whose contract this is): the pairs are refit_transforms', a pair is weighted by the inverse
        of the sum of the two sides' covariances, each I - (1 - epsilon) n n^T about its own normal, and T <- T * T_step.
        normals: [M, 3] float32 by original row, as Model.normals returns them; query_normals: [Q, 3] float32 by query, as
        Model(query).normals returns them (a pair with a non-finite component on either side is dropped; the signs are
        immaterial); either None: computed once on the device from the k nearest rows of its own cloud.  epsilon in (0, 1].
        -> refit_transforms' dict plus n_pairs [B] int32, the plane-to-plane pairs; sum_res2 [B] float64, the sum of their
        e^T W e; pair_rmse = sqrt(sum_res2 / n_pairs), NaN where there is none -- all for the transform that went INTO the last
        step.  empty is also set where fewer than six pairs, or pairs that leave a direction free, give no fit.
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_model_refit_gicp_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query, and everything above
        is about the kept pairs -- and the dict gains n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B]
        float32, the largest kept squared distance (+inf where nothing is kept).  Every step trims anew."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        steps, epsilon = int(steps), float(epsilon)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        if not 0.0 < epsilon <= 1.0:
            raise ValueError(f"epsilon must lie in (0, 1], got {epsilon}")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        nrm = nq = None
        if normals is not None:
            nrm = _fcol(normals, np.float32)
            if nrm.shape[0] != self.M:
                raise ValueError(f"normals are [M, 3] with M = {self.M} rows, got {nrm.shape[0]}")
        if query_normals is not None:
            nq = _fcol(query_normals, np.float32)
            if nq.shape[0] != Q:
                raise ValueError(f"query normals are [Q, 3] with Q = {Q} rows, got {nq.shape[0]}")
        if nrm is None or nq is None:
            k, _ = _normals_args(k, None)
        out = np.zeros((max(B, 1), 16), dtype=np.float64)
        n_close, n_pairs, empty = (np.zeros(max(B, 1), dtype=np.int32) for _ in range(3))
        sum_d2, sum_res2 = (np.zeros(max(B, 1), dtype=np.float64) for _ in range(2))
        trim = _Trim(keep_ratio, B)
        if trim:
            check(lib().pcreg_model_refit_gicp_trimmed_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2,
                                                           trim.ratio, steps, nrm.ctypes.data if nrm is not None else None, max(self.M, 1),
                                                           nq.ctypes.data if nq is not None else None, max(Q, 1), int(k), epsilon, out.ctypes.data,
                                                           n_close.ctypes.data, sum_d2.ctypes.data, n_pairs.ctypes.data, sum_res2.ctypes.data,
                                                           empty.ctypes.data, *trim.args))
        else:
            check(lib().pcreg_model_refit_gicp_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, r2, steps,
                                                   nrm.ctypes.data if nrm is not None else None, max(self.M, 1),
                                                   nq.ctypes.data if nq is not None else None, max(Q, 1), int(k), epsilon, out.ctypes.data,
                                                   n_close.ctypes.data, sum_d2.ctypes.data, n_pairs.ctypes.data, sum_res2.ctypes.data,
                                                   empty.ctypes.data))
        res = trim.into(score_summary(n_close[:B], sum_d2[:B], Q))
        with np.errstate(divide="ignore", invalid="ignore"):
            pair_rmse = np.where(n_pairs[:B] > 0, np.sqrt(sum_res2[:B] / n_pairs[:B]), np.nan)
        res.update(T=np.ascontiguousarray(out[:B].reshape(B, 4, 4).transpose(0, 2, 1)), empty=empty[:B] != 0, n_pairs=n_pairs[:B],
                   sum_res2=sum_res2[:B], pair_rmse=pair_rmse)
        return res

    def refit_cpd(self, query, T, sigma2=0.0, outlier: float = 0.1, steps: int = 1):
        """B transforms refitted by the coherent-point-drift step (rigid CPD) against the prepared model, `steps` times over
        (pcreg_model_refit_cpd_f32, whose contract this is): every moved query is paired softly with EVERY live model row by
        exp(-d2 / (2 sigma2)) against a uniform outlier term of weight `outlier` in [0, 1), the weighted rigid fit with the
        determinant correction follows, T <- T * T_step, and the variance is annealed by its own closed form.  No radius, no
        normals, no voxel size.  The cost is B * Q * M pairs a step: for downsampled clouds.
        sigma2: a number or [B] float64, the variance each candidate starts from; 0 (the default) asks for the initial value,
        the mean squared distance over all pairs divided by 3; negative or NaN makes the candidate empty.
        -> dict(T [B, 4, 4] as quickTF uses them, a ZERO matrix where empty; empty [B] bool; sigma2 [B] float64, the variance
        AFTER the last step (feed it to a later call), 0 where empty; and for the transform that went INTO the last step: Np [B]
        float64, the sum of the posterior weights; sum_res2 [B] float64, the weighted squared residual; sum_d2 [B] float64, the
        sum of the squared nearest-row distances (score_transforms' bits at r2 = +inf); n_live [B] int32, the queries whose moved
        point is finite)."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        steps, outlier = int(steps), float(outlier)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        if not 0.0 <= outlier < 1.0:
            raise ValueError(f"outlier must lie in [0, 1), got {outlier}")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        sig = np.asarray(sigma2, dtype=np.float64).reshape(-1)
        if sig.size == 1:
            sig = np.full(max(B, 1), sig[0])
        elif sig.size != B:
            raise ValueError(f"sigma2 is a number or one per transform ({B}), got {sig.size}")
        sig = np.ascontiguousarray(sig) if B else np.zeros(1)
        out = np.zeros((max(B, 1), 16), dtype=np.float64)
        sig_out, Np, sum_res2, sum_d2 = (np.zeros(max(B, 1), dtype=np.float64) for _ in range(4))
        n_live, empty = (np.zeros(max(B, 1), dtype=np.int32) for _ in range(2))
        check(lib().pcreg_model_refit_cpd_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, sig.ctypes.data,
                                              outlier, steps, out.ctypes.data, sig_out.ctypes.data, Np.ctypes.data, sum_res2.ctypes.data,
                                              sum_d2.ctypes.data, n_live.ctypes.data, empty.ctypes.data))
        return dict(T=np.ascontiguousarray(out[:B].reshape(B, 4, 4).transpose(0, 2, 1)), empty=empty[:B] != 0, sigma2=sig_out[:B], Np=Np[:B],
                    sum_res2=sum_res2[:B], sum_d2=sum_d2[:B], n_live=n_live[:B])

    def cluster(self, r2: float):
        """clusterPoints(model, r) on the prepared model's own rows with r2 = r^2: (label [M] int32, cl_off [C + 1] int32,
        members [M] int32), 0-based -- cluster_points' contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2 = _range_r2(r2)
        return _cluster_call(lambda lab, nc, off, mem: check(lib().pcreg_model_cluster_f32(self._h, r2, lab, nc, off, mem)), self.M)

    def dbscan(self, r2: float, minpts: int):
        """DBSCAN of the prepared model's own rows with r2 = epsilon^2: (label [M] int32, core [M] bool, cl_off [C + 1] int32,
        members int32), 0-based, noise -1 -- dbscan_points' contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2, minpts = _range_r2(r2), _dbscan_minpts(minpts)
        return _dbscan_call(lambda lab, nc, core, off, mem: check(lib().pcreg_model_dbscan_f32(self._h, r2, minpts, lab, nc, core, None, off, mem)),
                            self.M)

    def normals(self, k: int, viewpoint=None, variation: bool = False):
        """The surface normal of every row of the prepared model from its k nearest rows: normals [M, 3] float32, and with
        variation=True also the surface variation [M] float32 -- point_normals' contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        k, vp = _normals_args(k, viewpoint)
        return _normals_call(lambda v, n, ldn, va: check(lib().pcreg_model_normals_f32(self._h, k, v, n, ldn, va)), self.M, vp, variation)

    def fpfh(self, k: int, normals=None, k_normals=None, viewpoint=None, spfh: bool = False):
        """The FPFH descriptor of every row of the prepared model from its k nearest rows and a normal per row: [M, 33] float64,
        and with spfh=True also the SPFH counts [M, 33] uint8 -- point_fpfh's contract.  normals: what Model.normals returns
        (oriented: the sign matters), or None to compute them in the call with k_normals (default k) and the viewpoint."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        k, nrm, kn, vp = _fpfh_args(self.M, k, normals, k_normals, viewpoint)
        return _fpfh_call(lambda n, ldn, v, o, ldf, c: check(lib().pcreg_model_fpfh_f32(self._h, k, n, ldn, kn, v, o, ldf, c)), self.M, nrm, vp, spfh)

    def fpfh_radius(self, radius, normals=None, max_neighbors: int = 0, k_normals: int = 6, viewpoint=None, counts: bool = False,
                    n_neighbors: bool = False):
        """The FPFH descriptor of every row of the prepared model from the rows within the radius (at most the max_neighbors
        nearest of them; 0: all) and a normal per row: [M, 33] float64, with counts=True also the SPFH counts [M, 33] uint32 and
        with n_neighbors=True the neighbours counted per row [M] int32 -- point_fpfh_radius's contract.  normals: what
        Model.normals returns (oriented: the sign matters), or None to compute them in the call with k_normals and the viewpoint."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        r2, n, nrm, kn, vp = _fpfh_radius_args(self.M, radius, max_neighbors, normals, k_normals, viewpoint)
        return _fpfh_radius_call(lambda a, ldn, v, o, ldf, c, nn: check(lib().pcreg_model_fpfh_radius_f32(self._h, r2, n, a, ldn, kn, v, o, ldf, c, nn)),
                                 self.M, nrm, vp, counts, n_neighbors)

    def iss_keypoints(self, salient_radius, nonmax_radius, gamma21: float = 0.975, gamma32: float = 0.975, min_neighbors: int = 5) -> dict:
        """The ISS keypoints of the prepared model's own rows, with the neighbour count, the eigenvalues and the saliency of every
        row -- point_iss's dict and contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        a = iss_args(salient_radius, nonmax_radius, gamma21, gamma32, min_neighbors)
        return _iss_call(lambda nn, e, s, kp, n: check(lib().pcreg_model_iss_f32(self._h, *a, nn, e, s, kp, n)), self.M)

    def fit_planes(self, max_distance, ref_vec=None, max_angle=math.pi / 2, max_planes: int = 1, n_trials: int = 1000,
                   min_inliers: int = 3, seed: int = 0, samples=None) -> dict:
        """MSAC plane fitting and extraction over the prepared model's own rows -- point_fit_planes's dict and contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        t, rv, ang, P, B, mi, sd = planes_args(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed)
        smp = _planes_samples(samples, P, B)
        return _planes_call(lambda *o: check(lib().pcreg_model_fit_planes_f32(self._h, t, rv.ctypes.data if rv is not None else None, ang, P, B, mi,
                                                                              sd, smp.ctypes.data if smp is not None else None, *o)), self.M, P)

    def fit_spheres(self, max_distance, min_radius: float = 0.0, max_radius: float = math.inf, max_spheres: int = 1,
                    n_trials: int = 1000, min_inliers: int = 4, seed: int = 0, samples=None) -> dict:
        """MSAC sphere fitting and extraction over the prepared model's own rows -- point_fit_spheres's dict and contract."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        t, r0, r1, P, B, mi, sd = fit_spheres_args(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed)
        smp = _fit_spheres_samples(samples, P, B)
        return _fit_spheres_call(lambda *o: check(lib().pcreg_model_fit_spheres_f32(self._h, t, r0, r1, P, B, mi, sd,
                                                                                    smp.ctypes.data if smp is not None else None, *o)), self.M, P)

    def fit_cylinders(self, max_distance, min_radius: float = 0.0, max_radius: float = math.inf, ref_vec=None, max_angle=math.pi / 2,
                      normals=None, k_normals: int = 12, max_cylinders: int = 1, n_trials: int = 1000, min_inliers: int = 4,
                      seed: int = 0, samples=None) -> dict:
        """MSAC cylinder fitting and extraction over the prepared model's own rows -- point_fit_cylinders's dict and contract.
        normals: what Model.normals returns, or None to compute them in the call with k_normals."""
        if not self._h.value:
            raise ValueError("the model handle is closed")
        t, r0, r1, rv, ang, P, B, mi, sd = fit_cylinders_args(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders,
                                                              n_trials, min_inliers, seed)
        M = self.M
        nrm, kn = _fit_cylinders_normals(M, normals, k_normals)
        smp = _fit_cylinders_samples(samples, P, B)
        return _fit_cylinders_call(lambda *o: check(lib().pcreg_model_fit_cylinders_f32(
            self._h, t, r0, r1, rv.ctypes.data if rv is not None else None, ang, nrm.ctypes.data if nrm is not None and M else None, max(M, 1),
            kn, P, B, mi, sd, smp.ctypes.data if smp is not None else None, *o)), M, P)

    def denoise(self, k: int = 4, threshold: float = 1.0) -> dict:
        """pcdenoise on the prepared model's own rows: the mean distance of every row to its k nearest other rows, the threshold
        mean + threshold * std, and the rows at or below it -- point_denoise's dict."""
        if self._h is None:
            raise RuntimeError("model handle closed")
        k, threshold = _denoise_args(k, threshold)
        return _denoise_call(lambda md, inl, n, st: check(lib().pcreg_model_denoise_f32(self._h, k, threshold, md, inl, n, st)), self.M)

    def farthest_points(self, K: int, start: int = -1, stop_d2: float = 0.0) -> dict:
        """Farthest point sampling of the prepared model's own rows: at most K well-spread rows and the covering radius with every
        one of them -- point_farthest_points's dict and contract."""
        if self._h is None:
            raise RuntimeError("model handle closed")
        K, start, stop_d2 = _fps_args(self.M, K, start, stop_d2)
        return _fps_call(lambda *o: check(lib().pcreg_model_fps_f32(self._h, K, start, stop_d2, *o)), self.M, K)

    def close(self):
        if self._h.value:
            lib().pcreg_model_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NdtModel:
    """A cloud summarised ONCE as one Gaussian per occupied voxel (pcreg_ndt_create, whose contract this is): the table that
    NDT steps refine candidate transforms against, without a nearest-row search.  points: n x 3 float32; step: the voxel size;
    min_points: the rows a voxel needs to hold a Gaussian.  A step, not a registration policy: no convergence test, no line
    search, no multi-resolution schedule.  Use as a context manager or call close()."""

    def __init__(self, points, step: float, min_points: int = 6):
        step, min_points = float(step), int(min_points)
        if not (math.isfinite(step) and step > 0.0):
            raise ValueError(f"step must be a finite number > 0, got {step}")
        if min_points < 3:
            raise ValueError(f"min_points must be at least 3, got {min_points}")
        p = _fcol(points, np.float32)
        if p.shape[1] != 3:
            raise ValueError("points must be N x 3")
        n = p.shape[0]
        self.step, self.min_points = step, min_points
        self._h = C.c_void_p()
        check(lib().pcreg_ndt_create(p.ctypes.data if n else None, n, max(n, 1), step, min_points, C.byref(self._h)))
        nv, ng = C.c_int(), C.c_int()
        check(lib().pcreg_ndt_size(self._h, C.byref(nv), C.byref(ng)))
        self.n_voxels, self.n_gaussians = nv.value, ng.value

    def gaussians(self) -> dict:
        """-> cells [G, 3] int32, counts [G] int32, means [G, 3] float64, C [G, 6] float64 (xx xy xz yy yz zz of the floored inverse
        covariance), lo [3] and origin [3] float32; the Gaussians ascend by cell"""
        if not self._h.value:
            raise ValueError("the NDT handle is closed")
        G = self.n_gaussians
        cells, counts = np.zeros((G, 3), np.int32), np.zeros(G, np.int32)
        means, Cm = np.zeros((G, 3), np.float64), np.zeros((G, 6), np.float64)
        lo, origin = np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(lib().pcreg_ndt_get(self._h, cells.ctypes.data, counts.ctypes.data, means.ctypes.data, Cm.ctypes.data, lo.ctypes.data, origin.ctypes.data))
        return dict(cells=cells, counts=counts, means=means, C=Cm, lo=lo, origin=origin)

    def refit(self, query, T, neighbors: int = 1, outlier_ratio: float = 0.55, steps: int = 1) -> dict:
        """B transforms refined by `steps` NDT steps (pcreg_ndt_refit_f32): -> T [B, 4, 4] as quickTF uses them, empty [B] bool,
        n_pairs [B] int32 and sum_e [B] float64 (the pairs and the sum of their likelihood weights) for the transform that went
        INTO the last step"""
        if not self._h.value:
            raise ValueError("the NDT handle is closed")
        neighbors, outlier_ratio, steps = int(neighbors), float(outlier_ratio), int(steps)
        if neighbors not in (1, 7):
            raise ValueError(f"neighbors must be 1 or 7, got {neighbors}")
        if not 0.0 <= outlier_ratio < 1.0:
            raise ValueError(f"outlier_ratio must lie in [0, 1), got {outlier_ratio}")
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        q = _fcol(query, np.float32)
        Q = q.shape[0]
        T16 = _transforms16(T)
        B = T16.shape[0]
        out = np.zeros((max(B, 1), 16), dtype=np.float64)
        n_pairs, empty = (np.zeros(max(B, 1), dtype=np.int32) for _ in range(2))
        sum_e = np.zeros(max(B, 1), dtype=np.float64)
        check(lib().pcreg_ndt_refit_f32(self._h, q.ctypes.data if Q else None, Q, max(Q, 1), T16.ctypes.data if B else None, B, neighbors,
                                        outlier_ratio, steps, out.ctypes.data, n_pairs.ctypes.data, sum_e.ctypes.data, empty.ctypes.data))
        return dict(T=np.ascontiguousarray(out[:B].reshape(B, 4, 4).transpose(0, 2, 1)), empty=empty[:B] != 0, n_pairs=n_pairs[:B], sum_e=sum_e[:B])

    def close(self):
        if self._h.value:
            lib().pcreg_ndt_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_points(query, model, thr_abs: float, max_ratio: float, unique: bool = True) -> np.ndarray:
    """matchFeatures' filter chain on raw 3-D fp32 points -> P x 2 uint32 (1-based)."""
    q, m = _fcol(query, np.float32), _fcol(model, np.float32)
    Q, M = q.shape[0], m.shape[0]
    pairs = np.zeros((max(Q, 1), 2), dtype=np.uint32)
    P = C.c_int(0)
    check(lib().pcreg_match_points_f32(_ptr(q, C.c_float), C.c_int(Q), C.c_int(Q), _ptr(m, C.c_float), C.c_int(M),
                                       C.c_int(M), C.c_float(thr_abs), C.c_float(max_ratio), C.c_int(int(unique)),
                                       _ptr(pairs, C.c_uint32), C.byref(P)))
    return pairs[:P.value].copy()


# --------------------------------------------------------------------- AlignPoints_KNN
def AlignPoints_KNN(pts, *varargin):
    """[pts_aligned, coeff_unambig, c] = AlignPoints_KNN(pts[, C1, C2])  (AlignPoints_KNN.m:1-60).
    Like the reference, C1/C2 are honoured only when BOTH are given (:8-14)."""
    C1, C2 = (bool(varargin[0]), bool(varargin[1])) if len(varargin) == 2 else (False, False)
    if getattr(pts, "dtype", None) == np.float32:          # class-preserving, like MATLAB: single in -> single out
        p = _fcol(np.asarray(pts).reshape(-1, 3), np.float32)
        n = p.shape[0]
        aligned = np.zeros((n, 3), dtype=np.float32, order="F"); coeff = np.zeros(9, np.float32); c = np.zeros(3, np.float32)
        check(lib().pcreg_align_points_knn_f32(_ptr(p, C.c_float), C.c_int(n), C.c_int(n), C.c_int(int(C1)), C.c_int(int(C2)),
                                               _ptr(aligned, C.c_float), _ptr(coeff, C.c_float), _ptr(c, C.c_float)))
        return np.ascontiguousarray(aligned), coeff.reshape(3, 3, order="F").copy(), c.reshape(1, 3)
    p = _pts3(pts, "pts")
    n = p.shape[0]
    aligned = np.zeros((n, 3), order="F")
    coeff = np.zeros(9)
    c = np.zeros(3)
    check(lib().pcreg_align_points_knn(_ptr(p, C.c_double), C.c_int(n), C.c_int(n), C.c_int(int(C1)), C.c_int(int(C2)),
                                       _ptr(aligned, C.c_double), _ptr(coeff, C.c_double), _ptr(c, C.c_double)))
    return np.ascontiguousarray(aligned), coeff.reshape(3, 3, order="F").copy(), c.reshape(1, 3)


def AlignPoints_KNN_batched(pts_list, C1: bool = False, C2: bool = False):
    """The same LRF for a list of supports in one launch; returns (aligned_list, coeff [B,3,3], c [B,3], status [B])."""
    B = len(pts_list)
    sizes = [np.asarray(p).shape[0] for p in pts_list]
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    total = int(offsets[-1])
    p = _pts3(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in pts_list], axis=0), "pts")
    aligned = np.zeros((max(total, 1), 3), order="F")
    coeff = np.zeros(9 * B); c = np.zeros(3 * B); status = np.zeros(B, dtype=np.int32)
    check(lib().pcreg_align_points_knn_batched(_ptr(p, C.c_double), C.c_int(total), C.c_int(total), _ptr(offsets, C.c_int32),
                                               C.c_int(B), C.c_int(int(C1)), C.c_int(int(C2)), _ptr(aligned, C.c_double),
                                               _ptr(coeff, C.c_double), _ptr(c, C.c_double), _ptr(status, C.c_int32)))
    al = [np.ascontiguousarray(aligned[offsets[b]:offsets[b + 1]]) for b in range(B)]
    return al, coeff.reshape(B, 3, 3).transpose(0, 2, 1).copy(), c.reshape(B, 3), status


# ------------------------------------------------------- getSpacialHistogramDescriptors
def _desc_opts(options: dict) -> DescOpts:
    kk = options["k"]
    kf = 1.0 if (isinstance(kk, str) and kk == "all") or kk == 1 else float(kk)      # :75
    mx = options["max_pts"]
    mx = 2**31 - 1 if (mx == float("inf") or mx > 2**31 - 1) else int(mx)
    return DescOpts(int(options["min_pts"]), mx, float(options["R"]), (C.c_double * 2)(*[float(v) for v in options["thVar"]]),
                    kf, int(bool(options["ALIGN_POINTS"])))


def speedyDescriptors(pts, sample_opts: dict, options: dict, rng=None):
    """[feat, desc] = speedyDescriptors(pts, sample_opts, options)  (speedyDescriptors.m:2-82).

    The reference cuts the model into cuboid regions so that its brute-force getLocalPoints scans stay short, draws the
    keypoints of every region on the host (:55, :86-101) and calls getSpacialHistogramDescriptors once per region on the
    region's crop (+ a margin of R).  Every keypoint lies at least R inside its crop's bounding box, so its support is the same
    in the crop and in the whole cloud: here the keypoints are drawn exactly as the reference draws them (same regions, same
    order, same counts; `rng` -- a numpy Generator, default_rng(0) if None -- plays MATLAB's rand) and ALL of them go through
    ONE device call on the whole cloud (the uniform grid replaces the tiling): the same rows in the same order.
    -> (feat V x 3, desc V x 980, the sampled keypoints in region order)."""
    for k in ("max_region_size", "R"):
        if k not in options:
            raise KeyError(f"options.{k} is required (speedyDescriptors.m:10,33)")
    rng = rng or np.random.default_rng(0)
    p = np.asarray(pts)
    d, R = float(sample_opts["d"]), float(options["R"])
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)          # :18-19 (pointCloud limits)
    ext = hi - lo
    nreg = np.ceil(ext / float(options["max_region_size"])).astype(np.int64)              # :20
    step = ext / nreg                                                                     # :21
    edges = [lo[a] + step[a] * np.arange(int(np.floor(ext[a] / step[a] + 1e-10)) + 1) for a in range(3)]    # :24-26
    if [len(e) - 1 for e in edges] != nreg.tolist():                                      # :27
        raise AssertionError("region bounds do not tile the cloud")
    if options.get("VERBOSE", 0):
        print(f"Divided model into {int(nreg.prod())} regions")                           # :35-37
    draws = []
    for ix in range(nreg[0]):                                                             # :44-46
        inx = (p[:, 0] > edges[0][ix] - R) & (p[:, 0] < edges[0][ix + 1] + R)
        for iy in range(nreg[1]):
            inxy = inx & (p[:, 1] > edges[1][iy] - R) & (p[:, 1] < edges[1][iy + 1] + R)
            for iz in range(nreg[2]):
                crop = p[inxy & (p[:, 2] > edges[2][iz] - R) & (p[:, 2] < edges[2][iz + 1] + R)]        # :48-52
                if crop.shape[0] <= 500:                                                  # :87 / :99
                    continue
                clo, chi = crop.min(axis=0).astype(np.float64), crop.max(axis=0).astype(np.float64)
                span = (chi - clo) - 2.0 * R                                              # :89-91, margin = -R
                num = float(span[0] * span[1] * span[2]) / d ** 3
                num = int(math.floor(num + 0.5)) if num >= 0 else -int(math.floor(-num + 0.5))          # :92 round
                draws.append(rng.random((max(num, 0), 3)) * span + clo + R)              # :95-101
    kp = np.vstack(draws) if draws else np.zeros((0, 3))
    if kp.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros((0, 980)), kp
    opt = dict(options); opt["VERBOSE"] = 0                                               # :12
    feat, desc = getSpacialHistogramDescriptors(p, kp, opt)                               # ONE call instead of :58-59 per region
    return feat, desc, kp


def getSpacialHistogramDescriptors(pts, sample_pts, options: dict):
    """[feat, desc] = getSpacialHistogramDescriptors(pts, sample_pts, options)
    (getSpacialHistogramDescriptors.m:2-183): feat V x 3 keypoint locations, desc V x 980
    spherical count histograms of the surviving keypoints, in input order."""
    for k in ("min_pts", "max_pts", "R", "thVar", "k", "ALIGN_POINTS"):        # :18-23
        if k not in options:
            raise KeyError(f"options.{k} is required (getSpacialHistogramDescriptors.m:18-23)")
    import time
    t0 = time.time()
    ps, ss = getattr(pts, "dtype", None) == np.float32, getattr(sample_pts, "dtype", None) == np.float32
    if ps or ss:
        # `single` data (pcread; completeExperimentFast.m:309).  feat / desc are DOUBLE (the reference preallocates them with
        # nan(...), getSpacialHistogramDescriptors.m:61-62); getLocalPoints' element-wise single arithmetic -- which keypoints
        # survive, which points form a support -- is reproduced (include/pcreg.h)
        p = _fcol(np.asarray(pts).reshape(-1, 3), np.float32 if ps else np.float64)
        s = _fcol(np.asarray(sample_pts).reshape(-1, 3), np.float32 if ss else np.float64)
        P, S = p.shape[0], s.shape[0]
        o = _desc_opts(options)
        feat = np.zeros((max(S, 1), 3)); desc = np.zeros((max(S, 1), 980))
        V = C.c_int(0)
        check(lib().pcreg_spatial_histogram_descriptors_mixed(p.ctypes.data_as(C.c_void_p), C.c_int(int(ps)), C.c_int(P), C.c_int(P),
                                                              s.ctypes.data_as(C.c_void_p), C.c_int(int(ss)), C.c_int(S), C.c_int(S), C.byref(o),
                                                              _ptr(feat, C.c_double), _ptr(desc, C.c_double), C.byref(V)))
        if options.get("VERBOSE", 1):
            print("Calculated descriptors in %0.1f seconds..." % (time.time() - t0))
        return feat[:V.value].copy(), desc[:V.value].copy()
    p, s = _pts3(pts, "pts"), _pts3(sample_pts, "sample_pts")
    P, S = p.shape[0], s.shape[0]
    o = _desc_opts(options)
    feat = np.zeros((max(S, 1), 3))
    desc = np.zeros((max(S, 1), 980))
    V = C.c_int(0)
    check(lib().pcreg_spatial_histogram_descriptors(_ptr(p, C.c_double), C.c_int(P), C.c_int(P), _ptr(s, C.c_double),
                                                    C.c_int(S), C.c_int(S), C.byref(o), _ptr(feat, C.c_double),
                                                    _ptr(desc, C.c_double), C.byref(V)))
    if options.get("VERBOSE", 1):
        print("Calculated descriptors in %0.1f seconds..." % (time.time() - t0))       # :181
    return feat[:V.value].copy(), desc[:V.value].copy()


# ----------------------------------------------------------------- transform helpers
def quickTF(pts, TF) -> np.ndarray:
    """quickTF.m:5-7 -- [pts 1] * TF (host arithmetic: 12 flops per point, not a hot path)."""
    pts = np.asarray(pts, dtype=np.float64)
    return (np.hstack([pts, np.ones((pts.shape[0], 1))]) @ np.asarray(TF, dtype=np.float64))[:, :3]


def invertTF(TF) -> np.ndarray:
    """invertTF.m:5-7."""
    TF = np.asarray(TF, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = TF[:3, :3].T
    out[3, :3] = -TF[3, :3] @ TF[:3, :3].T
    return out
