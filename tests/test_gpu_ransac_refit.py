"""One RANSAC refit per call, against the oracle's counts and an extended-precision reference of the transform.

A call with iterNum = 1 and a one-row sample table returns that hypothesis's refit as T and its refined inlier set as the
inlier list; with REFINE off it returns the first pass.  The staged chain (one registration of n >= 4096 on the device
tier, pcreg_dev_ransac) is driven in its four modes -- default (refit sums on the int8 matrix cores), "ransac_nolane",
"ransac_fused", "ransac_f64score" -- and the host tier (pcreg_ransac, which returns both per-iteration counts) at the
sizes of its kernels: 1500 (LDS-resident), 2500 (fp64 on the raw coordinates) and 3500 (tiled).

The scenes (ransac_refit_scenes.py) hold knife-edge rows that stay within 1e-9 .. 1e-4 of thDist in BOTH passes, so a
refit that is wrong in the ninth digit changes a count.  Per scene, hypothesis and mode:
  1. first-pass count and inlier list (the REFINE-off call), refined count, numSuccess, maxInliers and the inlier list are
     the oracle's, bit for bit;
  2. e_dev = |T_dev - T_x|_F <= 8 e_ref + 32 eps |T_x|_F, with T_x = refit_reference on the oracle's first-pass inlier rows
     and e_ref = |T_oracle - T_x|_F: the device may be 8 times further from the truth than the oracle's plain fp64 sums
     (another, equally legitimate order of summation), above a floor for the one rounding of T_x and the 3 x 3 algebra;
  3. T of the default mode and of "ransac_nolane" / "ransac_fused" agree to 1e-10 (1 + max |coordinate|).
Each test prints its figures (REFIT lines: scene, n, mode, max e_dev, max e_ref, max e_dev / bar) before it asserts.
"""
import numpy as np
import pytest

from ransac_refit_scenes import HOST_SCENES, STAGED_SCENES, coef_of, prepare
from test_gpu_ransac_bound import _dev_ransac

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
STAGED_MODES = ("default", "ransac_nolane", "ransac_fused", "ransac_f64score")


def _judge(name, n, mode, runs, s):
    """runs: per usable hypothesis (h, first-pass count, first-pass list or None, refined count, numSuccess, maxInliers, list, T)."""
    bad, worst, e_dev_max, e_ref_max = [], 0.0, 0.0, 0.0
    for i, (h, c1, l1, c2, ns, mi, inl, T) in enumerate(runs):
        ref, ref1 = h["ref"], h["ref1"]
        if c1 != ref["inlrNum"][0] or (l1 is not None and not np.array_equal(l1, ref1["inlierIdx"])):
            bad.append("%s hyp %d: first pass %d against the oracle's %d" % (mode, i, c1, ref["inlrNum"][0]))
        if (c2, ns, mi) != (ref["inlrNum_refined"][0], ref["numSuccess"], ref["maxInliers"]) or not np.array_equal(inl, ref["inlierIdx"]):
            bad.append("%s hyp %d: refined count %d numSuccess %d maxInliers %d (%d listed) against the oracle's %d %d %d" %
                       (mode, i, c2, ns, mi, len(inl), ref["inlrNum_refined"][0], ref["numSuccess"], ref["maxInliers"]))
        e_dev = float(np.linalg.norm(T - h["Tx"])) if np.shape(T) == (4, 4) else np.inf
        bar = 8.0 * h["e_ref"] + 32.0 * EPS * float(np.linalg.norm(h["Tx"]))
        worst = max(worst, e_dev / bar); e_dev_max = max(e_dev_max, e_dev); e_ref_max = max(e_ref_max, h["e_ref"])
        if not e_dev <= bar:
            bad.append("%s hyp %d: e_dev %.3e over 8 e_ref + floor = %.3e (e_ref %.3e)" % (mode, i, e_dev, bar, h["e_ref"]))
    print("\nREFIT %-20s n %5d %-16s e_dev %.3e e_ref %.3e e_dev/e_ref %8.3f e_dev/bar %.3f unusable %d" %
          (name, n, mode, e_dev_max, e_ref_max, e_dev_max / e_ref_max if e_ref_max else np.inf, worst, s["n_unusable"]))
    return bad


@pytest.mark.parametrize("name,n", STAGED_SCENES)
def test_staged_chain_refit(name, n, debug_set):
    s = prepare(name, n)
    usable = [h for h in s["hyps"] if h["usable"]]
    bad, T_of = [], {}
    for mode in STAGED_MODES:
        if mode != "default":
            debug_set(mode, 1)
        runs = []
        for h in usable:
            r1 = _dev_ransac(s["p1"], s["p2"], coef_of(s, refine=False), 0, sample_idx=h["table"])
            r = _dev_ransac(s["p1"], s["p2"], coef_of(s), 0, sample_idx=h["table"])
            assert r["n"] == n
            if r["failed"] or r1["failed"]:
                bad.append("%s: a call failed" % mode)
                continue
            runs.append((h, r1["max_inliers"], r1["inl"], r["max_inliers"], r["num_success"], r["max_inliers"], r["inl"], r["T"]))
        if mode != "default":
            debug_set(mode, 0)
        bad += _judge(name, n, mode, runs, s)
        T_of[mode] = [run[-1] for run in runs]
    tol = 1e-10 * (1.0 + max(np.abs(s["p1"]).max(), np.abs(s["p2"]).max()))
    for mode in STAGED_MODES:
        if len(T_of[mode]) != len(usable):
            bad.append("%s: %d transforms for %d hypotheses" % (mode, len(T_of[mode]), len(usable)))
    for mode in ("ransac_nolane", "ransac_fused"):
        for i, (a, b) in enumerate(zip(T_of["default"], T_of[mode])):
            if not np.abs(a - b).max() <= tol:
                bad.append("default against %s, hyp %d: %.3e over %.3e" % (mode, i, np.abs(a - b).max(), tol))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,n", HOST_SCENES)
def test_host_tier_kernels_refit(name, n):
    """The scenes that move row 0, at the sizes of the resident, raw-coordinate and tiled kernels."""
    import pcreg_amd as pc
    s = prepare(name, n)
    runs = []
    for h in s["hyps"]:
        if not h["usable"]:
            continue
        T, inl, ns, mi, _, it1, it2 = pc.ransac(s["p1"], s["p2"], coef_of(s), sample_idx=h["table"], return_iter_counts=True)
        runs.append((h, int(it1[0]), None, int(it2[0]), ns, mi, np.asarray(inl).astype(np.int64), T))
    bad = _judge(name, n, "host", runs, s)
    assert not bad, "\n".join(bad)
