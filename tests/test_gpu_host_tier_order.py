"""The host-tier entries share one grow-only pool of staging buffers, taken in call order (Stage, common.hpp).  Every entry is
called twice in one process on the same small inputs -- once in a fixed order with sizes that grow from call to call (every call
regrows the buffers it meets), once in the reverse order (sizes shrink: every call meets buffers larger than it needs, left by
other entries) -- and every output of every call must be the same, bit for bit.  A buffer that a later take moved or overwrote
under a live pointer shows up as a difference."""
import numpy as np
import pytest

from test_gpu_descriptors import OPT, keypoints, strips
from test_gpu_sweep import OPT as RANSAC_OPT, PAR, _scene

pytestmark = pytest.mark.gpu


def _flat(x, out=None):
    """Every array / scalar of a nested result, in a fixed order."""
    out = [] if out is None else out
    if isinstance(x, dict):
        for k in sorted(x):
            _flat(x[k], out)
    elif isinstance(x, (list, tuple)):
        out.append(np.asarray(len(x)))
        for v in x:
            _flat(v, out)
    elif x is None:
        out.append(np.asarray(-1))
    else:
        out.append(np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x))
    return out


def _pairs3(n, seed):
    import oracle.pcreg_oracle as o
    rng = np.random.default_rng(seed)
    p1 = rng.uniform(-20, 20, (n, 3))
    p2 = p1 @ o.eul2rotm(np.array([0.2, -0.1, 0.3])).T + np.array([1.0, 2.0, -0.5]) + rng.normal(0, 0.05, (n, 3))
    p2[::3] = rng.uniform(-20, 20, (len(p2[::3]), 3))                      # a third are outliers
    return p1, p2


def _descs(Q, M, D, seed):
    rng = np.random.default_rng(seed)
    dM = rng.poisson(3.0, (M, D)).astype(np.float64)
    dS = dM[rng.choice(M, Q, replace=False)] + rng.poisson(0.15, (Q, D))
    return dS, dM


def _row_lists(M, S, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(M, M // 3 + 7 * z, replace=False)).astype(np.int32) for z in range(S)]


def _sweep_inputs(pc, VM, seed):
    """test_gpu_sweep's scene at VM model keypoints and its six fullest spheres."""
    import oracle.pcreg_oracle as o
    featM, descM, featS, descS = _scene(seed=seed, VM=VM, VS=160 + VM // 20, D=48)
    centres = o.pcUniformSamples(featM, 8.0)
    return featM, descM, featS, descS, centres


def _calls(pc):
    """[(name, function without arguments)] in the listed order; call i works on n(i) rows, growing with i."""
    from pcreg_amd._lib import lib
    n = lambda i: 400 + 220 * i
    coef = dict(RANSAC_OPT, iterNum=600)
    calls = []
    add = lambda name, f: calls.append((name, f))

    p1a, p2a = _pairs3(n(0), 1)
    add("estimateTransform", lambda: pc.estimateTransform(p1a, p2a))
    p1b, p2b = _pairs3(n(1), 2)
    Tb = np.eye(4); Tb[3, :3] = [1.0, 2.0, -0.5]
    add("calcDists", lambda: pc.calcDists(Tb, p1b, p2b))
    p1c, p2c = _pairs3(n(2), 3)
    add("ransac", lambda: pc.ransac(p1c, p2c, coef, pc.estimateTransform, pc.calcDists, seed=5, return_iter_counts=True))
    parts = [_pairs3(n(3) // 3 + 50 * b, 10 + b) for b in range(3)]
    add("ransac_batched", lambda: pc.ransac_batched([p[0] for p in parts], [p[1] for p in parts], coef, seed=6))

    dS4, dM4 = _descs(n(4) // 2, n(4), 48, 4)
    add("getMatches", lambda: pc.getMatches(dS4, dM4, PAR))
    dS5, dM5 = _descs(n(5) // 2, n(5), 48, 5)
    add("matchFeatures", lambda: pc.matchFeatures(dS5, dM5, Method="Exhaustive", MatchThreshold=10.0, MaxRatio=0.99, Metric="SAD", Unique=True))

    def on_set(dS, dM, rows):
        with pc.DescSet(dS) as hS, pc.DescSet(dM) as hM:
            return pc.getMatchesOnSet(hS, hM, rows, PAR)
    dS6, dM6 = _descs(n(6) // 2, n(6), 48, 6)
    rows6 = _row_lists(n(6), 1, 6)[0]
    add("getMatchesOnSet(rows)", lambda: on_set(dS6, dM6, rows6))
    dS7, dM7 = _descs(n(7) // 2, n(7), 48, 7)
    add("getMatchesOnSet(all)", lambda: on_set(dS7, dM7, None))
    dS8, dM8 = _descs(n(8) // 2, n(8), 48, 8)
    rl8 = _row_lists(n(8), 5, 8)
    add("getMatchesSegmented", lambda: pc.getMatchesSegmented(dS8, dM8, rl8, PAR))
    dS9, dM9 = _descs(n(9) // 2, n(9), 48, 9)
    rl9 = _row_lists(n(9), 6, 9)

    def seg_on_set():
        with pc.DescSet(dS9) as hS, pc.DescSet(dM9) as hM:
            return pc.getMatchesSegmentedOnSet(hS, hM, rl9, PAR)
    add("getMatchesSegmentedOnSet", seg_on_set)

    R = 9.0
    fM10, _, _, _, c10 = _sweep_inputs(pc, n(10), 10)
    add("sphereCounts", lambda: pc.sphereCounts(fM10, c10, R))
    fM11, dM11, fS11, dS11, c11 = _sweep_inputs(pc, n(11), 11)
    fM12, dM12, fS12, dS12, c12 = _sweep_inputs(pc, n(12), 12)

    def kept(featM, centres):
        counts = pc.sphereCounts(featM, centres, R)
        keep = np.argsort(-counts, kind="stable")[:6]
        return centres[np.sort(keep)], counts[np.sort(keep)]

    def sweep():
        c, nd = kept(fM11, c11)
        with pc.DescSet(dS11) as hS, pc.DescSet(dM11) as hM:
            return pc.sphereSweep(hS, hM, fS11, fM11, c, nd, R, PAR, 20, coef, seed=3)
    add("sphereSweep", sweep)

    def sweep_on_model():
        c, nd = kept(fM12, c12)
        with pc.DescSet(dS12) as hS, pc.DescSet(dM12) as hM, pc.SphereModel(hM, fM12, c, nd, R) as sm:
            return pc.sphereSweepOnModel(sm, hS, fS12, PAR, 20, coef, seed=3)
    add("SphereModel + sphereSweepOnModel", sweep_on_model)

    # the final stage: a crop of a strip model seen in another frame, three clusters around the true transform
    import oracle.pcreg_oracle as o
    model = strips(6000, 5)
    rng = np.random.default_rng(14)
    T_true = np.eye(4); T_true[:3, :3] = o.eul2rotm(np.array([0.4, -0.25, 0.15])); T_true[3, :3] = [3.0, -2.0, 1.5]
    surface = o.quickTF(model[(model[:, 0] > 8) & (model[:, 0] < 42)], T_true)
    kpM = keypoints(500, 7)
    opt = dict(OPT, min_pts=40, ALIGN_POINTS=False)

    def jitter(ang, sh):
        dT = np.eye(4); dT[:3, :3] = o.eul2rotm(rng.normal(0, ang, 3)); dT[3, :3] = rng.normal(0, sh, 3)
        return T_true @ dT
    clusters = [(np.array([25.0, 18.0, 12.0]), jitter(0.004, 0.03)), (np.array([24.0, 19.0, 12.0]), jitter(0.012, 0.1)),
                (np.array([20.0, 24.0, 11.0]), jitter(0.008, 0.05))]
    near = kpM[(kpM[:, 0] > 10) & (kpM[:, 0] < 40)][:170]
    kps = [near + rng.normal(0, 0.05, near.shape) for _ in clusters]
    add("finalStageLimits", lambda: pc.finalStageLimits(surface, [c[1] for c in clusters]))

    def final_stage():
        featM, descM = pc.getSpacialHistogramDescriptors(model, kpM, opt)     # the model side of the stage, a host-tier call of its own
        assert len(featM) > 100
        assert all(len(k) * descM.shape[1] * 8 > 1 << 20 for k in kps)      # 170 keypoints x 7.84 KB > 1 MB: three batches of one cluster
        L = lib()
        assert L.pcreg_debug_set(b"final_batch_mb", 1) == 0
        try:
            with pc.DescSet(descM) as hM:
                return featM, descM, pc.finalStage(hM, featM, surface, clusters, kps, opt, PAR, 14.0, 1.5)
        finally:
            L.pcreg_debug_set(b"final_batch_mb", 0)
    add("finalStage", final_stage)

    cloud15 = strips(n(15), 15)
    add("getLocalPoints", lambda: pc.getLocalPoints(cloud15, 6.0, np.array([30.0, 18.0, 12.0]), 10, np.inf))
    cloud16, kp16 = strips(n(16), 16), keypoints(60, 17)
    add("getSpacialHistogramDescriptors", lambda: pc.getSpacialHistogramDescriptors(cloud16, kp16, dict(OPT, min_pts=20)))
    sup = [np.random.default_rng(18 + b).normal(0, [3.0, 1.0, 0.3], (n(17) // 4 + 30 * b, 3)) for b in range(4)]
    add("AlignPoints_KNN_batched", lambda: pc.AlignPoints_KNN_batched(sup, True, True))

    def clouds(i):
        rng = np.random.default_rng(100 + i)
        m = (rng.random((n(i), 3)) * [100, 56, 99]).astype(np.float32)
        q = (m[rng.choice(n(i), n(i) // 2, replace=False)] + rng.normal(0, 0.05, (n(i) // 2, 3))).astype(np.float32)
        return q, m
    q18, m18 = clouds(18)
    add("knn2_points", lambda: pc.knn2_points(q18, m18))
    q19, m19 = clouds(19)
    add("knn_points", lambda: pc.knn_points(q19, m19, 5))
    q20, m20 = clouds(20)
    add("match_points", lambda: pc.match_points(q20, m20, 0.5, 0.9, True))
    q21, m21 = clouds(21)

    def model_match():
        with pc.Model(m21) as h:
            return pc.Model.match_points(h, q21, 0.5, 0.9, True)
    add("Model.match_points", model_match)
    q22, m22 = clouds(22)

    def model_knn():
        with pc.Model(m22) as h:
            return pc.Model.knn(h, q22, 7)
    add("Model.knn", model_knn)
    return calls


def test_every_entry_gives_the_same_bits_in_either_order():
    import pcreg_amd as pc
    calls = _calls(pc)
    assert len(calls) == 23
    first = {name: _flat(f()) for name, f in calls}                         # sizes grow from call to call
    second = {name: _flat(f()) for name, f in reversed(calls)}              # and shrink
    for name, _ in calls:
        a, b = first[name], second[name]
        assert len(a) == len(b) and sum(x.size for x in a) > 0, name
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    # the calls do something: pairs, trials and a refined transform exist
    assert len(first["getMatches"][0]) > 50 and len(first["getMatchesOnSet(rows)"][0]) > 10
    assert sum(x.size for x in first["sphereSweep"]) > 1000 and sum(x.size for x in first["finalStage"]) > 1000
    assert len(first["getSpacialHistogramDescriptors"][1]) > 0              # keypoints survive
