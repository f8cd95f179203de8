"""The plane-to-plane reference (tests/gicp_ref.py) and the premises of tests/test_gpu_refit_gicp.py, without a GPU.

On plane_ref.scene() with surface normals from normals_ref at k = 8: the smallest pivot of the scaled 6 x 6 matrix is at least 1e-2
for every non-empty transform at r = 0.5, 1.5 and +inf; five reference steps from each of the four perturbed starts end nearer
the truth than five reference point-to-plane steps; a flat model, which leaves the point-to-plane step empty, has pivots far above
1e-2 here.  Of the float64 restatement pair64: epsilon = 1 gives S = 2 I exactly, and negating either normal changes no bit.
The relative error of the float64 restatement's sum_res2 against the longdouble reference is measured over the main scene's
radii and epsilon in {1e-3, 1e-2}: the GPU test's bound on sum_res2 is 8 x the worst of these, and not below 1e-12."""
import os

import numpy as np

import gicp_ref
import plane_ref

CORES = min(len(os.sched_getaffinity(0)), 16)
R15 = np.float32(1.5) ** 2
RADII = [np.float32(0.0), np.float32(0.5) ** 2, R15, np.float32(np.inf)]
SUM_RES2_BOUND = 1e-12                                # tests/test_gpu_refit_gicp.py's: max(8 x the worst measured below, 1e-12)


def flat_scene():
    """tests/test_gpu_refit_gicp.py's flat model: a 64 x 64 lattice of pitch 0.5 at z = 2, normals (0, 0, 1); 600 points of the plane
    z = 2 over the lattice's interior, their normals (0, 0, 1), and the starts: a shift along the plane, and a small rotation about
    the plane's normal with a lift off it"""
    g = np.arange(64) * 0.5
    a, b = (v.ravel() for v in np.meshgrid(g, g))
    model = np.column_stack([a, b, np.full_like(a, 2.0)]).astype(np.float32)
    rng = np.random.default_rng(21)
    pts = np.column_stack([rng.uniform(6, 25, (600, 2)), np.full(600, 2.0)]).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(model), 1))
    nq = np.tile(np.float32([0, 0, 1]), (len(pts), 1))
    c = pts.mean(axis=0).astype(np.float64)
    T = np.stack([plane_ref.rigid([0, 0, 0], [0.11, -0.07, 0.0]), plane_ref.about(plane_ref.rigid([0.004, 0, 0], [0.05, 0.02, 0.03]), c)])
    return dict(model=model, pts=pts, normals=nrm, qnormals=nq, T=T)


def test_pivots_of_the_main_scene():
    sc = plane_ref.scene()
    nq = gicp_ref.surface_normals()
    assert nq.shape == sc["surf"].shape and np.isfinite(nq).all()
    for r2 in RADII[1:]:
        want = gicp_ref.scene_ref(r2, threads=CORES)
        live = ~want["empty"]
        print(f"r2 = {float(r2):.4g}: n_close {want['n_close'].tolist()}, n_pairs {want['n_pairs'].tolist()}, empty {want['empty'].tolist()}, "
              f"smallest pivots {want['pivot'].tolist()}")
        assert live[:4].all() and want["empty"][4:].all() and (want["n_close"][4:] == 0).all()
        assert (want["pivot"][live] >= 1e-2).all()
        assert (want["n_pairs"] == want["n_close"]).all()          # unit normals: S factorises for every pair
    want = gicp_ref.scene_ref(RADII[0], threads=CORES)
    assert want["empty"].all() and (want["n_pairs"] < 6).all()


def test_five_steps_end_nearer_the_truth_than_five_plane_steps():
    sc = plane_ref.scene()
    nq = gicp_ref.surface_normals()
    Tg = Tp = sc["T"][:4]
    for _ in range(5):
        a = gicp_ref.step(sc["surf"], sc["model"], sc["normals"], nq, Tg, R15, threads=CORES)
        b = plane_ref.step(sc["surf"], sc["model"], sc["normals"], Tp, R15, threads=CORES)
        assert not a["empty"].any() and not b["empty"].any() and (a["pivot"] >= 1e-2).all()
        Tg, Tp = a["T_out"], b["T_out"]
    for s in range(4):
        gicp, plane = (plane_ref.rms_to_truth(sc["surf"], T[s], sc["cloud"]) for T in (Tg, Tp))
        print(f"start {s}: RMS distance from the truth after five plane-to-plane steps {gicp:.5f}, after five point-to-plane steps {plane:.5f}")
        assert gicp < plane


def test_a_flat_model_keeps_its_pivots():
    fl = flat_scene()
    plane = plane_ref.step(fl["pts"], fl["model"], fl["normals"], fl["T"], np.float32(1.0), threads=CORES)
    gicp = gicp_ref.step(fl["pts"], fl["model"], fl["normals"], fl["qnormals"], fl["T"], np.float32(1.0), threads=CORES)
    print(f"flat model: n_pairs {gicp['n_pairs'].tolist()}, smallest pivots {gicp['pivot'].tolist()}")
    assert plane["empty"].all() and (plane["n_plane"] == 600).all()
    assert not gicp["empty"].any() and (gicp["n_pairs"] == 600).all() and (gicp["pivot"] >= 1e-2).all()


def test_epsilon_one_gives_twice_the_identity():
    rng = np.random.default_rng(2)
    T16 = gicp_ref.t16(plane_ref.rigid([0.3, -0.2, 0.5], [1, 2, 3]))
    for _ in range(50):
        n, nq = rng.normal(size=(2, 3)).astype(np.float32)
        assert gicp_ref.pair64(n, nq, T16, 1.0 - 1.0, want_s=True) == [2.0, 0.0, 0.0, 2.0, 0.0, 2.0]
        W = gicp_ref.pair64(n, nq, T16, 0.0)
        assert W[1] == 0.0 and W[2] == 0.0 and W[4] == 0.0 and W[0] == W[3] == W[5] and abs(W[0] - 0.5) < 1e-15


def test_the_sign_of_a_normal_changes_no_bit():
    rng = np.random.default_rng(4)
    T16 = gicp_ref.t16(plane_ref.rigid([0.3, -0.2, 0.5], [1, 2, 3]))
    for eps in (1e-6, 1e-3, 0.25):
        for _ in range(50):
            n, nq = (v / np.linalg.norm(v) for v in rng.normal(size=(2, 3)))
            n, nq = n.astype(np.float32), nq.astype(np.float32)
            W = gicp_ref.pair64(n, nq, T16, 1.0 - eps)
            assert W is not None
            for sn, sq in ((-1, 1), (1, -1), (-1, -1)):
                assert gicp_ref.pair64(sn * n, sq * nq, T16, 1.0 - eps) == W


def test_pair64_follows_the_extended_reference():
    rng = np.random.default_rng(6)
    R = plane_ref.rigid([0.3, -0.2, 0.5], [1, 2, 3])
    n, nq = (v / np.linalg.norm(v, axis=1, keepdims=True) for v in rng.normal(size=(2, 200, 3)))
    n, nq = n.astype(np.float32), nq.astype(np.float32)
    for eps in (1e-3, 1e-2):
        W, ok = gicp_ref.weights(n.astype(np.float64), nq.astype(np.float64) @ R[:3, :3], 1.0 - eps)
        assert ok.all()
        for k in range(200):
            w = gicp_ref.pair64(n[k], nq[k], gicp_ref.t16(R), 1.0 - eps)
            full = np.array([[w[0], w[1], w[2]], [w[1], w[3], w[4]], [w[2], w[4], w[5]]])
            assert np.abs(full - W[k].astype(np.float64)).max() <= 1e-12 / eps


def test_the_float64_sum_res2_measured_against_the_reference():
    sc = plane_ref.scene()
    nq = gicp_ref.surface_normals()
    worst = 0.0
    for eps in (1e-3, 1e-2):
        for r2 in RADII:
            want = gicp_ref.scene_ref(r2, eps, threads=CORES)
            for b in range(4):
                got, cnt = gicp_ref.sum_res2_64(sc["model"], sc["normals"], nq, want["idx"][b], want["tq"][b], sc["T"][b], eps)
                assert cnt == want["n_pairs"][b]
                if want["sum_res2"][b] > 0:
                    rel = abs(got - want["sum_res2"][b]) / want["sum_res2"][b]
                    worst = max(worst, rel)
    print(f"float64 sum_res2 against the longdouble reference, worst relative error {worst:.3e}; 8 x that {8 * worst:.3e}; the GPU test's bound "
          f"{SUM_RES2_BOUND:.1e}")
    assert max(8 * worst, 1e-12) <= SUM_RES2_BOUND
