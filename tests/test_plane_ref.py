"""The point-to-plane reference (tests/plane_ref.py) on known answers, and the premises of the GPU test's main scene, without a GPU.

Known answers, in float64 pairs (no fp32 rounding of the moved points, so the limit is double's): three mutually orthogonal plane
patches with exact normals, and points on them displaced by a known small rigid motion D.  With every point on its plane the
residuals vanish exactly at invertTF(D), and the three normals constrain all six unknowns, so that is the unique minimiser.  The
linearisation drops the terms of second order in the motion: one step leaves an error that falls by about four when the motion
is halved, and since each step squares the relative error, four steps from a motion of 0.02 reach the rounding level -- asserted
below 1e-12 at coordinates below ten.  A flat model (all normals (0, 0, 1)) leaves in-plane sliding free: A_22 = A_33 = A_44 = 0
and the fit is empty.

Premises of tests/test_gpu_refit_plane.py, from the references alone: the chunk, block and tile counts; the smallest pivot of the
scaled matrix is at least 1e-2 for every non-empty candidate at every radius; after five steps from the largest perturbation the
plane reference's RMS distance from the truth is at most 1/6 of refit_ref's."""
import os

import numpy as np

import plane_ref
import refit_ref
from oracle.pcreg_oracle import invertTF

CORES = min(len(os.sched_getaffinity(0)), 16)
R15 = np.float32(1.5) ** 2
RADII = [np.float32(0.0), np.float32(0.5) ** 2, R15, np.float32(np.inf)]


def _patches():
    """rows on a 0.25 lattice of [2, 8]^2 on each of the planes x = 0, y = 0, z = 0, with the plane's unit normal; 150 points on
    each patch's inner part [3, 7]^2"""
    g = np.arange(2.0, 8.0 + 1e-9, 0.25)
    a, b = (v.ravel() for v in np.meshgrid(g, g))
    z = np.zeros_like(a)
    rows = np.vstack([np.column_stack([z, a, b]), np.column_stack([a, z, b]), np.column_stack([a, b, z])])
    nrm = np.repeat(np.eye(3), len(a), axis=0)
    rng = np.random.default_rng(3)
    u, v = rng.uniform(3, 7, (2, 150))
    zz = np.zeros(150)
    pts = np.vstack([np.column_stack([zz, u, v]), np.column_stack([u, zz, v]), np.column_stack([u, v, zz])])
    return rows, nrm, pts


def _step64(rows, nrm, pts, T, o):
    """one reference step on float64 pairs: the nearest row of every moved point by brute force"""
    p = pts @ T[:3, :3] + T[3, :3]
    near = ((p[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
    S, pivot = plane_ref.fit(*plane_ref.sums_of_pairs(rows[near], p, nrm[near], o), o)
    return None if S is None else refit_ref.compose(T, S), pivot


def _error_after(steps, scale):
    rows, nrm, pts = _patches()
    o = np.array([4.0, 4.0, 4.0])
    D = plane_ref.about(plane_ref.rigid([0.02 * scale, -0.015 * scale, 0.01 * scale], [0.03 * scale, 0.02 * scale, -0.025 * scale]), o)
    moved = pts @ D[:3, :3] + D[3, :3]
    T, errs = np.eye(4), []
    for _ in range(steps):
        T, pivot = _step64(rows, nrm, moved, T, o)
        assert T is not None and pivot > 1e-2, pivot
        errs.append(float(np.linalg.norm(T - invertTF(D))))
    return float(np.linalg.norm(np.eye(4) - invertTF(D))), errs


def test_three_orthogonal_patches_recover_a_known_motion():
    e0, full = _error_after(4, 1.0)
    _, half = _error_after(1, 0.5)
    print(f"|I - inv(D)| = {e0:.3e}; after 1 .. 4 steps {['%.3e' % e for e in full]}; one step from half the motion {half[0]:.3e}")
    assert full[0] < e0 * e0                                   # second order: below the square of the motion's own size ...
    assert 3.0 < full[0] / half[0] < 5.0                       # ... and a quarter of it for half the motion
    assert full[3] < 1e-12


def test_a_flat_model_is_empty():
    g = np.arange(0.0, 10.0, 0.5)
    a, b = (v.ravel() for v in np.meshgrid(g, g))
    rows = np.column_stack([a, b, np.zeros_like(a)])
    nrm = np.tile([0.0, 0.0, 1.0], (len(rows), 1))
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(1, 9, (200, 2)), rng.normal(0, 0.01, 200)])
    T, _ = _step64(rows, nrm, pts, np.eye(4), np.array([5.0, 5.0, 0.0]))
    assert T is None
    sums, n = plane_ref.sums_of_pairs(rows[:200], pts, nrm[:200], np.array([5.0, 5.0, 0.0]))
    assert n == 200 and sums[plane_ref.tri(2, 2)] == 0 and sums[plane_ref.tri(3, 3)] == 0 and sums[plane_ref.tri(4, 4)] == 0
    assert plane_ref.finish64(sums.astype(np.float64), n, [5.0, 5.0, 0.0]) is None


def test_finish64_follows_the_extended_reference():
    """the float64 restatement against the longdouble fit on the main scene's sums: far inside the GPU test's bound of 1e-9"""
    sc = plane_ref.scene()
    want = plane_ref.scene_ref(R15, threads=CORES)
    o = plane_ref.origin(sc["model"])
    for b in range(4):
        sums, n = plane_ref.plane_sums(sc["model"], sc["normals"], want["idx"][b], want["tq"][b], o)
        got = plane_ref.finish64(sums.astype(np.float64), n, o)
        assert np.linalg.norm(got.reshape(4, 4).T - want["T_step"][b]) < 1e-12
    assert plane_ref.finish64(np.zeros(28), 100, o) is None and plane_ref.finish64(sums.astype(np.float64), 5, o) is None


def test_the_gpu_scene_is_what_its_checks_need():
    sc = plane_ref.scene()
    Q, M = len(sc["surf"]), len(sc["model"])
    assert 2049 <= Q <= 3000 and (Q + 2047) // 2048 == 2 and (Q + 511) // 512 >= 5 and (M + 511) // 512 == 8
    assert np.isfinite(sc["normals"]).all()
    for r2 in RADII:
        want = plane_ref.scene_ref(r2, threads=CORES)
        live = ~want["empty"]
        print(f"r2 = {float(r2):.4g}: n_close {want['n_close'].tolist()}, n_plane {want['n_plane'].tolist()}, empty {want['empty'].tolist()}, "
              f"smallest pivots {want['pivot'].tolist()}")
        assert (want["pivot"][live] >= 1e-2).all()
        assert want["empty"][4:].all() and (want["n_close"][4:] == 0).all()
    want = plane_ref.scene_ref(R15, threads=CORES)
    assert want["empty"].tolist() == [False] * 4 + [True] * 2 and (want["n_plane"][:4] > 2000).all()


def test_five_plane_steps_beat_five_point_steps_by_six():
    """what the feature is for, in the references: from the largest perturbation at r = 1.5"""
    sc = plane_ref.scene()
    Tp = Tq = sc["T"][3:4]
    start = plane_ref.rms_to_truth(sc["surf"], Tp[0], sc["cloud"])
    for _ in range(5):
        a = plane_ref.step(sc["surf"], sc["model"], sc["normals"], Tp, R15, threads=CORES)
        b = refit_ref.step(sc["surf"], sc["model"], Tq, R15, threads=CORES)
        assert not a["empty"][0] and not b["empty"][0] and a["pivot"][0] >= 1e-2
        Tp, Tq = a["T_out"], b["T_out"]
    plane, point = (plane_ref.rms_to_truth(sc["surf"], T[0], sc["cloud"]) for T in (Tp, Tq))
    print(f"RMS distance from the truth: start {start:.4f}, five plane steps {plane:.4f}, five point-to-point steps {point:.4f}, ratio {plane / point:.4f}")
    assert plane <= point / 6.0
