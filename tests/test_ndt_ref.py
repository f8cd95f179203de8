"""The premises of the NDT step's GPU tests (tests/test_gpu_ndt.py), recomputed without a GPU on the reference
tests/ndt_ref.py: the main scene's voxel and Gaussian counts, its pairs per candidate, the conditioning of its normal equations,
five NDT steps against five point-to-point steps, a known small motion recovered from three orthogonal patches, and the empty
table."""
import numpy as np
import pytest

import ndt_ref
import plane_ref
import refit_ref

STEP = 4.0
PIVOT = 1e-2


@pytest.fixture(scope="module")
def main():
    sc = plane_ref.scene()
    return sc, ndt_ref.table(sc["model"], STEP, 6)


def test_the_main_scenes_table(main):
    sc, tab = main
    assert tab["n_voxels"] == 131 and len(tab["cells"]) == 124
    assert int(tab["voxel_counts"].sum()) == len(sc["model"]) and (tab["counts"] >= 6).all()
    assert (np.diff(ndt_ref.key_of(tab["cells"].astype(np.int64))) > 0).all()
    # the floor bounds the conditioning of every C by 100 (up to rounding)
    w = np.linalg.eigvalsh(ndt_ref.full(tab["C"]))
    assert (w[:, 0] > 0).all() and (w[:, 2] / w[:, 0] <= 100.0 * (1 + 1e-9)).all()
    err = np.linalg.norm((tab["C"].astype(ndt_ref.LD) - tab["C_ref"]).astype(np.float64) * [1, 2 ** 0.5, 2 ** 0.5, 1, 2 ** 0.5, 1], axis=1)
    ref = np.linalg.norm(tab["C_ref"].astype(np.float64) * [1, 2 ** 0.5, 2 ** 0.5, 1, 2 ** 0.5, 1], axis=1)
    print(f"worst |C - C_ref|_F / |C_ref|_F over {len(ref)} Gaussians: {(err / ref).max():.3e}")
    assert (err / ref).max() < 1e-13


@pytest.mark.parametrize("neighbors", [1, 7])
def test_pairs_and_pivots_of_the_main_scene(main, neighbors):
    sc, tab = main
    want = ndt_ref.step(sc["surf"], tab, sc["T"], neighbors)
    print(f"neighbors = {neighbors}: n_pairs {want['n_pairs'].tolist()}, pivots {np.round(want['pivot'], 3).tolist()}, sum_e {want['sum_e'].tolist()}")
    if neighbors == 1:                                     # nearly every moved point lies in a Gaussian voxel, whatever the perturbation
        assert want["n_pairs"][:4].tolist() == [2480, 2477, 2461, 2406]
    else:
        assert (want["n_pairs"][:4] > 3 * 2400).all() and (want["n_pairs"][:4] <= 7 * 2500).all()
    assert want["n_pairs"][4:].tolist() == [0, 0] and want["empty"].tolist() == [False] * 4 + [True] * 2
    assert (want["pivot"][:4] >= PIVOT).all()


def test_five_ndt_steps_against_five_point_to_point_steps(main):
    sc, tab = main
    outs = ndt_ref.steps(sc["surf"], tab, sc["T"][:4], 5)
    assert outs[-1]["n_pairs"].tolist() == [2479] * 4          # once the candidates have settled, each has the same 2479 pairs
    T = sc["T"][3:4]
    start = plane_ref.rms_to_truth(sc["surf"], T[0], sc["cloud"])
    ndt = outs[-1]["T_out"][3]
    p2p = T
    for _ in range(5):
        p2p = refit_ref.step(sc["surf"], sc["model"], p2p, np.float32(1.5) ** 2)["T_out"]
    a, b = plane_ref.rms_to_truth(sc["surf"], ndt, sc["cloud"]), plane_ref.rms_to_truth(sc["surf"], p2p[0], sc["cloud"])
    print(f"RMS to truth: start {start:.3f}, five NDT steps {a:.4f}, five point-to-point steps {b:.4f}")
    assert start > 0.7 and a <= b / 4


def _patches(rng, n=400):
    """three orthogonal planar patches of 12 x 12 with 0.01 noise off the plane, around (50, 60, 70)"""
    out = []
    for axis in range(3):
        p = rng.uniform(0, 12, (n, 3))
        p[:, axis] = rng.normal(0, 0.01, n)
        out.append(p)
    return np.vstack(out) + [50.0, 60.0, 70.0]


def test_three_orthogonal_patches_recover_a_small_motion():
    rng = np.random.default_rng(5)
    model = _patches(rng, 3000).astype(np.float32)
    cloud = _patches(rng, 400)
    P = plane_ref.about(plane_ref.rigid([0.01, -0.008, 0.012], [0.05, -0.04, 0.06]), cloud.mean(axis=0))
    surf = (cloud @ P[:3, :3] + P[3, :3]).astype(np.float32)
    tab = ndt_ref.table(model, 3.0, 6)
    assert len(tab["cells"]) >= 30
    before = plane_ref.rms_to_truth(surf, np.eye(4), cloud)
    out = ndt_ref.steps(surf, tab, np.eye(4)[None], 4, neighbors=7)
    after = plane_ref.rms_to_truth(surf, out[-1]["T_out"][0], cloud)
    print(f"RMS to truth {before:.4f} -> {after:.5f}; pairs {out[0]['n_pairs'].tolist()}, pivot {out[0]['pivot'].tolist()}")
    assert not out[-1]["empty"][0] and out[0]["pivot"][0] >= PIVOT and after < before / 10


def test_a_table_without_gaussians_is_empty():
    rng = np.random.default_rng(6)
    sparse = rng.uniform(0, 100, (200, 3)).astype(np.float32)        # about one row per voxel of step 4
    tab = ndt_ref.table(sparse, 4.0, 6)
    assert tab["n_voxels"] > 100 and len(tab["cells"]) == 0
    got = ndt_ref.step(sparse, tab, np.eye(4)[None], 7)
    assert got["empty"].tolist() == [True] and got["n_pairs"].tolist() == [0] and got["sum_e"].tolist() == [0.0] and not got["T_out"].any()
    assert len(ndt_ref.table(np.zeros((0, 3)), 4.0)["cells"]) == 0 and ndt_ref.table(np.full((5, 3), np.nan), 4.0)["n_voxels"] == 0
