"""The premises of tests/test_gpu_desc_branches.py that need no GPU: the scenes of tests/desc_scene_ref.py against the C oracle
and against their own construction.  Each of the seven grid subdivisions is picked by its scene, planted support sizes are
exact, the oracle's rows equal the brute-force support sizes, and the oracle's rows for the exact-arithmetic scenes do not
change when the cloud's rows are permuted (so a device that sums in another order owes the same bits)."""
import numpy as np
import pytest

import desc_scene_ref as D

GEO = (4.2e6, -3.9e6, 5.1e5)


@pytest.mark.parametrize("option, offset", [(k, (0.0, 0.0, 0.0)) for k in range(7)] + [(1, GEO), (5, GEO)])
def test_each_grid_scene_picks_its_subdivision_and_plants_its_supports(option, offset, oracle_c):
    pts, kp, opt, f = D.grid_scene(option, offset)
    g = f["grid"]
    assert g["option"] == option and g["f"] == D.SUBDIVISIONS[option] and g["cell"] == opt["R"]
    assert np.prod(g["n"]) <= D.MAX_CELLS
    if option in (2, 3):
        assert g["n"][0] == 1                                        # thin in x: one cell, whatever fx
    # the two clusters pin the box: its corners are the planned ones
    np.testing.assert_array_equal(f["lo"], np.asarray(offset))
    np.testing.assert_allclose(f["hi"] - f["lo"], D.GRID_EXTENTS[option], rtol=0, atol=1e-8)
    n, at = D.support_sizes(pts, kp, opt["R"])
    kind = np.array(f["kind"])
    assert (n[kind == "outside, over R"] == 0).all()
    assert (n[kind == "outside, under R"] >= 40).all() and (n[kind == "outside, under R"] < 121).all()
    assert (n[kind == "corner"] >= 121).all() and (at[kind == "corner"] == 1).all()
    assert (n[kind == "on a face"] >= 121).all()
    faces = np.array([k.startswith("face") for k in kind])
    assert faces.sum() >= 18 and (n[faces] >= 100).all()
    assert (n[kind == "generic"] >= 100).sum() >= 12
    # the keypoints called "face" sit on a cell face of the kernel's grid, their neighbours one ulp off it
    for c, k in zip(kp[faces], kind[faces]):
        hit = [a for a in (1, 2) for j in range(g["n"][a] + 1)
               if (c[a] if k == "face" else np.nextafter(c[a], np.inf if k == "face-ulp" else -np.inf)) == g["origin"][a] + j * g["h"][a]]
        assert hit, (c, k)
    # the oracle's row sums are the brute-force support sizes (the point AT a corner keypoint is in no bin)
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    want, alive = D.expected_row_sums(pts, kp, opt)
    np.testing.assert_array_equal(rfeat, kp[alive])
    np.testing.assert_array_equal(rdesc.sum(axis=1), want)
    assert alive.sum() >= 40


def test_grid_pick_follows_the_cell_growth():
    """a box too large for 65 536 cells of edge R grows the cell by 1.26 until it fits, then only (1, 1, 1) is left"""
    g = D.grid_pick([0, 0, 0], [60000.0, 40000.0, 30000.0], 3.5)
    assert g["option"] == 6 and g["cell"] > 3.5 and np.prod(g["n"]) <= D.MAX_CELLS
    steps = np.log(g["cell"] / 3.5) / np.log(1.26)
    assert abs(steps - round(steps)) < 1e-9
    assert D.grid_pick([0, 0, 0], [0, 0, 0], 3.5)["n"] == [1, 1, 1]


@pytest.mark.parametrize("align", [True, False])
def test_lattice_rows_do_not_depend_on_the_clouds_order(align, oracle_c):
    pts, kp, opt = D.lattice_scene()
    opt = dict(opt, ALIGN_POINTS=align)
    n, at = D.support_sizes(pts, kp, opt["R"])
    assert list(n) == [4913] * 3 and list(at) == [1, 1, 0]
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 3 and list(rdesc.sum(axis=1)) == [4912, 4912, 4913]
    for seed in range(1, 5):
        p2 = pts[np.random.default_rng(seed).permutation(len(pts))]
        f2, d2 = oracle_c.getSpacialHistogramDescriptors(p2, kp, opt)
        np.testing.assert_array_equal(d2, rdesc)
    # exact in single as well: MATLAB's single arithmetic finds the same supports and values
    for sm in (1, 2):
        f3, d3 = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt, single_mode=sm)
        np.testing.assert_array_equal(d3, rdesc)
    assert (pts.astype(np.float32) == pts).all() and (kp.astype(np.float32) == kp).all()
    # the premises in the coordinates: 289 points on the plane y = 0 of the first two keypoints, 17 on their z axis
    for c in kp[:2]:
        rel = pts - c
        assert (rel[:, 1] == 0).sum() == 289 > D.K_DEF and ((rel[:, 0] == 0) & (rel[:, 1] == 0)).sum() == 17
    assert ((pts - kp[0])[:, 0] == 0).sum() == 289                    # zero votes in x at the centre
    assert ((pts - kp[2]) == 0).sum() == 0                            # the third keypoint is off every lattice plane


@pytest.mark.parametrize("k", [0.85, 0.5])
def test_lattice_selection_without_alignment(k, oracle_c):
    """k < 1, ALIGN_POINTS off: ties at the K-th distance are cut by original index, so the kept set -- and the frame -- depends
    on the order; the histogram does not.  select_facts says which branches the selection takes."""
    pts, kp, opt = D.lattice_scene()
    opt = dict(opt, ALIGN_POINTS=False, k=k)
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 3
    for seed in range(1, 4):
        p2 = pts[np.random.default_rng(seed).permutation(len(pts))]
        np.testing.assert_array_equal(oracle_c.getSpacialHistogramDescriptors(p2, kp, opt)[1], rdesc)
    for c in kp:
        f = D.select_facts(pts - c, k)
        assert f["tie_rank"] and not f["bisect"] and f["m"] <= D.K_SMALL and 8 <= f["n_eq"] <= 48
        assert f["recount"] == (k == 0.5)                              # at k = 0.5 the tie group straddles a bin border


def test_shell_scene_collides_as_planned(oracle_c):
    pts, kp, opt, facts = D.shell_scene()
    assert [f["n"] for f in facts] == [320, 368, 208]
    assert facts[0]["all_equal"] and facts[0]["bisect"] and facts[0]["tie_rank"] and facts[0]["n_eq"] == 320
    assert not facts[1]["all_equal"] and facts[1]["bisect"] and facts[1]["recount"] and facts[1]["tie_rank"] and facts[1]["m"] == 320
    assert not facts[2]["bisect"] and not facts[2]["recount"] and facts[2]["tie_rank"] and facts[2]["m"] == 160
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 3 and list(rdesc.sum(axis=1)) == [320, 368, 208]
    for seed in range(1, 4):
        p2 = pts[np.random.default_rng(seed).permutation(len(pts))]
        np.testing.assert_array_equal(oracle_c.getSpacialHistogramDescriptors(p2, kp, opt)[1], rdesc)


def test_tie_order_scene_turns_on_which_ties_are_kept(oracle_c):
    pts, kp, opt = D.tie_order_scene()
    for c in kp:
        f = D.select_facts(pts[np.abs(pts - c).max(axis=1) < 3.4] - c, opt["k"])
        assert f["n"] == 340 and f["K"] == 260 and f["n_eq"] == 120 and f["tie_rank"] and not f["bisect"]
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    np.testing.assert_array_equal(rfeat, kp[:1])                       # the x-axis ties come first for keypoint 0 only
    assert rdesc.sum() == 340
    rfeat2, rdesc2 = oracle_c.getSpacialHistogramDescriptors(*D.tie_order_scene(reverse=True))
    np.testing.assert_array_equal(rfeat2, kp[1:])                      # the order alone decides
    assert rdesc2.sum() == 340


@pytest.mark.parametrize("n_dirs", [1, 12])
def test_radial_edge_scene_plants_all_three_cases(n_dirs, oracle_c):
    pts, kp, opt, f = D.radial_edge_scene(n_dirs)
    assert len(f["cases"]) == 10 and all(on > 0 and above > 0 and below > 0 for on, above, below in f["cases"])
    assert (f["planted"] <= D.K_DEF) == (n_dirs == 1)
    # the reference's own expressions: the planted norms are within 3 ulps of an edge, and all seven offsets occur
    e = D.radial_edges(opt["R"])
    d = D._norm(pts)
    near = np.abs(d[:, None] - e[None, 1:]) <= 4 * np.spacing(e[None, 1:])
    assert near.any(axis=1).sum() == f["planted"]
    offs = set(np.rint((d[:, None] - e[None, 1:])[near] / np.spacing(e[None, 1:] * np.ones_like(near))[near]).astype(int))
    assert {-1, 0, 1} <= offs
    n, at = D.support_sizes(pts, kp, opt["R"])
    assert n[0] == len(pts) - 4 * n_dirs                               # on R and above it: outside (dists < R)
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 1 and rdesc.sum() == n[0]
    # the oracle puts a point ON edge k into radial bin k + 1 and a point one ulp below into bin k
    per_r = rdesc[0].reshape(14, 7, 10).sum(axis=(0, 1))
    lr = np.searchsorted(e, d[d < opt["R"]], side="right")
    np.testing.assert_array_equal(per_r, np.bincount(lr, minlength=11)[1:])


def test_theta_edge_scene(oracle_c):
    pts, kp, opt, f = D.theta_edge_scene()
    assert f["planted"] == 96 <= D.K_DEF
    th = np.arccos(pts[:, 2] / D._norm(pts))
    t = D.theta_edges()
    rel = np.abs(th[:, None] / t[None, 1:7] - 1.0)
    assert ((rel > 5e-10) & (rel < 2e-9)).any(axis=1).sum() == 96 and (rel > 1e-12).all()
    assert (np.abs(pts[:, 1]) > 1e-3).all()
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 1 and rdesc.sum() == len(pts)
    per_t = rdesc[0].reshape(14, 7, 10).sum(axis=(0, 2))
    np.testing.assert_array_equal(per_t, np.bincount(np.searchsorted(t, th, side="right"), minlength=8)[1:])


def test_literal_scene(oracle_c):
    pts, kp, opt, f = D.literal_scene()
    assert ((pts[:, 1] == 0) | ((pts[:, 0] == 0) & (pts[:, 1] == 0))).sum() == f["literal"] == 26 <= D.K_DEF
    n, at = D.support_sizes(pts, kp, opt["R"])
    assert n[0] == len(pts) and at[0] == 1
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    assert len(rfeat) == 1 and rdesc.sum() == len(pts) - 1
    # atan2(0, 0) = 0: the points with y == 0 share the phi bin that holds 0
    per_p = rdesc[0].reshape(14, 7, 10).sum(axis=(1, 2))
    assert per_p[7] + per_p[6] >= 25 and np.count_nonzero(per_p) <= 4


def test_ball_scene_sizes_are_exact():
    sizes = [8190, 8191, 8192, 300, 4, 11]
    pts, kp = D.ball_scene(sizes)
    for R in (0.95 * D.R0, D.R0, 1.5 * D.R0):
        assert list(D.support_sizes(pts, kp, R)[0]) == sizes
