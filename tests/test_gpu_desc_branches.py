"""The rarely taken branches of desc_kernel (pcreg_amd/csrc/descriptors.hip) against the oracle, bit for bit, on scenes built to
reach them (tests/desc_scene_ref.py; their host premises are checked without a GPU by tests/test_desc_scene_ref.py).  Every
test also asserts, through the "desc_stats" counters, that the kernel went the way the scene was built for: an equality that
holds because the fast screen succeeded proves nothing about the path behind it.

While "desc_stats" is on, the library runs the instantiation of desc_kernel that holds the counting code; the default one holds
none (the kernel has no register to spare).  Both come from the same source and the scenes are deterministic, so they take the
same branches: every scene is therefore described twice, key off (the kernel everybody runs) and key on (the one that says which
way it went), and both results are compared with the oracle."""
import ctypes as C

import numpy as np
import pytest

import desc_scene_ref as D
from desc_scene_ref import BISECT, DEFERRED, LITERAL, REBIN, RECOUNT, RETEST, SELECT, SUBDIV, TIE_RANK, VOTE64

pytestmark = pytest.mark.gpu

GEO = (4.2e6, -3.9e6, 5.1e5)


def _stats(reset=1):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 10)()
    check(lib().pcreg_debug_desc_stats(out, reset))
    return [int(v) for v in out]


@pytest.fixture
def stats_on(debug_set):
    """"desc_stats" on and the counters cleared; the fixture's value reads (and clears) them"""
    debug_set("desc_stats", 1)
    _stats(1)
    return _stats


def _off_then_on(run):
    """run() with the key off (the default instantiation; the counters must not move) and then on (the counting one)"""
    from pcreg_amd._lib import check, lib
    before = _stats(0)
    check(lib().pcreg_debug_set(b"desc_stats", 0))
    try:
        run()
        assert _stats(0) == before, "the counters moved while desc_stats was off"
    finally:
        check(lib().pcreg_debug_set(b"desc_stats", 1))
    run()


def _equal_to_oracle(pts, kp, opt, oracle_c, single_mode=0):
    import pcreg_amd as pc
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(np.asarray(pts, np.float64), np.asarray(kp, np.float64), opt, single_mode=single_mode)

    def run():
        feat, desc = pc.getSpacialHistogramDescriptors(pts, kp, opt)
        np.testing.assert_array_equal(feat, rfeat)
        np.testing.assert_array_equal(desc, rdesc)
        assert desc.shape[1] == 980
    _off_then_on(run)
    return rfeat, rdesc


def _soa(a):
    import torch
    from pcreg_amd.device import soa
    return soa(torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(torch.device("cuda", 0)))


# ---- the contrast: what the ordinary scenes reach -------------------------------------------------------------------------
def test_ordinary_strips_reach_none_of_the_rare_branches(stats_on, oracle_c):
    """The scene of tests/test_gpu_descriptors.py: the finest subdivision, every screen succeeds.  (With the key off the counters
    do not move: _off_then_on asserts that for every scene of this file.)"""
    from test_gpu_descriptors import OPT, keypoints, strips
    pts, kp = strips(40000, 0), keypoints(300, 1)
    rfeat, rdesc = _equal_to_oracle(pts, kp, OPT, oracle_c)
    st = stats_on()
    assert st[SELECT] >= len(rfeat) > 50
    for word, name in ((BISECT, "bisection"), (RECOUNT, "full recount"), (TIE_RANK, "tie rank"), (VOTE64, "fp64 votes"), (REBIN, "literal re-bin"),
                       (LITERAL, "literal bins"), (RETEST, "re-tested chunks")):
        assert st[word] == 0, f"the strips scene took the {name} branch {st[word]} times"
    assert st[SUBDIV] == D.subdiv_word((4, 2, 2))


def test_chunks_past_the_kept_ballots_are_counted(stats_on, oracle_c):
    """the scene of test_more_candidate_chunks_than_the_kept_ballots: a coarse grid, rows of > 4 x 192 chunks"""
    rng = np.random.default_rng(77)
    n = 100000
    x = rng.uniform(0, 150, n); y = rng.uniform(-1.2, 1.2, n); z = 10 + 0.05 * x + rng.normal(0, 0.2, n)
    pts = np.vstack([np.column_stack([x, y, z]), [[30000.0, 20000.0, 15000.0], [-30000.0, -20000.0, -15000.0]]])
    kx = rng.uniform(5, 145, 12)
    kp = np.column_stack([kx, rng.uniform(-0.8, 0.8, 12), 10 + 0.05 * kx])
    opt = dict(min_pts=100, max_pts=8000, R=3.5, thVar=[3, 1.5], k=0.85, ALIGN_POINTS=True, VERBOSE=0)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    st = stats_on()
    assert len(rfeat) >= 6
    assert st[RETEST] > 0, "no chunk was re-tested: the rows were meant to hold more than 4 x 192 chunks"
    assert st[SUBDIV] == D.subdiv_word((1, 1, 1))


# ---- a. every grid subdivision ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option, offset", [(k, (0.0, 0.0, 0.0)) for k in range(7)] + [(1, GEO), (5, GEO)])
def test_every_grid_subdivision(option, offset, stats_on, oracle_c):
    """Keypoints on cell faces (and an ulp off them), at the box's corners and faces, just inside and just outside its reach: a
    row cut that is too tight drops a support point, and with thVar = [1, 1] every lost point shows in a row sum."""
    pts, kp, opt, f = D.grid_scene(option, offset)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    st = stats_on()
    want, alive = D.expected_row_sums(pts, kp, opt)
    assert st[SUBDIV] == f["subdiv"], f"the scene was built for subdivision {D.SUBDIVISIONS[option]}, the grid took {st[SUBDIV]:#x}"
    assert st[SELECT] == alive.sum(), "every keypoint inside the size gates reaches the selection"
    np.testing.assert_array_equal(rfeat, kp[alive])
    np.testing.assert_array_equal(rdesc.sum(axis=1), want)
    kind = np.array(f["kind"])
    assert not alive[kind == "outside, over R"].any() and alive[kind == "outside, under R"].all() and alive[kind == "corner"].all()


# ---- b. the exact lattice ------------------------------------------------------------------------------------------------
def _lattice_premises(st, align, n_calls=1):
    assert st[SELECT] == 3 * n_calls
    assert st[REBIN] >= 2 * n_calls, f"289 points with y == 0 were meant to send two keypoints to the literal re-bin, {st[REBIN]} went"
    assert st[LITERAL] >= 2 * 289 * n_calls, f"the points with y == 0 (17 of them on the z axis, one at the keypoint) were meant to reach bin_literal, {st[LITERAL]} did"
    if align:
        assert st[VOTE64] == 3 * n_calls, f"289 kept points with a zero vote were meant to send every keypoint to the fp64 votes, {st[VOTE64]} went"
    else:
        assert st[VOTE64] == 0


@pytest.mark.parametrize("align", [True, False])
def test_lattice_all_points_kept(align, stats_on, oracle_c):
    """Every sum is exact in any order, so the device owes the oracle's bits although it sums in another order."""
    pts, kp, opt = D.lattice_scene()
    opt = dict(opt, ALIGN_POINTS=align)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert list(rdesc.sum(axis=1)) == [4912, 4912, 4913]              # the point AT a keypoint is in the support and in no bin
    _lattice_premises(stats_on(), align)


@pytest.mark.parametrize("k", [0.85, 0.5])
def test_lattice_selection_ties(k, stats_on, oracle_c):
    """k < 1 without alignment (with it the kept set is cut by index, the frame tilts, and the exact zeros become rounding noise
    on which device and oracle may differ): tie groups of up to 48 at the K-th distance are kept in part, by original index; at
    k = 0.5 the group straddles a border of the selection's histogram.  (The lattice never crowds a bin beyond 256 keys: the
    bisection is the shell scene's.)"""
    pts, kp, opt = D.lattice_scene()
    opt = dict(opt, ALIGN_POINTS=False, k=k)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert len(rfeat) == 3
    st = stats_on()
    facts = [D.select_facts(pts - c, k) for c in kp]
    assert st[TIE_RANK] == sum(f["tie_rank"] for f in facts) == 3, f"three tie groups were meant to be ranked by original index, {st[TIE_RANK]} were"
    assert st[RECOUNT] == sum(f["recount"] for f in facts) == (3 if k == 0.5 else 0), f"full recounts: {st[RECOUNT]}"
    assert st[BISECT] == 0


def test_shells_of_equal_distances(stats_on, oracle_c):
    """dhi == dlo (scale = 0: 320 equal keys), a bin crowded by 320 keys inside a range (the bisection iterates), and a shell
    of 160 (ranked directly); each tie group is kept in part."""
    pts, kp, opt, facts = D.shell_scene()
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert list(rdesc.sum(axis=1)) == [320, 368, 208]
    st = stats_on()
    assert st[SELECT] == 3
    assert st[BISECT] == sum(f["bisect"] for f in facts) == 2, f"two crowded bins were meant to take the bisection, {st[BISECT]} did"
    assert st[TIE_RANK] == 3, f"three tie groups were meant to be ranked by original index, {st[TIE_RANK]} were"
    assert st[RECOUNT] == sum(f["recount"] for f in facts) == 2, f"full recounts: {st[RECOUNT]}"


@pytest.mark.parametrize("reverse", [False, True])
def test_tie_groups_keep_the_lowest_original_indices(reverse, stats_on, oracle_c):
    """Half of a tie group of 120 is kept; which half decides whether the kept set passes thVar.  (Without alignment and with
    thVar = [1, 1], as in the scenes above, the choice would not show in any count.)"""
    pts, kp, opt = D.tie_order_scene(reverse)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    np.testing.assert_array_equal(rfeat, kp[1:] if reverse else kp[:1])
    st = stats_on()
    assert st[SELECT] == 2 and st[TIE_RANK] == 2, f"two tie groups were meant to be ranked by original index, {st[TIE_RANK]} were"


def test_lattice_through_the_device_tier_u16_rows(stats_on, oracle_c):
    """DescriptorPipeline.describe(compact=True): the re-binned rows leave through the u16 store loop of the literal path"""
    import torch
    from pcreg_amd.device import DescriptorPipeline
    pts, kp, opt = D.lattice_scene()
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    dp = DescriptorPipeline(torch.device("cuda", 0))

    def run():
        feat, rows, V = dp.describe(_soa(pts), _soa(kp), opt, compact=True)
        assert V == len(rfeat) == 3
        np.testing.assert_array_equal(feat[:V].cpu().numpy(), rfeat)
        np.testing.assert_array_equal(rows.compact(V).cpu().numpy().astype(np.float64), rdesc)
    _off_then_on(run)
    _lattice_premises(stats_on(), True)


@pytest.mark.parametrize("mode", [1, 2])
def test_lattice_in_single_arithmetic(mode, stats_on, oracle_c):
    """The lattice is exact in single: the single-arithmetic instantiation finds the same supports and values, so its rows equal
    the oracle's single_mode rows AND the double ones."""
    pts, kp, opt = D.lattice_scene()
    p32, k32 = pts.astype(np.float32), kp.astype(np.float32) if mode == 1 else kp
    rfeat, rdesc = _equal_to_oracle(p32, k32, opt, oracle_c, single_mode=mode)
    dfeat, ddesc = oracle_c.getSpacialHistogramDescriptors(pts, kp, opt)
    np.testing.assert_array_equal(rdesc, ddesc)
    _lattice_premises(stats_on(), True)


# ---- c. planted bin edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dirs", [1, 12])
def test_points_within_ulps_of_the_radial_edges(n_dirs, stats_on, oracle_c):
    """sqrt(d2) on each radial edge and 1..3 ulps to either side: the squared images r2ge / r2gt must put every one of them
    where sqrt + histcounts does.  One direction: at most 128 deferred points, binned one by one; twelve: the whole support is
    binned again in fp64."""
    pts, kp, opt, f = D.radial_edge_scene(n_dirs)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    n, at = D.support_sizes(pts, kp, opt["R"])
    assert len(rfeat) == 1 and rdesc.sum() == n[0] == len(pts) - 4 * n_dirs
    st = stats_on()
    inside = f["planted"] - 4 * n_dirs
    if n_dirs == 1:
        assert st[REBIN] == 0 and st[DEFERRED] >= inside, f"{inside} planted points were meant to be deferred one by one, {st[DEFERRED]} were"
    else:
        assert st[REBIN] == 1, f"{inside} planted points were meant to exceed the deferred list, re-bins: {st[REBIN]}"
    assert st[LITERAL] == 0, "generic directions: the fp64 images decide, not sqrt / acos"


def test_points_beside_the_theta_edges(stats_on, oracle_c):
    """relative offsets of 1e-9 from each theta edge: deferred by the fp32 screen, decided by the exact images cts"""
    pts, kp, opt, f = D.theta_edge_scene()
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert len(rfeat) == 1 and rdesc.sum() == len(pts)
    st = stats_on()
    assert st[DEFERRED] >= f["planted"] and st[REBIN] == 0, f"96 planted points were meant to be deferred, {st[DEFERRED]} were (re-bins {st[REBIN]})"
    assert st[LITERAL] == 0, f"{st[LITERAL]} points took the literal path: 1e-9 is outside the 1e-12 band"


def test_a_few_points_on_the_frames_planes_and_axis(stats_on, oracle_c):
    """20 points with y == 0, 5 on the z axis, one at the keypoint: at most 128 deferred points, none of which the fp64 images
    can decide -- each takes sqrt / acos / atan2(y, y) as the reference does."""
    pts, kp, opt, f = D.literal_scene()
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert len(rfeat) == 1 and rdesc.sum() == len(pts) - 1              # the point at the keypoint is in no bin
    st = stats_on()
    assert st[REBIN] == 0 and st[DEFERRED] >= f["literal"]
    assert st[LITERAL] == f["literal"] == 26, f"26 planted points were meant to reach bin_literal, {st[LITERAL]} did"


# ---- d. capacity and size gates ------------------------------------------------------------------------------------------
BALL_OPT = dict(min_pts=100, max_pts=100000, R=D.R0, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=True, VERBOSE=0)


@pytest.mark.parametrize("k", [0.85, "all"])
def test_supports_of_8190_and_8191_points(k, stats_on, oracle_c):
    """the LDS list holds 8191 entries: 32 per thread, the last bit of selmask and the last slot of kreg"""
    pts, kp = D.ball_scene([8190, 8191])
    opt = dict(BALL_OPT, k=k)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    assert list(rdesc.sum(axis=1)) == [8190, 8191]
    assert stats_on()[SELECT] == 2


def test_a_support_of_8192_points_is_refused(stats_on, oracle_c):
    import torch
    import pcreg_amd as pc
    from pcreg_amd._lib import PCREG_E_ARG, PcregError
    from pcreg_amd.device import DescriptorPipeline
    pts, kp = D.ball_scene([300, 8192, 5000])
    assert list(D.support_sizes(pts, kp, D.R0)[0]) == [300, 8192, 5000]
    rfeat, rdesc = oracle_c.getSpacialHistogramDescriptors(pts, kp[[0, 2]], BALL_OPT)
    dp = DescriptorPipeline(torch.device("cuda", 0))

    def run():
        with pytest.raises(PcregError, match="8192") as e:
            pc.getSpacialHistogramDescriptors(pts, kp, BALL_OPT)
        assert e.value.code == PCREG_E_ARG
        # device tier: the flag carries the count, the other keypoints of the call are described all the same
        feat, rows, counters = dp.describe_async(_soa(pts), _soa(kp), BALL_OPT, compact=True)
        V, over = (int(v) for v in counters.cpu())
        assert over == 8192 and V == 2
        np.testing.assert_array_equal(feat[:V].cpu().numpy(), rfeat)
        np.testing.assert_array_equal(rows.compact(V).cpu().numpy().astype(np.float64), rdesc)
    _off_then_on(run)
    assert stats_on()[SELECT] == 4                                     # two counting calls, two keypoints each


@pytest.mark.parametrize("sizes, min_pts, max_pts, survive", [([8191, 300], 100, 8190, [1]), ([299, 300, 301], 100, 300, [0, 1]),
                                                              ([4, 5, 10, 11], 5, 10, [1, 2])])
def test_supports_at_the_size_gates(sizes, min_pts, max_pts, survive, stats_on, oracle_c):
    """n == max_pts and n == min_pts pass, max_pts + 1 and min_pts - 1 do not; max_pts = 10 is under the list's floor of 64"""
    pts, kp = D.ball_scene(sizes)
    opt = dict(BALL_OPT, min_pts=min_pts, max_pts=max_pts)
    rfeat, rdesc = _equal_to_oracle(pts, kp, opt, oracle_c)
    np.testing.assert_array_equal(rfeat, kp[survive])
    assert list(rdesc.sum(axis=1)) == [sizes[i] for i in survive]
    assert stats_on()[SELECT] == len(survive)
