"""tests/fpfh_radius_ref.py held to known answers without a GPU: hand-worked cases, its long-double and plain-float forms against each
other, its equality with tests/fpfh_ref.py where the two neighbourhood rules coincide, and the share of rows every (family, radius,
max_neighbors) case of the GPU test excludes against fpfh_ref's cap of 1 %, established with the exact fp32 lists."""
import numpy as np
import pytest

import fpfh_radius_ref as ref
import fpfh_ref

UP = np.array([0.0, 0.0, 1.0], np.float32)


def _one_bin(out):
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    return (np.asarray(out, np.float64) == want[None, :]).all()


def test_hand_worked_four_points():
    """fpfh_ref's hand-worked case ((0,0,0), (2,0,0), (0,2,0), (0,0,1), every normal (0,0,1)) with a radius that covers the cloud is
    that case: counts, m = 2, 3, 3, 2, row 0's f3 = 200/3, 200/9, 100/9 at bins 3, 5, 7 and row 3's 1900/21, 200/21 at bins 5, 7.
    With r2 = 4 row 3 (at squared distance 5 from rows 1, 2) keeps row 0 only, a pair along the normal: m_3 = 0, its FPFH is row 0's
    SPFH -- 100 at 5, 16, 27 -- and rows 1, 2 lose row 3 and each other (squared distance 8).  max_neighbors = 1 keeps the nearest
    neighbour only: row 0 keeps row 3 (no contribution), rows 1, 2 keep row 0, row 3 keeps row 0."""
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1]], np.float32)
    nrm = np.tile(UP, (4, 1))
    r = ref.fpfh(pts, nrm, 100.0)
    want = np.zeros((4, 33), np.int64)
    want[0, [5, 16, 27]] = 2
    want[1, [5, 16]] = 3; want[1, 27] = 2; want[1, 29] = 1
    want[2] = want[1]
    want[3, [5, 16, 25]] = 2
    assert np.array_equal(r["counts"], want) and list(r["m"]) == [2, 3, 3, 2] and list(r["n"]) == [3, 3, 3, 3]
    assert not r["sensitive"].any()
    out = np.asarray(r["out"], np.float64)
    w0 = np.zeros(11); w0[3], w0[5], w0[7] = 200 / 3, 200 / 9, 100 / 9
    w3 = np.zeros(11); w3[5], w3[7] = 1900 / 21, 200 / 21
    tol = ref.out_tol(3)
    assert np.abs(out[0, 22:] - w0).max() <= tol and np.abs(out[3, 22:] - w3).max() <= tol
    counts, pout = ref.plain_double(pts, nrm, 100.0)
    assert np.array_equal(counts, want) and np.abs(pout - out).max() <= tol
    # r2 = 4 (inclusive): rows 1, 2 are in row 0's neighbourhood, row 3 keeps row 0 only
    r = ref.fpfh(pts, nrm, 4.0)
    assert list(r["n"]) == [3, 1, 1, 1] and list(r["m"]) == [2, 1, 1, 0]
    assert _one_bin(r["out"][[1, 2, 3]])
    assert np.array_equal(ref.plain_double(pts, nrm, 4.0)[0], r["counts"])
    # the nearest neighbour only
    r = ref.fpfh(pts, nrm, 100.0, 1)
    assert list(r["n"]) == [1, 1, 1, 1] and list(r["m"]) == [0, 1, 1, 0] and list(r["idx"][:, 0]) == [3, 0, 0, 0]
    assert (r["out"][[0, 3]] == 0).all() and (r["out"][[1, 2]] == 0).all()           # row 0's SPFH is empty, so nothing is added anywhere


@pytest.mark.parametrize("radius,n", [(1.5, 2), (3.0, 4), (4.6, 6)])
def test_rows_on_a_line(radius, n):
    """40 rows 1.5 apart with the normal across the line: every pair lands in bins 5, 16, 27; an inner row has n rows inside"""
    pts = np.column_stack([np.arange(40, dtype=np.float32) * 1.5 + 3, np.full(40, 2, np.float32), np.full(40, -1, np.float32)])
    r = ref.fpfh(pts, np.tile(UP, (40, 1)), ref.r2_of(radius))
    assert (r["n"][n // 2:40 - n // 2] == n).all() and r["n"][0] == n // 2 and not r["excluded"].any()
    assert (r["m"] == r["n"]).all() and _one_bin(r["out"])
    counts, out = ref.plain_double(pts, np.tile(UP, (40, 1)), ref.r2_of(radius))
    assert np.array_equal(counts, r["counts"]) and _one_bin(out)
    r1 = ref.fpfh(pts, np.tile(UP, (40, 1)), ref.r2_of(radius), 1)
    assert (r1["n"] == 1).all() and _one_bin(r1["out"])


def test_lattice_in_a_plane():
    """32 x 32 integer lattice in z = 7: r2 = 2 holds the 8 surrounding rows of an inner row, r2 = 1 its 4; 100 at 5, 16, 27"""
    g = np.arange(32, dtype=np.float32)
    pts = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    inner = ((pts[:, 0] > 0) & (pts[:, 0] < 31) & (pts[:, 1] > 0) & (pts[:, 1] < 31))
    for r2, n in ((1.0, 4), (2.0, 8), (4.0, 12)):
        r = ref.fpfh(pts, np.tile(UP, (1024, 1)), r2)
        assert (r["n"][(pts[:, 0] > 1) & (pts[:, 0] < 30) & (pts[:, 1] > 1) & (pts[:, 1] < 30)] == n).all() and r["n"][0] == {4: 2, 8: 3, 12: 5}[n]
        assert (r["m"] == r["n"]).all() and not r["excluded"].any() and _one_bin(r["out"])
    r = ref.fpfh(pts, np.tile(UP, (1024, 1)), 2.0, 5)
    assert (r["n"][inner] == 5).all() and (r["d2"][inner, :4] == 1).all() and (r["d2"][inner, 4] == 2).all()
    # ties at the window's end go to the lowest row: the fifth neighbour of an inner row is (x - 1, y - 1)
    assert (r["idx"][inner, 4] == np.flatnonzero(inner) - 33).all()


def test_rows_without_a_descriptor():
    same = np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (5, 1))
    r = ref.fpfh(same, np.tile(UP, (5, 1)), 9.0)
    assert (r["out"] == 0).all() and (r["counts"] == 0).all() and (r["n"] == 0).all()
    model, nrm = fpfh_ref.family_inputs("sheet")
    model, nrm = model[:300].copy(), nrm[:300].copy()
    model[7, 1] = np.nan
    model[9, 0] = np.inf
    nrm[11] = np.nan
    for r2 in (ref.r2_of(6.0), np.float32(np.inf)):
        r = ref.fpfh(model, nrm, r2)
        assert np.isnan(r["out"][[7, 9]]).all() and not np.isnan(np.delete(r["out"], [7, 9], axis=0)).any()
        assert (r["counts"][[7, 9, 11]] == 0).all() and (r["n"][[7, 9]] == 0).all() and r["out"][11].sum() > 299.0
        assert not (r["nb"] & ((r["idx"] == 7) | (r["idx"] == 9))).any()
    assert (ref.fpfh(model, nrm, 0.0)["out"][[0, 5]] == 0).all()


@pytest.mark.parametrize("k", [4, 9, 32])
def test_equals_the_k_nearest_reference_where_the_rules_coincide(k):
    """a radius that covers the cloud, no coincident rows, max_neighbors = k - 1: fpfh_ref.fpfh(model, normals, k)"""
    model, nrm = fpfh_ref.family_inputs("volume")
    model, nrm = model[:300], nrm[:300]
    assert len(np.unique(model, axis=0)) == 300
    want = fpfh_ref.fpfh(model, nrm, k)
    kidx, kd2, knb = fpfh_ref.neighbours(model, k)
    assert knb[:, 1:].all() and not knb[:, 0].any()
    r = ref.fpfh(model, nrm, np.float32(np.inf), k - 1)
    assert np.array_equal(r["idx"], kidx[:, 1:]) and np.array_equal(r["d2"], kd2[:, 1:]) and r["nb"].all()
    assert np.array_equal(r["counts"], want["counts"]) and np.array_equal(r["m"], want["m"])
    assert np.array_equal(r["out"], want["out"]) and np.array_equal(r["excluded"], want["excluded"])


def test_long_double_and_plain_float_forms_agree():
    model, nrm = fpfh_ref.family_inputs("sheet")
    model, nrm = model[:400], nrm[:400]
    for r2, n in ((ref.r2_of(9.0), 0), (ref.r2_of(20.0), 50)):
        r = ref.fpfh(model, nrm, r2, n)
        counts, out = ref.plain_double(model, nrm, r2, n)
        cmp = ~r["excluded"]
        assert cmp.mean() >= 0.99 and np.array_equal(counts[cmp], r["counts"][cmp])
        n_max = int(r["n"].max())
        err = float(np.abs(out[cmp] - np.asarray(r["out"], np.float64)[cmp]).max())
        print(f"sheet[:400] r2 = {float(r2):g} n = {n}: n_max {n_max}, plain double at most {err:.2e} from the reference (bound {ref.out_tol(n_max):.2e})")
        assert n_max > 31 and err <= ref.out_tol(n_max)


@pytest.mark.parametrize("max_neighbors", ref.MAX_NEIGHBORS)
@pytest.mark.parametrize("name,radius", ref.CASES)
def test_excluded_share_of_the_family_cases(name, radius, max_neighbors):
    r = ref.case(name, radius, max_neighbors)
    share = ref.excluded_share(r)
    print(f"{name} radius {radius:g} max_neighbors {max_neighbors}: neighbourhoods {int(r['n'].min())}-{int(r['n'].max())}, largest count "
          f"{int(r['counts'].max())}, sensitive {100 * r['sensitive'].mean():.2f} %, excluded {100 * share:.2f} %")
    assert share <= ref.EXCLUDED_CAP
    if max_neighbors:
        assert int(r["n"].max()) <= max_neighbors
    s = np.asarray(r["out"], np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.abs(s - 100.0).max() <= 1e-10
