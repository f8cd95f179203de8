"""tests/iss_ref.py against the contract of pcreg_model_iss_f32, without a GPU: the share of rows the GPU test may not compare, the
exact zeros of planar and collinear clouds, a case worked by hand, exact ties on a lattice, and the quantisation bound."""
import functools

import numpy as np
import pytest

import iss_ref as ref

L = np.longdouble


@functools.lru_cache(maxsize=None)
def _case(name, rs, rn, quantised=True):
    return ref.case(name, rs, rn, quantised)


@pytest.mark.parametrize("name,rs,rn", ref.cases())
def test_excluded_share_is_under_the_cap(name, rs, rn):
    r = _case(name, rs, rn)
    share = r["excluded"].mean()
    live = r["n"] >= ref.MIN_NEIGHBORS
    print(f"{name} r = ({rs}, {rn}): {int(r['excluded'].sum())} of {len(r['n'])} rows excluded ({100 * share:.2f} %), "
          f"{int(r['sensitive'].sum())} sensitive, {int(r['cand'].sum())} candidates, {len(r['keypoints'])} keypoints, "
          f"n in {int(r['n'].min())}..{int(r['n'].max())}, {int(live.sum())} rows with n >= {ref.MIN_NEIGHBORS}")
    assert share <= ref.EXCLUDED_CAP
    assert len(r["keypoints"]) >= 10 and r["n"].min() >= 1


def test_fmaf_chain_is_the_c_chain():
    """the float64 route of iss_ref._fmaf against the fp32 k-nearest reference's compiled fmaf chain"""
    import knn_k_ref
    m = ref.family("volume")[:300]
    idx, d = knn_k_ref.knn(m, m, 300)
    D = ref.d2_matrix(m)
    assert np.array_equal(np.sort(D, axis=1).view(np.uint32), d.view(np.uint32))


def test_plane_and_line_have_exact_zeros_and_no_keypoint():
    r = ref.iss(ref.lattice_plane(), ref.r2_of(3.0), ref.r2_of(2.0))
    assert (r["mu"][:, 2] == 0).all() and (r["mu"][:, 0] > 0).all() and (r["N"][:, [2, 4, 5]] == 0).all()
    assert not r["cand"].any() and len(r["keypoints"]) == 0 and not r["sensitive"].any()
    line = np.column_stack([np.arange(40, dtype=np.float32) * 0.5 + 3, np.full(40, 5, np.float32), np.full(40, -2, np.float32)])
    r = ref.iss(line, ref.r2_of(3.0), ref.r2_of(2.0))
    assert (r["mu"][:, 1:] == 0).all() and (r["mu"][:, 0] > 0).all() and r["n"].max() == 13
    assert not r["cand"].any() and len(r["keypoints"]) == 0 and not r["sensitive"].any()


def test_hand_worked_eight_points():
    """Rows 0 .. 6: the origin and (+-1.5, 0, 0), (0, +-1, 0), (0, 0, +-0.5), moved by (8, 16, 4); row 7 far away.  r2_salient = 4:
    e2 = 3, e = 2, q = 2^16 dx.  Rows 0, 3, 4, 5, 6 see all seven: sum x^2 = 4.5, y^2 = 2, z^2 = 0.5 about the mean, so
    N = 7 diag(4.5, 2, 0.5) 2^32 = diag(31.5, 14, 3.5) 2^32 and lambda = (31.5, 14, 3.5) / 49.  Rows 1 and 2 do not see each other
    (distance 3): n = 6, S1 = (-+7.5, 0, 0) 2^16, S2 = diag(11.25, 2, 0.5) 2^32, N = diag(11.25, 12, 3) 2^32, lambda = (12, 11.25, 3) / 36.
    Row 7: n = 1, N = 0."""
    pts = ref.hand_case()
    r = ref.iss(pts, 4.0, 9.0, 0.975, 0.975, 5)
    assert r["e"] == 2 and list(r["n"]) == [7, 6, 6, 7, 7, 7, 7, 1]
    two32 = 2.0 ** 32
    for i in (0, 3, 4, 5, 6):
        assert np.array_equal(r["N"][i], np.array([31.5, 0, 0, 14, 0, 3.5]) * two32)
        assert np.array_equal(r["lam"][i], np.array([31.5, 14, 3.5], L) / L(49))
    for i in (1, 2):
        assert np.array_equal(r["N"][i], np.array([11.25, 0, 0, 12, 0, 3]) * two32)
        assert np.array_equal(r["lam"][i], np.array([12, 11.25, 3], L) / L(36))
    assert not r["N"][7].any() and list(r["cand"]) == [True] * 7 + [False]
    # radius 3 (inclusive: rows 1 and 2 are exactly 3 apart): rows 1 and 2 tie at 3 / 36 > 3.5 / 49, the lower row wins
    assert list(r["keypoints"]) == [1] and not r["sensitive"].any()
    # a tiny nonmax radius: every candidate is a keypoint
    assert list(ref.iss(pts, 4.0, 0.01, 0.975, 0.975, 5)["keypoints"]) == [0, 1, 2, 3, 4, 5, 6]
    # seven neighbours asked for: rows 0, 3, 4, 5, 6 tie exactly, row 0 wins
    r7 = ref.iss(pts, 4.0, 9.0, 0.975, 0.975, 7)
    assert list(r7["cand"]) == [True, False, False, True, True, True, True, False] and list(r7["keypoints"]) == [0]
    assert list(ref.keypoints_of(pts, r7["s"].astype(np.float64), 9.0)) == [0]
    assert len(ref.iss(pts, 4.0, 9.0, 0.975, 0.975, 8)["keypoints"]) == 0


def test_cube_lattice_ties_go_to_the_lowest_row():
    """9 x 9 x 9 unit lattice, r2 = 1: an interior row has its six axis neighbours, N = diag(14, 14, 14) 2^34 exactly; with
    min_neighbors = 7 and thresholds of 2 exactly the 343 interior rows are candidates, all tied; the keypoints are the interior
    rows without an interior axis neighbour of a lower row number"""
    pts, interior = ref.lattice_cube()
    r = ref.iss(pts, 1.0, 1.0, 2.0, 2.0, 7)
    assert r["e"] == 1 and np.array_equal(r["cand"], interior) and interior.sum() == 343
    assert (r["N"][interior] == np.array([14, 0, 0, 14, 0, 14]) * 2.0 ** 34).all()
    assert (r["s"][interior] == L(2) / L(7)).all() and not r["sensitive"].any()
    where = {tuple(int(v) for v in p): i for i, p in enumerate(pts)}
    want = []
    for i in np.flatnonzero(interior):
        x, y, z = (int(v) for v in pts[i])
        nb = [where.get(c) for c in ((x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1), (x, y, z + 1))]
        if not any(j is not None and interior[j] and j < i for j in nb):
            want.append(i)
    assert list(r["keypoints"]) == want and 20 < len(want) < 343


@pytest.mark.parametrize("name,rs,rn", ref.cases())
def test_quantisation_moves_eigenvalues_within_the_bound(name, rs, rn):
    a, b = _case(name, rs, rn), _case(name, rs, rn, False)
    bound = ref.quantisation_bound(ref.r2_of(rs))
    err = np.abs(a["lam"] - b["lam"]).astype(np.float64)
    print(f"{name} r = ({rs}, {rn}): worst |lambda - lambda_unq| = {err.max():.3e} = {err.max() / float(ref.r2_of(rs)):.2e} r^2, "
          f"{err.max() / bound:.3e} of the bound; keypoints equal: {np.array_equal(a['keypoints'], b['keypoints'])}")
    assert (err <= bound).all()
    assert np.array_equal(a["n"], b["n"])
