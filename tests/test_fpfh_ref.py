"""tests/fpfh_ref.py held to known answers without a GPU, a plain-double restatement of the contract against it on the families the
GPU test uses, and the share of rows every (family, k) excludes against the cap of 1 %."""
import numpy as np
import pytest

import fpfh_ref as ref

UP = np.array([0.0, 0.0, 1.0], np.float32)


def _one_bin(out):
    """every row exactly 100 at places 5, 16, 27 and 0 elsewhere"""
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    return (np.asarray(out, np.float64) == want[None, :]).all()


@pytest.mark.parametrize("k", [3, 8])
def test_rows_on_a_line(k):
    pts = np.column_stack([np.arange(40, dtype=np.float32) * 1.5 + 3, np.full(40, 2, np.float32), np.full(40, -1, np.float32)])
    r = ref.fpfh(pts, np.tile(UP, (40, 1)), k)
    assert (r["m"] == k - 1).all() and not r["excluded"].any()
    assert _one_bin(r["out"])
    counts, out = ref.plain_double(pts, np.tile(UP, (40, 1)), k)
    assert np.array_equal(counts, r["counts"]) and _one_bin(out)


@pytest.mark.parametrize("k", [4, 5, 9])
def test_lattice_in_a_plane(k):
    g = np.arange(32, dtype=np.float32)
    pts = np.column_stack([np.repeat(g, 32), np.tile(g, 32), np.full(1024, 7, np.float32)])
    r = ref.fpfh(pts, np.tile(UP, (1024, 1)), k)
    assert (r["m"] == k - 1).all() and not r["excluded"].any()
    assert _one_bin(r["out"])


def test_hand_worked_four_points():
    """(0,0,0), (2,0,0), (0,2,0), (0,0,1), every normal (0,0,1), k = 4.  Equal normals: a_i = a_j = dz / len, a tie, the source is i;
    v = d x n = (dy, -dx, 0) / vl, w . nt = 0 and v . nt = 0, so f1 = f2 = 0 (bin 5) and f3 = dz / len.  The pair of rows 0 and 3
    has d along the normal: vl = 0, no contribution.  Row 0: rows 1, 2 at f3 = 0 (bin 5).  Rows 1, 2: row 0 and each other at
    f3 = 0, row 3 at f3 = 1 / sqrt(5): 11 (1.4472 / 2) = 7.96, bin 7.  Row 3: rows 1, 2 at f3 = -1 / sqrt(5): 3.04, bin 3.
    FPFH of row 0, list (row 3, d2 1), (row 1, 4), (row 2, 4): f3 = c_3 / 2 / 1 + c_1 / 3 / 4 + c_2 / 3 / 4 -> bin 3: 1, bin 5: 1/3,
    bin 7: 1/6; S = 3/2 -> 200/3, 200/9, 100/9.  Row 3, list (row 0, 1), (row 1, 5), (row 2, 5): bin 5: 1 + 2 (2/3)/5 = 19/15,
    bin 7: 2 (1/3)/5 = 2/15; S = 21/15 -> 1900/21, 200/21."""
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1]], np.float32)
    nrm = np.tile(UP, (4, 1))
    r = ref.fpfh(pts, nrm, 4)
    want = np.zeros((4, 33), np.int64)
    want[0, [5, 16, 27]] = 2
    want[1, [5, 16]] = 3; want[1, 27] = 2; want[1, 29] = 1
    want[2] = want[1]
    want[3, [5, 16, 25]] = 2
    assert np.array_equal(r["counts"], want) and list(r["m"]) == [2, 3, 3, 2]
    assert not r["sensitive"].any()
    out = np.asarray(r["out"], np.float64)
    f12 = np.zeros(22); f12[[5, 16]] = 100.0
    assert (out[:, :22] == f12[None, :]).all()
    w0 = np.zeros(11); w0[3], w0[5], w0[7] = 200 / 3, 200 / 9, 100 / 9
    w3 = np.zeros(11); w3[5], w3[7] = 1900 / 21, 200 / 21
    assert np.abs(out[0, 22:] - w0).max() <= ref.OUT_TOL and np.abs(out[3, 22:] - w3).max() <= ref.OUT_TOL
    counts, pout = ref.plain_double(pts, nrm, 4)
    assert np.array_equal(counts, want) and np.abs(pout - out).max() <= ref.OUT_TOL


def test_rows_without_a_descriptor():
    """a non-finite row is 33 NaN and nobody's neighbour; coincident rows and a lone row are 33 zeros; a NaN normal counts in no
    SPFH but its row still receives an FPFH"""
    same = np.tile(np.array([[1.5, 2.5, 3.5]], np.float32), (5, 1))
    r = ref.fpfh(same, np.tile(UP, (5, 1)), 4)
    assert (r["out"] == 0).all() and (r["counts"] == 0).all()
    r = ref.fpfh(same[:1], UP[None], 3)
    assert (r["out"] == 0).all()
    model, nrm = ref.family_inputs("sheet")
    model, nrm = model[:300].copy(), nrm[:300].copy()
    model[7, 1] = np.nan
    nrm[11] = np.nan
    r = ref.fpfh(model, nrm, 8)
    assert np.isnan(r["out"][7]).all() and not np.isnan(np.delete(r["out"], 7, axis=0)).any()
    assert (r["counts"][[7, 11]] == 0).all() and r["out"][11].sum() > 299.0
    idx, _d2, nb = ref.neighbours(model, 8)
    assert not (nb & (idx == 7)).any()
    near11 = (nb & (idx == 11)).any(axis=1)
    assert near11.any() and (r["m"][near11] < 7).all()


@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("name", ["sheet", "volume"])
def test_plain_double_restatement_and_the_excluded_share(name, k):
    model, nrm = ref.family_inputs(name)
    r = ref.case(name, k)
    share = ref.excluded_share(r)
    print(f"{name} k = {k}: sensitive {100 * r['sensitive'].mean():.2f} %, excluded {100 * share:.2f} %")
    assert share <= ref.EXCLUDED_CAP
    assert (r["m"] == k - 1).all()
    counts, out = ref.plain_double(model, nrm, k)
    assert np.array_equal(counts, r["counts"])
    err = float(np.abs(out - np.asarray(r["out"], np.float64)).max())
    print(f"{name} k = {k}: plain double at most {err:.2e} from the reference (bound {ref.OUT_TOL:.2e})")
    assert err <= ref.OUT_TOL
    s = np.asarray(r["out"], np.float64).reshape(len(model), 3, 11).sum(axis=2)
    assert np.abs(s - 100.0).max() <= 1e-10
