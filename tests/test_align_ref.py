"""The premises of tests/align_ref.py, checked without a GPU: every scene reaches the branch of align.hip's selection it is named
for, is well-posed, keeps its coeff bound at or below the 1e-9 the older align tests state; the project's fp64 oracles fall inside
the bounds (they are not too tight) and a subtly wrong rule lands at least 100 x outside them (they are not too loose)."""
import math

import numpy as np
import pytest

import align_ref as ref

SCENES = ref.SCENES
CASES = [(name, C1, C2) for name, s in SCENES.items() for (C1, C2) in s.flags]
_ID = lambda v: v if isinstance(v, str) else str(int(v))


def _all(name, C1, C2):
    s = SCENES[name]
    r = ref.scene_ref(name, C1, C2)
    q = ref.conditioning(s.X, C1, C2, r)
    return s, r, q, ref.tolerances(s.X, C1, C2, r, q)


def test_round_formula_is_sound():
    """align.hip:124 computes K = floor(n * 0.85 + 0.5) in fp64; the reference's round(0.85 n), half away from zero, exactly"""
    for n in range(2, 8193):
        assert int(math.floor(n * 0.85 + 0.5)) == ref.round_k(n), n
    assert [ref.round_k(n) for n in range(2, 8)] == [2, 3, 3, 4, 5, 6]


def test_exact_sums_against_fractions():
    """the integer core against brute-force Fractions on a small support with awkward exponents"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    X = rng.normal(size=(9, 3)) * np.array([0.25, 1.0, 40.0]) + np.array([0.1, -7.0, 1e6])
    r = ref.align(X, False, False)
    F = [[Fraction(float(v)) for v in row] for row in X]
    c = [sum(row[k] for row in F) / 9 for k in range(3)]
    assert [float(v) for v in c] == list(r["c"])
    d2 = [sum((row[k] - c[k]) ** 2 for k in range(3)) for row in F]
    kept = sorted(sorted(range(9), key=lambda i: (d2[i], i))[:8])
    assert kept == list(r["kept"]) and r["K"] == 8
    m = [sum(F[i][k] - c[k] for i in kept) / 8 for k in range(3)]
    C = np.array([[float(sum((F[i][a] - c[a] - m[a]) * (F[i][b] - c[b] - m[b]) for i in kept) / 7) for b in range(3)] for a in range(3)])
    w, V = np.linalg.eigh(C)
    assert np.allclose(np.sort(w)[::-1], r["eigenvalues"], rtol=1e-10, atol=0)      # (numpy's eigh is the loose side)
    assert np.abs(np.abs(V[:, ::-1].T @ r["coeff_pca"]) - np.eye(3)).max() < 1e-9


def test_scenes_fit_and_are_deterministic():
    assert all(2 <= s.n <= 8192 for s in SCENES.values())
    again = ref._build()
    assert list(again) == list(SCENES) and all(np.array_equal(again[k].X, SCENES[k].X) for k in SCENES)
    for pt, nt in ref.INSTANTIATIONS:
        assert f"filler_{pt * nt}" in SCENES and SCENES[f"filler_{pt * nt}"].n == pt * nt
    assert sum(s.n <= 1024 for s in SCENES.values()) >= 25          # most scenes run under all five instantiations


@pytest.mark.parametrize("name", list(SCENES))
def test_selection_reaches_the_branch(name):
    s = SCENES[name]
    sm = ref.selection_model(s.X)
    assert sm["robust"], (name, sm["m"], sm["edge_margin"])
    for key in ("branch", "split", "flat", "exact", "m", "n_eq", "take_eq", "bstar", "K"):
        if key in s.expect:
            assert sm[key] == s.expect[key], (name, key, sm[key], s.expect[key])
    assert sm["K"] == ref.round_k(s.n)
    if sm["split"]:
        assert 0 < sm["take_eq"] < sm["n_eq"]
        if not s.about_degeneracy:                                  # the tied rows differ in position
            assert len(np.unique(s.X[sm["tied_rows"]], axis=0)) > 1
    # the model and the exact reference keep the same rows
    c = s.X.sum(axis=0) / s.n
    x, y, z = s.X[:, 0] - c[0], s.X[:, 1] - c[1], s.X[:, 2] - c[2]
    kept = np.sort(np.lexsort((np.arange(s.n), np.sqrt(x * x + y * y + z * z)))[:sm["K"]])
    assert np.array_equal(kept, ref.scene_ref(name, *s.flags[0])["kept"])


def test_every_branch_has_a_scene():
    sms = {name: ref.selection_model(s.X) for name, s in SCENES.items()}
    have = {(m["branch"], m["split"]) for m in sms.values()}
    assert have == {("small", False), ("small", True), ("bisect", False), ("bisect", True)}
    assert {m["branch"] for m in sms.values() if m["flat"]} == {"small", "bisect"}
    for pt, nt in ref.INSTANTIATIONS:                                # every instantiation holds a scene of every kind
        fit = [n for n, s in SCENES.items() if s.holds(pt, nt)]
        assert {(sms[n]["branch"], sms[n]["split"]) for n in fit} == have
        assert any(n.startswith("crowded_split_interleaved") for n in fit) and "vote_tie" in fit
    # the interleaved order puts chosen ties into several register rows and waves of both workgroup sizes
    sm = sms["crowded_split_interleaved"]
    chosen = sm["tied_rows"][:sm["take_eq"]]
    for nt in (256, 512):
        assert len(set(chosen // nt)) >= 2 and len(set((chosen % nt) // 64)) == nt // 64
    big = sms["crowded_split_large"]["tied_rows"][:sms["crowded_split_large"]["take_eq"]]
    assert SCENES["crowded_split_large"].n <= 3072 and len(set(big // 256)) >= 11 and len(set(big // 512)) >= 6


@pytest.mark.parametrize("name,C1,C2", CASES, ids=_ID)
def test_scene_is_well_posed(name, C1, C2):
    s, r, q, tol = _all(name, C1, C2)
    # the K-th boundary: bit-equal distances, or a gap no rounding closes (2^-40, and the centroid's own bound where that is larger)
    if q["K"] < q["n"]:
        assert q["kth_bit_equal"] or q["kth_rel_gap"] * q["kth_distance"] >= 2.0 ** -40 * q["kth_distance"] + 8 * tol["c"].sum(), \
            (q["kth_rel_gap"], q["kth_exactly_equal"])
    if not s.about_degeneracy:
        assert min(q["eigen_gaps"]) >= 0.01 * q["trace"] > 0
        assert all(tol["determined"]) and all(tol["votes_determined"])
    want = s.expect.get("determined")
    if want is not None:
        assert tol["determined"] == tuple(want)
    for j in range(3):
        if tol["determined"][j]:
            assert q["column_sign_margins"][j] >= 1e-3
            assert tol["coeff"][j] <= 1e-9, (j, tol["coeff"][j])      # never looser than the tolerance the older tests state
    if "votes" in s.expect:
        assert r["votes"] == tuple(s.expect["votes"])
    if "signs_xz" in s.expect:
        assert (r["signs"][0], r["signs"][2]) == tuple(s.expect["signs_xz"])
    if name.startswith("vote_tie"):
        assert q["min_abs_proj"] >= 1e-6 and C2
        want = {"vote_tie": 0, "vote_tie_minus_half": -1, "vote_tie_plus_half": 1}[name]
        assert [2 * p - q["n"] for p in r["votes"]] == [want, want]      # n / 2 exactly, n / 2 - 1/2, n / 2 + 1/2
    if s.expect.get("kept_majority_below_half_n"):
        assert not C2 and 2 * r["votes"][0] >= q["K"] + 10 and 2 * r["votes"][0] <= q["n"] - 10
    if s.expect.get("permutation"):
        a = np.abs(r["coeff"])
        assert set(np.unique(a)) == {0.0, 1.0} and (a.sum(axis=0) == 1).all() and (a.sum(axis=1) == 1).all()
        assert tol["ortho"] == 8 * ref.U
    if name == "far":
        assert np.abs(s.X).max() > 4e6 and tol["c"].max() > 1e-9 > tol["coeff_max"]    # the bounds scale with |X|


def test_boxes_cover_all_six_orders():
    perms = set()
    for name, s in SCENES.items():
        if name.startswith("box_"):
            perms.add(tuple(np.argmax(np.abs(ref.scene_ref(name, False, False)["coeff"]), axis=0)))
    assert len(perms) == 6


@pytest.fixture(scope="module")
def oracle_ratios(oracle_c, oracle_py):
    out = {}
    for label, orc in (("oracle_c", oracle_c), ("oracle_py", oracle_py)):
        worst = dict(c=0.0, coeff=0.0, aligned=0.0)
        for name, C1, C2 in CASES:
            s, r, q, tol = _all(name, C1, C2)
            al, co, c = orc.AlignPoints_KNN(s.X, C1, C2)
            got = ref.compare(s.X, r, tol, c, co, al)                # asserts
            for k, v in got.items():
                worst[k] = max(worst[k], v)
        out[label] = worst
    return out


def test_oracles_fall_inside_the_bounds(oracle_ratios):
    """not too tight: two independent fp64 implementations with sequential sums pass the comparison the kernel must pass"""
    for label, worst in oracle_ratios.items():
        print(f"{label}: largest error / bound   centroid {worst['c']:.2e}   coeff {worst['coeff']:.2e}   aligned {worst['aligned']:.2e}")
        assert max(worst.values()) <= 1.0


MUTANTS = [(name, i) for name, s in SCENES.items() for i in range(len(s.mutants))]


@pytest.mark.parametrize("name,i", MUTANTS, ids=_ID)
def test_a_wrong_rule_lands_far_outside(name, i):
    """not too loose: the reference with one rule subtly wrong is at least 100 x the bound away, under every flag pair the rule
    shows under, and the comparison the GPU test uses rejects it"""
    s = SCENES[name]
    rules = s.mutants[i]
    if isinstance(rules.get("ties"), tuple):
        assert s.n > rules["ties"][1]                                # thread-major differs only beyond one row of points per thread
    for C1, C2 in rules.get("flags", s.flags):
        assert (C1, C2) in s.flags
        _, r, q, tol = _all(name, C1, C2)
        bad = ref.align(s.X, C1, C2, rules=rules)
        err = np.abs(bad["coeff"] - r["coeff"]).max(axis=0)
        assert (err / tol["coeff"]).max() >= 100.0, (rules, C1, C2, err, tol["coeff"])
        with pytest.raises(AssertionError):
            ref.compare(s.X, r, tol, bad["c"], bad["coeff"], bad["aligned"])


def test_every_rule_has_a_mutant():
    seen = set()
    for s in SCENES.values():
        for m in s.mutants:
            seen |= {(k, v if not isinstance(v, tuple) else v) for k, v in m.items() if k != "flags"}
    want = {("ties", "highest"), ("ties", ("thread", 256)), ("ties", ("thread", 512)), ("k_delta", 1), ("k_delta", -1), ("vote_cmp", ">"),
            ("vote_den", "K"), ("eig_order", "asc"), ("sign_rule", "first")}
    assert want <= seen
