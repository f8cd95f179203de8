"""The staged chain's band re-score (rs_score32_kernel's PCREG_SCORE_HYP and rs_block_count), slot by slot, against the C oracle.

The fp32 screen of a (hypothesis, 512 correspondences) unit leaves eight ballots and an 8-bit mask of the slots that hold a row
whose distance lies in the band around thDist; only those slots are scored again in fp64 on the raw coordinates and their ballot
replaced.  A slot that is skipped, or a ballot that lands in another slot, changes a count, an inlier list or -- through the masks
the refit sums read -- the refit itself.  Every scene therefore holds KNIFE-EDGE rows (ransac_refit_scenes.py: squared residual
thDist (1 + s delta), s = +-1) at chosen (point block, wave, slot, lane) positions, most of them on the INLIER side (s = -1), which
the screen leaves OUT of its ballot: only the re-score of the right slot puts them back.  The other rows of a slot are exact
inliers or far outliers (30 % at random rows), so the slots' ballots all differ.

Balance.  An inlier-side row is part of the refit.  The rows come in pairs that share their p2 row and carry opposite vectors v,
-v: sum v = 0 and sum (m - cm) v^T = 0 hold exactly, the refit is the scene's motion to rounding (ransac_refit_scenes.py,
"BALANCED") and the rows stay on the knife edge in the second pass.  A scene that asks for ONE band row in a unit or a block keeps
that row's partner in another unit / block.  The machinery's own scenes (scene("base"), scene("georef_zero"): every other inlier
row a knife-edge row, so every slot is a band slot) are taken as they are, with the hypotheses prepare() calls usable.

Honesty, checked on the host for every built scene, under the oracle's sample fit AND under its refit: each knife-edge row lies
within 1e-6 (relative) of thDist -- inside the band whatever the scene, whose half-width is at least 1.5 x 5.2 x 2^-24 x 4 =
1.86e-6 (make_t32) -- on the planned side; every other row lies further from thDist than an upper bound of the band's half-width
E (make_t32's formula with A, B, tau bounded from the scene).  So the band slots are exactly the planned ones.

Every scene runs with REFINE off (first pass alone: rs_score32_kernel<false>) and on (rs_score32_kernel<true>, then the second
pass forced full, "ransac_pass2" 1, and forced bounded, 2, where the "ransac_stats" counters prove the bounded kernels ran), with
iterNum = 1 and a one-row sample table (that refit is a seed: rs_bprep_kernel scores it in stored order) and with a table of 70
rows (64 seeds; the other six refits tie at the maximum, so rs_bounded_kernel walks them through every block of the bucket order).
Counts, numSuccess and inlier lists are the oracle's bits.  The staged chain needs a capacity of 4096 at these iterNum (staged_pays),
so the device n (2113, 512, 513) sits below a capacity of 4096, as in test_gpu_ransac_bound.py.

n = 2113: one full 2048-row point block (four waves x eight slots) and a block of 65 rows (one full slot, one slot with a single
live lane); for the bounded pass four 512-row blocks and one of 65.  n = 512 / 513: the bounded pass's block edge.
"""
import functools

import numpy as np
import pytest

from conftest import rigid_case
from ransac_refit_scenes import TH, _triples, prepare
from test_gpu_ransac_bound import _dev_ransac, _stats

pytestmark = pytest.mark.gpu

CAP = 4096
N = 2113
RATIO = 0.2
U = 2.0 ** -24
BAND_MIN = 1.5 * 5.2 * U * 4.0                  # relative half-width every band has (make_t32: E >= 1.5 * 5.2 u * 4 thDist)
LANES = (0, 31, 32, 63)                         # both halves of the ballot, their first and last lanes


def row_of(pb, wave, slot, lane):
    """Index of the correspondence that (point block, wave, slot, lane) of rs_score32_kernel scores."""
    return pb * 2048 + (wave * 8 + slot) * 64 + lane


def build(n, seed, pairs, outer=()):
    """rigid_case without noise; `pairs`: (row a, row b) -- both become inlier-side knife-edge rows on one p2 row with vectors v, -v;
    `outer`: rows that become outlier-side knife-edge rows (they are in no refit and need no partner)."""
    p1, p2, T = rigid_case(n, seed, noise=0.0, outlier_frac=0.3)
    p1 = p1.copy(); p2 = p2.copy()
    rng = np.random.default_rng(seed + 1)
    R, t = T[:3, :3], T[3, :3]

    def vec(sign):
        delta = 10.0 ** rng.uniform(-9.0, np.log10(5e-7))
        v = rng.normal(size=3)
        return v * (np.sqrt(TH * (1.0 + sign * delta)) / np.linalg.norm(v))

    knife, inner = [], []
    for a, b in pairs:
        assert a != b and a < n and b < n and a not in knife and b not in knife
        p2[b] = p2[a]
        v = vec(-1.0)
        p1[a] = p2[a] @ R + t + v; p1[b] = p2[a] @ R + t - v
        knife += [a, b]; inner += [a, b]
    for r in outer:
        assert r < n and r not in knife
        p1[r] = p2[r] @ R + t + vec(+1.0)
        knife.append(r)
    plain = np.flatnonzero(np.linalg.norm(p1 - (p2 @ R + t), axis=1) < 1e-9)
    plain = plain[~np.isin(plain, knife)]
    tab = _triples(rng, plain, p2, 64)
    junk = np.stack([rng.choice(n, 3, replace=False) + 1 for _ in range(6)]).astype(np.int32)     # hypotheses that mostly fail
    table70 = np.vstack([tab[:40], junk[:3], tab[40:], junk[3:]]).astype(np.int32)
    assert len(table70) == 70
    return dict(n=n, p1=p1, p2=p2, th=TH, knife=np.array(sorted(knife)), inner=np.array(sorted(inner)), table=tab[:1], table70=table70, built=True)


def band_ub(s, T):
    """Upper bound of make_t32's E for transform T (4 x 4, pts1 = [pts2 1] T): the origin is one of the rows, so A, B are at most the
    point sets' diameters and |t'| is that row's residual."""
    p1, p2 = s["p1"], s["p2"]
    A = 2.0 * np.linalg.norm(p1 - p1.mean(axis=0), axis=1).max(); B = 2.0 * np.linalg.norm(p2 - p2.mean(axis=0), axis=1).max()
    Rm = T[:3, :3]
    rho = max(np.linalg.norm(Rm, axis=0).max(), np.linalg.norm(Rm, axis=1).max())
    tau = np.linalg.norm(p1 - (p2 @ Rm + T[3, :3]), axis=1).max()
    e1 = U * (A + 5.1 * (B * rho + tau))
    return 1.5 * (2.0 * np.sqrt(3.0) * np.sqrt(4.0 * s["th"]) * e1 + 3.0 * e1 * e1 + 5.2 * U * 4.0 * s["th"])


def assert_band_rows(s, T, oracle_c):
    """Under T the knife-edge rows are in the band on their planned side and nobody else is."""
    d = oracle_c.calcDists(T, s["p1"], s["p2"])
    th = s["th"]
    k = np.zeros(s["n"], bool); k[s["knife"]] = True
    inner = np.zeros(s["n"], bool); inner[s["inner"]] = True
    assert (np.abs(d[k] / th - 1.0) < 1e-6).all() and 1e-6 < BAND_MIN, "a knife-edge row left the band"
    assert (d[inner] < th).all() and (d[k & ~inner] >= th).all(), "a knife-edge row changed sides"
    E = band_ub(s, T)
    assert E < 0.5 * th and (np.abs(d[~k] - th) > E).all(), "a row outside the plan may be in the band"


def coef_of(s, iters, refine):
    return dict(minPtNum=3, iterNum=iters, thDist=s["th"], thInlrRatio=RATIO, REFINE=refine, VERBOSE=0)


def same(r, ref, what, bad):
    if r["failed"] != int(bool(ref["failed"])):
        bad.append("%s: failed %d against the oracle's %d" % (what, r["failed"], int(bool(ref["failed"]))))
    elif not ref["failed"]:
        if (r["num_success"], r["max_inliers"]) != (ref["numSuccess"], ref["maxInliers"]) or not np.array_equal(r["inl"], ref["inlierIdx"]):
            bad.append("%s: numSuccess %d maxInliers %d (%d listed) against the oracle's %d %d (%d listed)" %
                       (what, r["num_success"], r["max_inliers"], len(r["inl"]), ref["numSuccess"], ref["maxInliers"], len(ref["inlierIdx"])))


def run_table(s, table, debug_set, oracle_c, label, check_rows=False):
    """One sample table through the first pass alone, the full and the bounded second pass; returns the list of disagreements."""
    p1, p2, n = s["p1"], s["p2"], s["n"]
    iters = len(table)
    ref1 = oracle_c.ransac(p1, p2, coef_of(s, iters, False), sample_idx=table)
    ref = oracle_c.ransac(p1, p2, coef_of(s, iters, True), sample_idx=table)
    if check_rows:                                   # a one-row table of a built scene: T is that hypothesis' fit / refit
        assert not ref1["failed"] and not ref["failed"] and ref["numSuccess"] == 1
        assert_band_rows(s, ref1["T"], oracle_c); assert_band_rows(s, ref["T"], oracle_c)
        assert np.isin(s["inner"] + 1, ref1["inlierIdx"]).all() and np.isin(s["inner"] + 1, ref["inlierIdx"]).all()
    bad = []
    r1 = _dev_ransac(p1, p2, coef_of(s, iters, False), 0, sample_idx=table, extra_cap=CAP - n)
    assert r1["n"] == n
    same(r1, ref1, "%s, %d rows, first pass" % (label, iters), bad)
    debug_set("ransac_pass2", 1)
    full = _dev_ransac(p1, p2, coef_of(s, iters, True), 0, sample_idx=table, extra_cap=CAP - n)
    same(full, ref, "%s, %d rows, full second pass" % (label, iters), bad)
    debug_set("ransac_stats", 1)
    _stats(reset=True)
    debug_set("ransac_pass2", 2)
    bounded = _dev_ransac(p1, p2, coef_of(s, iters, True), 0, sample_idx=table, extra_cap=CAP - n)
    st = _stats()
    debug_set("ransac_pass2", 0)
    assert st[0] == 1 and 0 < st[1] <= st[2], ("the bounded pass did not run", st)
    same(bounded, ref, "%s, %d rows, bounded second pass" % (label, iters), bad)
    if not bad and not ref["failed"]:
        for k in ("T", "winner"):
            if not np.array_equal(full[k], bounded[k]):
                bad.append("%s, %d rows: %s differs between the full and the bounded pass" % (label, iters, k))
    return bad


def run_built(s, debug_set, oracle_c, label):
    bad = run_table(s, s["table"], debug_set, oracle_c, label, check_rows=True)
    bad += run_table(s, s["table70"], debug_set, oracle_c, label)
    return bad


def bucket_positions(s, oracle_c):
    """Where the bounded pass's order can put the knife-edge rows: bucket 0 holds the rows with d >= thDist, the rows with d just below
    it follow in bucket 1, the exact inliers come last; a knife-edge row sits in bucket 0 or 1 depending on its fp32 rounding, so its
    position is below (rows clearly outside) + (knife-edge rows)."""
    ref = oracle_c.ransac(s["p1"], s["p2"], coef_of(s, 1, True), sample_idx=s["table"])
    d = oracle_c.calcDists(ref["T"], s["p1"], s["p2"])
    return int((d > 1.01 * s["th"]).sum()) + len(s["knife"])


# ---- one band row per unit, by slot ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", range(8))
def test_one_band_row_per_unit_by_slot(slot, debug_set, oracle_c):
    """Slot `slot` of each of the four waves of the full point block holds one inlier-side row (waves 0 / 1 and 2 / 3 are partners);
    the lanes rotate through 0, 31, 32, 63.  Wave 3's row has an index of 1536 or more and a position in the bucket order below
    1024: the bounded pass meets it in another block than its index."""
    bad = []
    for rot in range(4):
        rows = [row_of(0, w, slot, LANES[(w + rot) % 4]) for w in range(4)]
        s = build(N, 100 + 8 * rot + slot, [(rows[0], rows[1]), (rows[2], rows[3])])
        assert rows[3] >= 1536 and bucket_positions(s, oracle_c) <= 1024
        bad += run_built(s, debug_set, oracle_c, "slot %d rotation %d" % (slot, rot))
    assert not bad, "\n".join(bad)


# ---- several band slots in one unit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [(3, 4), (0, 7), (1, 1, 4, 6), (0, 1, 2, 3, 4, 5, 6, 7)], ids=["adjacent", "first_and_last", "three", "all_eight"])
def test_several_band_slots_in_one_unit(slots, debug_set, oracle_c):
    """All the band rows of the scene in ONE unit (wave 2 of the full block), partners included: two adjacent slots, slots 0 and 7,
    three slots (two rows in slot 1) and all eight; plus one outlier-side row in a planned slot."""
    lanes = [LANES[k % 4] for k in range(len(slots))]
    rows = [row_of(0, 2, sl, ln) for sl, ln in zip(slots, lanes)]
    assert len(set(rows)) == len(rows)
    outer = [row_of(0, 2, slots[-1], 17)]
    s = build(N, 300 + len(slots) + slots[0], list(zip(rows[0::2], rows[1::2])), outer)
    bad = run_built(s, debug_set, oracle_c, "slots %s" % (slots,))
    assert not bad, "\n".join(bad)


# ---- the ragged tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["last_row", "full_slot_of_the_tail"])
def test_ragged_tail(kind, debug_set, oracle_c):
    """The 65-row block holds exactly one band row: the last row (n - 1), alone in a slot whose other lanes are past n, or a row of
    the block's full slot; the partner sits in the full block."""
    row = N - 1 if kind == "last_row" else 2048 + 40
    assert row_of(1, 0, 1, 0) == N - 1
    s = build(N, 400 + len(kind), [(row, row_of(0, 1, 5, 32))])
    bad = run_built(s, debug_set, oracle_c, kind)
    assert not bad, "\n".join(bad)


# ---- the bounded pass's block edge ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 513])
def test_block_edge_of_the_bounded_pass(n, debug_set, oracle_c):
    """n = 512: one full 512-row block; 513: a second block of one row.  The last row and row 100 are partners; then the machinery's
    base scene of that n (every slot a band slot)."""
    s = build(n, 500 + n, [(n - 1, 100)], outer=[n - 2])
    bad = run_built(s, debug_set, oracle_c, "n %d" % n)
    b = prepare("base", n)
    for i, h in enumerate(b["hyps"]):
        if h["usable"]:
            bad += run_table(b, h["table"], debug_set, oracle_c, "base n %d hyp %d" % (n, i))
    assert not bad, "\n".join(bad)


# ---- the screen unusable: every slot in the band ---------------------------------------------------------------------------------------
def test_screen_unusable_every_slot_in_the_band(debug_set, oracle_c):
    """scene("georef_zero"): coordinates of 4e6 with row 0 at zero.  The offsets alone do NOT trip make_t32's gate (E > thDist / 2) --
    the screen works on coordinates relative to an origin among the rows -- but row 0 lies 6e6 from every other row, the origin is
    not row 0 (it is the row at the MEDIAN distance from row 0 among 31 spread rows), so A >= min |p1[r] - p1[0]| and
    E >= 1.5 x 2 sqrt(3) sqrt(4 thDist) u A, computed here: far above thDist / 2.  lo = -inf, hi = +inf: every slot with a live lane
    is re-scored."""
    s = prepare("georef_zero", N)
    A_lb = np.linalg.norm(s["p1"][1:] - s["p1"][0], axis=1).min()
    E_lb = 1.5 * 2.0 * np.sqrt(3.0) * np.sqrt(4.0 * s["th"]) * U * A_lb
    print("\nBAND georef_zero n %d: A >= %.3e, E >= %.3e against thDist / 2 = %.3e" % (N, A_lb, E_lb, 0.5 * s["th"]))
    assert E_lb > 0.5 * s["th"]
    bad = []
    for i, h in enumerate(s["hyps"]):
        if h["usable"]:
            bad += run_table(s, h["table"], debug_set, oracle_c, "georef_zero hyp %d" % i)
    assert not bad, "\n".join(bad)


# ---- hypothesis loop edges and the other modes, on the machinery's base scene ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base_tables():
    s = prepare("base", N)
    rng = np.random.default_rng(9)
    tab = _triples(rng, s["plain"], s["p2"], 70)
    return s, tab


@pytest.mark.parametrize("iters", [1, 33, 70])
def test_hypothesis_loop_edges(iters, debug_set, oracle_c):
    """kSChunk = 32 hypotheses per workgroup, two per trip of the row-prefetch loop: 1 (the `h + 1 < h1` branch not taken), 33 (a full
    chunk and a chunk of one) and 70 (two full chunks and six: an even tail; more refits than seeds)."""
    s, tab = _base_tables()
    bad = []
    if iters == 1:
        for i, h in enumerate(s["hyps"]):
            if h["usable"]:
                bad += run_table(s, h["table"], debug_set, oracle_c, "base hyp %d" % i)
    else:
        bad += run_table(s, tab[:iters], debug_set, oracle_c, "base")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["ransac_f64score", "ransac_nolane"])
def test_other_modes_on_the_base_scene(mode, debug_set, oracle_c):
    """No fp32 screen at all / the first pass without masks (rs_score32_kernel<false>) and the fp64 sweep's refit sums."""
    s, tab = _base_tables()
    debug_set(mode, 1)
    bad = []
    for table in [h["table"] for h in s["hyps"] if h["usable"]][:3] + [tab[:33]]:
        iters = len(table)
        for refine in (False, True):
            ref = oracle_c.ransac(s["p1"], s["p2"], coef_of(s, iters, refine), sample_idx=table)
            r = _dev_ransac(s["p1"], s["p2"], coef_of(s, iters, refine), 0, sample_idx=table, extra_cap=CAP - N)
            same(r, ref, "%s, %d rows, REFINE %d" % (mode, iters, refine), bad)
    assert not bad, "\n".join(bad)
