"""Fast global registration (fgr.hip + fgr_pair.hpp) on the GPU, both kernel forms, every tier.

The reference is tests/fgr_ref.py.  EXACT against it: n_live, n_kept, kept, mu0, mu_final, failed (the contract defines them in
float64); n_inliers, inlier_idx and sum_d2 against a float64 restatement on the T that the device reported (fgr_ref.tail64); the
inlier set against the planted one.  THE BOUND of T and cost is tests/test_gpu_cpd.py's rule: within 8 x E_method of run_ld, where
E_method = |run64 - run_ld| is recomputed on the CPU for the inputs of the call (run64: the contract in float64 with sequential
sums), per output the worst over the call's registrations and never below E_FLOOR = 2^-49.  The 8 is that test's margin and is
taken for the same reason: the device's trees against the restatement's sequences.
On top of the issue's checks the device is held to run_tree -- run64 with the contract's own sum order -- BIT FOR BIT, in every
test of this file: the contract fixes every operation and every order, so nothing is left to a tolerance.

MEASURED on one MI355X, the worst share of the bound over the three scenes: 0.108 for T and 0.102 for cost (both at n = 1000),
the same for both forms (they give the same bits)."""
import numpy as np
import pytest
import torch

import fgr_ref

pytestmark = pytest.mark.gpu
FACTOR = 8.0
EXACT = ("failed", "n", "n_live", "n_kept", "n_inliers")
BITS = ("T", "mu0", "mu_final", "cost", "sum_d2")
QUICK = dict(iterations=12, decrease_every=2)              # the edges need the paths, not the convergence


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _as_dict(r, inl, kept, off, n):
    return dict(T=np.array(r.T[:]).reshape(4, 4, order="F"), failed=bool(r.failed), n=r.n, n_live=r.n_live, n_kept=r.n_kept, mu0=r.mu0,
                mu_final=r.mu_final, cost=r.cost, n_inliers=r.n_inliers, sum_d2=r.sum_d2, inlier_idx=inl[off:off + r.n_inliers].copy(),
                kept=None if kept is None else kept[off:off + n].astype(bool))


def _enqueue(p1s, p2s, opts, T0=None, table=None, pad=5, ws_fill=None, n_cap=None):
    """the device tier: offsets on the device, ld > total (the rows behind total hold NaN) -> a function that reads the results"""
    from pcreg_amd._lib import lib
    from pcreg_amd.device import fgr_batched_dev, fgr_results
    dev = torch.device("cuda")
    sizes = [len(p) for p in p1s]
    offs = np.zeros(len(sizes) + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    total, ld = int(offs[-1]), int(offs[-1]) + pad
    a1, a2 = np.full((3, ld), np.nan), np.full((3, ld), np.nan)
    if total:
        a1[:, :total], a2[:, :total] = np.concatenate(p1s).T, np.concatenate(p2s).T
    cap = max(sizes) if n_cap is None else n_cap
    need = lib().pcreg_dev_fgr_batched_workspace(cap, len(sizes), fgr_ref.options(**opts)["iterations"])
    ws = None if ws_fill is None else torch.full((need,), ws_fill, dtype=torch.uint8, device=dev)
    t0 = None if T0 is None else torch.from_numpy(np.ascontiguousarray(np.asarray(T0, np.float64).transpose(0, 2, 1)).reshape(-1, 16)).to(dev)
    tb = None if table is None else torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    res, inl, kept = fgr_batched_dev(torch.from_numpy(a1).to(dev), torch.from_numpy(a2).to(dev), torch.from_numpy(offs).to(dev), cap, opts, T0=t0,
                                     tuple_idx=tb, kept=True, ws=ws)

    def read():
        rs, hi, hk = fgr_results(res.cpu().numpy()), inl.cpu().numpy(), kept.cpu().numpy()
        return [_as_dict(r, hi, hk, int(offs[b]), sizes[b]) for b, r in enumerate(rs)]
    return read


def _dev(*a, **k):
    return _enqueue(*a, **k)()


def _same(got, ref, what=""):
    for k in EXACT:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in BITS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg=f"{what} {k}")
    np.testing.assert_array_equal(got["inlier_idx"], ref["inlier_idx"], err_msg=what)
    if got["kept"] is not None and ref["kept"] is not None:
        np.testing.assert_array_equal(got["kept"], ref["kept"], err_msg=what)


_REFS = {}


def _scene_refs():
    """the three scenes' references at the defaults, computed once: (ld, r64, tree) per scene"""
    if not _REFS:
        o = fgr_ref.options()
        for k, sc in enumerate(fgr_ref.scenes()):
            _REFS[k] = tuple(f(sc["p1"], sc["p2"], o, b=k) for f in (fgr_ref.run_ld, fgr_ref.run64, fgr_ref.run_tree))
    return [_REFS[k] for k in range(len(fgr_ref.CASES))]


@pytest.mark.parametrize("form", ["resident", "chain"])
def test_the_three_scenes_against_the_reference(form, debug_set):
    """check 1 (and the forms of check 2)"""
    import pcreg_amd as pc
    if form == "chain":
        debug_set("fgr_chain", 1)
    scs, refs = fgr_ref.scenes(), _scene_refs()
    opts = {"delta2": fgr_ref.DELTA ** 2}
    got = pc.fgr_batched([s["p1"] for s in scs], [s["p2"] for s in scs], opts)
    E = fgr_ref.method_error([r[0] for r in refs], [r[1] for r in refs])
    worst = dict(T=0.0, cost=0.0)
    for b, (sc, g, (ld, r64, tree)) in enumerate(zip(scs, got, refs)):
        g = dict(g, n=len(sc["p1"]))
        for k in ("failed", "n_live", "n_kept", "mu0", "mu_final"):
            assert g[k] == ld[k] == r64[k], (b, k)
        assert not g["failed"]
        np.testing.assert_array_equal(g["kept"], ld["kept"])
        n_inl, idx, sum_d2, _cost = fgr_ref.tail64(sc["p1"], sc["p2"], g["kept"], g["T"], g["mu_final"], opts["delta2"])
        assert g["n_inliers"] == n_inl and _bits(g["sum_d2"]) == _bits(sum_d2)
        np.testing.assert_array_equal(g["inlier_idx"], idx)
        np.testing.assert_array_equal(g["inlier_idx"], np.flatnonzero(sc["inliers"]) + 1)          # the planted set
        shares = dict(T=float(np.linalg.norm(g["T"] - ld["T"])) / (FACTOR * E["T"]), cost=abs(g["cost"] - ld["cost"]) / abs(ld["cost"]) / (FACTOR * E["cost"]))
        print(f"  {form} n = {len(sc['p1'])}: " + ", ".join(f"{k} {v:.3f} of its bound ({FACTOR * E[k]:.2e})" for k, v in shares.items()))
        for k, v in shares.items():
            assert v <= 1.0, (b, k, v)
            worst[k] = max(worst[k], v)
        _same(g, tree, f"{form} scene {b}")
    print(f"  {form}: the worst share of the bound: T {worst['T']:.3f}, cost {worst['cost']:.3f}")


def _small_batch(B, seed):
    rng = np.random.default_rng(seed)
    p1s, p2s = [], []
    for _ in range(B):
        s = fgr_ref.scene(int(rng.integers(0, 40)), 0.3, float(rng.uniform(0.1, 3.0)), int(rng.integers(1 << 30)))
        p1s.append(s["p1"]); p2s.append(s["p2"])
    return p1s, p2s


def test_same_bits_whatever_the_call(debug_set):
    """check 2: repeated, B = 1 against any position of a mixed batch of 300, two streams at once, a workspace of 0xFF, both forms"""
    sc = fgr_ref.scenes()[0]
    opts = dict(delta2=1.0, n_tuples=700, seed=11)
    alone = _dev([sc["p1"]], [sc["p2"]], opts)[0]
    assert not alone["failed"] and 3 < alone["n_kept"] < len(sc["p1"])
    _same(alone, fgr_ref.run_tree(sc["p1"], sc["p2"], fgr_ref.options(**opts)), "alone")
    _same(_dev([sc["p1"]], [sc["p2"]], opts, ws_fill=0xFF, pad=0)[0], alone, "repeated on a workspace of 0xFF")
    p1s, p2s = _small_batch(300, 9)
    for form in ("resident", "chain"):
        debug_set("fgr_chain", int(form == "chain"))
        for pos in (0, 151, 299):
            a1, a2 = list(p1s), list(p2s)
            a1[pos], a2[pos] = sc["p1"], sc["p2"]
            got = _dev(a1, a2, dict(opts, seed=11 - pos), ws_fill=0xFF)          # (the built-in triples are seeded seed + b)
            _same(got[pos], alone, f"{form} position {pos}")
            if pos == 151:                                                       # the neighbours are themselves, too
                for b in (0, 150, 152, 299):
                    _same(got[b], fgr_ref.run_tree(a1[b], a2[b], fgr_ref.options(**dict(opts, seed=11 - pos)), b=b), f"{form} neighbour {b}")
        # two streams at once, each with its own buffers
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            r1 = _enqueue([sc["p1"]] * 40, [sc["p2"]] * 40, dict(opts, n_tuples=0))
        with torch.cuda.stream(s2):
            r2 = _enqueue([sc["p1"]] * 40, [sc["p2"]] * 40, dict(opts, n_tuples=0))
        torch.cuda.synchronize()
        a, b = r1(), r2()
        ref = _scene_refs()[0][2]
        for k in (0, 17, 39):
            _same(a[k], dict(ref, n=len(sc["p1"])), f"{form} stream 1, {k}")
            _same(b[k], dict(ref, n=len(sc["p1"])), f"{form} stream 2, {k}")


def _exact3():
    R = fgr_ref.rotation([1.0, 2.0, -1.0], 0.5)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.T, [3.0, -2.0, 1.0]
    p2 = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 1.0], [1.0, 5.0, 0.0]])
    return p2 @ R.T + T[3, :3], p2, T


@pytest.mark.parametrize("form", ["resident", "chain"])
def test_edges(form, debug_set):
    """check 3, in one batch: offsets on the device, ld > total"""
    debug_set("fgr_chain", int(form == "chain"))
    e1, e2, Te = _exact3()
    x = np.linspace(-3.0, 5.0, 30)
    line = np.stack([x, 2 * x + 1, -x], axis=1)
    big = fgr_ref.scene(2049, 0.4, 0.8, 31)
    sc = fgr_ref.scenes()[0]
    bad1, bad2 = sc["p1"][:100].copy(), sc["p2"][:100].copy()
    bad1[5, 2], bad2[40, 0], bad2[41, 1] = np.nan, np.inf, -np.inf
    cases = [("n = 0", np.zeros((0, 3)), np.zeros((0, 3))), ("n = 2", e1[:2], e2[:2]), ("n = 3 exact", e1, e2),
             ("n = 2047", big["p1"][:2047], big["p2"][:2047]), ("n = 2048", big["p1"][:2048], big["p2"][:2048]), ("n = 2049", big["p1"], big["p2"]),
             ("collinear", line + [0.5, 0.0, 0.0], line), ("NaN and Inf rows", bad1, bad2)]
    # a small mu and, for the three sizes around a chunk, a start near the truth: twelve iterations reach their inliers
    opts = dict(delta2=1.0, mu0=4.0, **QUICK)
    Tb = big["T"].copy()
    Tb[3, :3] += [0.3, -0.2, 0.25]
    T0s = np.stack([Tb if name.startswith("n = 204") else np.eye(4) for name, _p1, _p2 in cases])
    got = _dev([c[1] for c in cases], [c[2] for c in cases], opts, T0=T0s, ws_fill=0xFF)
    full = fgr_ref.options(**opts)
    res = {}
    for b, ((name, p1, p2), g) in enumerate(zip(cases, got)):
        _same(g, fgr_ref.run_tree(p1, p2, full, b=b, T0=T0s[b]), f"{form} {name}")
        res[name] = g
    for name in ("n = 0", "n = 2", "collinear"):
        g = res[name]
        assert g["failed"] and not g["T"].any() and g["n_inliers"] == 0 and g["cost"] == 0.0 and len(g["inlier_idx"]) == 0, name
    assert res["collinear"]["n_kept"] == 30                                    # failed by the pivot rule, not for want of pairs
    assert res["NaN and Inf rows"]["n_live"] == 97 and not res["NaN and Inf rows"]["kept"][[5, 40, 41]].any() and not res["NaN and Inf rows"]["failed"]
    for name in ("n = 2047", "n = 2048", "n = 2049"):
        assert not res[name]["failed"] and res[name]["n_inliers"] == big["inliers"][:int(name[4:])].sum() > 1000, name
    # three exact pairs at the defaults: the planted motion, within the bound
    g = _dev([e1], [e2], dict(delta2=1.0))[0]
    ld, r64 = fgr_ref.run_ld(e1, e2, fgr_ref.options()), fgr_ref.run64(e1, e2, fgr_ref.options())
    E = fgr_ref.method_error([ld], [r64])
    assert not g["failed"] and g["n_inliers"] == 3 and np.linalg.norm(ld["T"] - Te) < 1e-9
    assert np.linalg.norm(g["T"] - ld["T"]) <= FACTOR * E["T"], (np.linalg.norm(g["T"] - ld["T"]), E)
    # T0 given against the identity, iterations = 1, mu0 given
    T0 = sc["T"].copy()
    T0[3, :3] += [0.5, -0.3, 0.2]
    for o2, t0 in ((dict(delta2=1.0, **QUICK), T0), (dict(delta2=1.0, iterations=1), None), (dict(delta2=1.0, iterations=1), T0),
                   (dict(delta2=1.0, mu0=4.0, **QUICK), T0), (dict(delta2=2.0, mu0=1.0, iterations=3, decrease_every=1, division_factor=3.0), T0)):
        g = _dev([sc["p1"], sc["p1"]], [sc["p2"], sc["p2"]], o2, T0=None if t0 is None else np.stack([np.eye(4), t0]))
        _same(g[0], fgr_ref.run_tree(sc["p1"], sc["p2"], fgr_ref.options(**o2), b=0), f"{form} identity {o2}")
        _same(g[1], fgr_ref.run_tree(sc["p1"], sc["p2"], fgr_ref.options(**o2), b=1, T0=t0), f"{form} T0 {o2}")
        if "mu0" in o2:
            assert g[1]["mu0"] == o2["mu0"]
        assert t0 is None or not np.array_equal(_bits(g[0]["T"]), _bits(g[1]["T"]))        # the start is read
        if o2.get("mu0") == 4.0:                        # a start near the truth and a small mu: the planted set in twelve iterations
            assert g[1]["n_inliers"] == sc["inliers"].sum()


def test_the_resident_capacity_and_one_more():
    """check 3: the two sizes around the switch between the forms, without the key; a registration above n_cap is refused"""
    from pcreg_amd._lib import lib
    cap = lib().pcreg_fgr_resident_capacity()
    assert cap * 48 <= 160 * 1024 - 2048
    s = fgr_ref.scene(cap + 1, 0.5, 1.2, 77)
    opts = dict(delta2=1.0, n_tuples=4000, seed=2, **QUICK)
    for n in (cap, cap + 1):
        g = _dev([s["p1"][:n], s["p1"][:50]], [s["p2"][:n], s["p2"][:50]], opts, ws_fill=0xFF)
        for b, m in ((0, n), (1, 50)):
            _same(g[b], fgr_ref.run_tree(s["p1"][:m], s["p2"][:m], fgr_ref.options(**opts), b=b), f"n = {n}, registration {b}")
        assert not g[0]["failed"] and 3 < g[0]["n_kept"] < n
    g = _dev([s["p1"][:50], s["p1"][:40]], [s["p2"][:50], s["p2"][:40]], dict(delta2=1.0, **QUICK), n_cap=45)
    assert g[0]["failed"] and g[0]["n"] == 50 and g[0]["n_live"] == 0 and not g[0]["T"].any() and not g[0]["kept"].any()
    _same(g[1], fgr_ref.run_tree(s["p1"][:40], s["p2"][:40], fgr_ref.options(delta2=1.0, **QUICK), b=1), "beside a refused registration")


@pytest.mark.parametrize("form", ["resident", "chain"])
def test_the_tuple_test(form, debug_set):
    """check 4: the built-in triples against the oracle's sample_table (fgr_ref.kept_mask draws from it), a caller's table with
    out-of-range entries, n_tuples = 1 and 4096, a case where no triple passes"""
    debug_set("fgr_chain", int(form == "chain"))
    sc = fgr_ref.scenes()[1]
    p1, p2 = sc["p1"].copy(), sc["p2"].copy()
    p1[np.flatnonzero(~sc["inliers"])[0], 0] = np.nan
    inl = np.flatnonzero(sc["inliers"])
    for nt in (1, 4096):
        opts = dict(delta2=1.0, n_tuples=nt, seed=21, **QUICK)
        got = _dev([p1, p1[inl[:3]], p1], [p2, p2[inl[:3]], p2], opts)
        for b, (a1, a2) in enumerate(((p1, p2), (p1[inl[:3]], p2[inl[:3]]), (p1, p2))):
            ref = fgr_ref.run_tree(a1, a2, fgr_ref.options(**opts), b=b)
            np.testing.assert_array_equal(got[b]["kept"], fgr_ref.kept_mask(a1, a2, fgr_ref.options(**opts), b))
            _same(got[b], ref, f"{form} n_tuples {nt} registration {b}")
        if nt == 4096:
            assert 3 < got[0]["n_kept"] < len(p1) and not np.array_equal(got[0]["kept"], got[2]["kept"]) and not got[0]["failed"]
        else:                                           # one triple of three inliers keeps exactly them
            assert got[1]["n_kept"] == 3 and not got[1]["failed"]
    rng = np.random.default_rng(8)
    table = rng.integers(-1000, len(p1) + 1000, (2, 900, 3))
    table[0, :40] = inl[rng.integers(0, len(inl), (40, 3))] + 1
    opts = dict(delta2=1.0, n_tuples=900, **QUICK)
    got = _dev([p1, p1[:200]], [p2, p2[:200]], opts, table=table)
    for b, m in ((0, len(p1)), (1, 200)):
        _same(got[b], fgr_ref.run_tree(p1[:m], p2[:m], fgr_ref.options(**opts), b=b, tuple_idx=table[b]), f"{form} table, registration {b}")
    assert got[0]["n_kept"] >= 3
    s0 = fgr_ref.scenes()[0]                            # (tests/test_fgr_ref.py: no triple of this case passes)
    opts = dict(delta2=1.0, n_tuples=3000, **QUICK)
    got = _dev([s0["p1"] * 1.1], [s0["p2"]], opts)[0]
    _same(got, fgr_ref.run_tree(s0["p1"] * 1.1, s0["p2"], fgr_ref.options(**opts)), f"{form} no triple passes")
    assert got["failed"] and got["n_kept"] == 0 and got["n_live"] == len(s0["p1"]) and not got["kept"].any() and not got["T"].any()


def test_fgr_trials_equals_fgr_batched_with_one_host_sync(monkeypatch):
    """check 5, on the small sweep scene of tests/test_gpu_sweep.py"""
    import pcreg_amd as pc
    from pcreg_amd.sweep import SphereSweep
    from test_gpu_sweep import OPT, PAR, _scene
    featM, descM, featS, descS = _scene()
    sw = SphereSweep(featM, descM, featS, descS)
    res = sw.run(PAR, OPT, R_desc=9.0, d_spheres=6.0, min_pts=500, putative_thresh=60, seed=3)
    assert len(res["trial"]) >= 1
    opts = dict(delta2=OPT["thDist"], n_tuples=300, seed=4)
    calls = []
    orig_cpu, orig_item, orig_sync = torch.Tensor.cpu, torch.Tensor.item, torch.cuda.synchronize
    orig_ssync, orig_esync = torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu"), orig_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: (calls.append("item"), orig_item(self, *a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("synchronize"), orig_sync(*a, **k))[1])
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append("stream"), orig_ssync(self))[1])
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: (calls.append("event"), orig_esync(self))[1])
    got = sw.fgr_trials(res, opts)
    monkeypatch.undo()
    assert calls == ["cpu"], calls                                     # the final read and nothing else
    assert got["host_syncs"] == 1
    p1s = [featS[res["matches"][i][:, 0].astype(np.int64) - 1] for i in res["trial"]]
    p2s = [featM[res["model_rows"][i]][res["matches"][i][:, 1].astype(np.int64) - 1] for i in res["trial"]]
    want = pc.fgr_batched(p1s, p2s, opts)
    np.testing.assert_array_equal(got["trial"], res["trial"])
    np.testing.assert_array_equal(got["statsPutative"], res["statsPutative"])
    assert any(not w["failed"] for w in want)
    for t, w in enumerate(want):
        assert (got["transforms"][t] is None) == w["failed"]
        if not w["failed"]:
            np.testing.assert_array_equal(_bits(got["transforms"][t]), _bits(w["T"]))
        assert got["statsInliers"][t] == w["n_inliers"] and got["n_kept"][t] == w["n_kept"] and _bits(got["cost"][t]) == _bits(w["cost"])
        np.testing.assert_array_equal(got["inlierIdx"][t], w["inlier_idx"])
        assert got["statsRatio"][t] == 100.0 * w["n_inliers"] / len(p1s[t])
    with pytest.raises(ValueError, match="not the result"):
        sw.fgr_trials(dict(res), opts)


def test_register_fgr_is_its_chain_written_out():
    """check 6: bit for bit; no accuracy claim is made on a synthetic shape"""
    import pcreg_amd as pc
    rng = np.random.default_rng(12)
    u, v = rng.random(6000) * 8.0, rng.random(6000) * 6.0
    fixed = np.stack([u, v, np.sin(u) * np.cos(0.7 * v) + 0.3 * np.sin(2.3 * u + v)], axis=1).astype(np.float32)
    R = fgr_ref.rotation([0.2, -0.4, 1.0], 0.4)
    moving = ((fixed.astype(np.float64) - [4.0, 3.0, 0.0]) @ R.T + [0.7, -0.4, 0.3]).astype(np.float32)
    got = pc.register_fgr(moving, fixed, 0.25, opts=dict(n_tuples=500, seed=3))
    md, fd = pc.pcdownsample(moving, 0.25)[0], pc.pcdownsample(fixed, 0.25)[0]
    dm = pc.point_fpfh(md, 16, normals=pc.point_normals(md, 16))
    df = pc.point_fpfh(fd, 16, normals=pc.point_normals(fd, 16))
    m = pc.getMatches(dm, df, pc.api.REGISTER_FGR_MATCH)
    assert len(m) >= 3
    want = pc.fgr(fd[m[:, 1].astype(np.int64) - 1].astype(np.float64), md[m[:, 0].astype(np.int64) - 1].astype(np.float64),
                  dict(delta2=0.25 * 0.25, n_tuples=500, seed=3))
    np.testing.assert_array_equal(got["matches"], m)
    np.testing.assert_array_equal(got["moving_down"], md)
    assert got["failed"] == want["failed"]
    for k in BITS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    for k in ("n_live", "n_kept", "n_inliers"):
        assert got[k] == want[k]
    np.testing.assert_array_equal(got["inlier_idx"], want["inlier_idx"])
    np.testing.assert_array_equal(got["kept"], want["kept"])
