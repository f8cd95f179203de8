"""What a caller-owned workspace holds before a call must not change any result.

pcreg_amd/device.py caches one workspace per operation and reuses it for every later call, whatever its shape, so a launcher
nearly always runs on an earlier call's counters, list lengths, flags and candidate lists.  This module holds ONE registry of
cases -- a case per device-tier entry with a *_workspace size function (include/pcreg.h) -- and the three checks every case gets
(tests/test_gpu_ws_state.py runs them):

fills     the call on a workspace of exactly need bytes of 0x00 and on one of 0xFF (-1 as an int32, a NaN as a float, a huge
          unsigned count): the same bits, and the 0x00 run is held against the operation's own reference.
sequence  the case's shapes A, B, C, ..., A in order on ONE workspace of max(need) bytes filled with 0xFF once, each call told
          workspace_bytes = need(shape): every result has the bits of the same shape on a fresh 0x00 workspace.
outputs   every output is allocated with a sentinel (-7; a NaN with a payload) between two guards of 64 elements: the guards keep
          the sentinel, the documented region equals the reference, slots the header documents as untouched keep the sentinel.

A case has need(shape), call(shape, ws, ws_bytes, new) -> nested dicts / lists of numpy arrays (the region the header
documents as written; `new(shape, dtype)` allocates an output), expect(shape, got), which asserts against the reference the
operation's own test file uses through that file's comparator, and optionally untouched(shape, raw), which asserts on the raw
output tensors.  Every output of every call of every check is a sentinel tensor between guards, and the guards are checked after
every call.
"""
import ctypes as C
import functools

import numpy as np
import torch

GUARD = 64
INT_SENTINEL = -7
F32_SENTINEL, F64_SENTINEL = 0x7FC0BEEF, 0x7FF80000DEADBEEF        # quiet NaNs with a payload
_AS_INT = {torch.float32: (torch.int32, F32_SENTINEL), torch.float64: (torch.int64, F64_SENTINEL)}


def dev():
    return torch.device("cuda", 0)


def ptr(t):
    """the address of a tensor; of an output of no elements, the address between its guards (torch reports none for it)"""
    return C.c_void_p(getattr(t, "empty_at", 0) or t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fill_sentinel(buf):
    if buf.dtype in _AS_INT:
        as_int, word = _AS_INT[buf.dtype]
        buf.view(as_int).fill_(word)
    elif buf.dtype == torch.uint8:
        buf.fill_(INT_SENTINEL & 0xFF)
    else:
        buf.fill_(INT_SENTINEL)


def is_sentinel(a):
    """elementwise, on a numpy array an output tensor was copied to"""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32) == np.uint32(F32_SENTINEL)
    if a.dtype == np.float64:
        return a.view(np.uint64) == np.uint64(F64_SENTINEL)
    if a.dtype == np.uint8:
        return a == np.uint8(INT_SENTINEL & 0xFF)
    return a == INT_SENTINEL


class Outputs:
    """Allocates a call's outputs: each a contiguous tensor of sentinels with GUARD sentinel elements in front and behind."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape, dtype=np.int64))
        buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev())
        _fill_sentinel(buf)
        self.bufs.append((buf, n))
        view = buf[GUARD:GUARD + n].view(shape)
        if n == 0:
            view.empty_at = buf.data_ptr() + GUARD * buf.element_size()
        return view

    def check_guards(self, what=""):
        torch.cuda.synchronize()
        for k, (buf, n) in enumerate(self.bufs):
            h = buf.cpu().numpy()
            assert is_sentinel(h[:GUARD]).all(), f"{what}: a write in front of output {k}"
            assert is_sentinel(h[GUARD + n:]).all(), f"{what}: a write behind output {k}"


def same_bits(a, b, where=""):
    """nested dicts / lists / arrays / numbers: the same structure, dtypes, shapes and bits (NaNs included)"""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same_bits(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{where}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, where
    else:
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, (where, x.dtype, y.dtype, x.shape, y.shape)
        bad = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))
        assert bad.size == 0, f"{where}: {bad.size} bytes differ, the first at byte {bad[:1]}"


def workspace(nbytes, fill):
    """nbytes (at least one allocation granule, so that an empty call still has an address) of the byte `fill`"""
    return torch.full((max(int(nbytes), 256),), fill, dtype=torch.uint8, device=dev())


def run(case, shape, ws, raw=None):
    """one call on the first need(shape) bytes of ws -> its documented outputs; the guards of every output are checked.
    raw: a list that receives the Outputs (for `untouched`)."""
    outs = Outputs()
    need = int(case.need(shape))
    assert 0 <= need <= ws.numel() or need <= 256, (need, ws.numel())
    got = case.call(shape, ws, need, outs.new)
    outs.check_guards(f"{case.name} {shape}")
    if raw is not None:
        raw.append(outs)
    return got


def fills(case, shape):
    zero = run(case, shape, workspace(case.need(shape), 0x00))
    ones = run(case, shape, workspace(case.need(shape), 0xFF))
    same_bits(zero, ones, f"{case.name} {shape}: 0x00 against 0xFF")
    case.expect(shape, zero)
    return zero


def sequence(case, shapes=None):
    shapes = list(case.shapes if shapes is None else shapes)
    fresh = [run(case, s, workspace(case.need(s), 0x00)) for s in shapes]
    ws = workspace(max(int(case.need(s)) for s in shapes), 0xFF)
    order = list(range(len(shapes))) + [0]
    for step, k in enumerate(order):
        got = run(case, shapes[k], ws)
        same_bits(got, fresh[k], f"{case.name} step {step} {shapes[k]}: the reused workspace against a fresh one")
    case.expect(shapes[0], fresh[0])


def outputs(case):
    shape = case.shapes[0]
    raw = []
    got = run(case, shape, workspace(case.need(shape), 0xFF), raw)
    case.expect(shape, got)
    case.untouched(shape, raw[0].bufs)


def host(t):
    return t.cpu().numpy()


def inner(bufs, k):
    """output k of a call as numpy, without its guards"""
    buf, n = bufs[k]
    return buf[GUARD:GUARD + n].cpu().numpy()


def soa32(x):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    t = torch.empty((3, len(x)), dtype=torch.float32, device=dev())
    if len(x):
        t.copy_(torch.from_numpy(np.array(x.T, order="C")))
    return t


def oracle_c():
    from oracle import c_oracle
    c_oracle.build()
    c_oracle.lib()
    return c_oracle


CASES = {}


def register(cls):
    case = cls()
    assert case.name not in CASES
    CASES[case.name] = case
    return cls


class Case:
    """size_fn: the size function of include/pcreg.h the case covers; shapes: its sequence (the helper appends the first again);
    flags: the pcreg_debug_set settings under which the whole sequence runs again, by id"""
    name = size_fn = None
    shapes = ()
    flags = {"default": {}}

    def untouched(self, shape, bufs):
        pass

    def shapes_for(self, flag):
        """the sequence under one of `flags`"""
        return list(self.shapes)


# ---- pcreg_dev_ransac ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ransac_scene(n, seed, frac):
    from test_gpu_ransac_bound import _bench_like
    p1, p2, _ = _bench_like(n, seed, outlier_frac=frac)
    return p1, p2


@functools.lru_cache(maxsize=None)
def _ransac_ref(n, seed, frac, iters, ratio, refine, rseed):
    p1, p2 = _ransac_scene(n, seed, frac)
    return oracle_c().ransac(p1, p2, _ransac_coef(iters, ratio, refine), seed=rseed)


def _ransac_coef(iters, ratio, refine):
    return dict(minPtNum=3, iterNum=iters, thDist=0.3, thInlrRatio=ratio, REFINE=refine, VERBOSE=0)


@register
class Ransac(Case):
    """(n, scene seed, outlier share, iterNum, thInlrRatio, REFINE): a long handover list; fewer refits than seeds; the resident
    kernel; a scene in which no hypothesis reaches thInlr"""
    name, size_fn = "ransac", "pcreg_dev_ransac_workspace"
    shapes = [(9000, 9700, 0.2, 800, 0.08, True), (4097, 4137, 0.2, 3, 0.08, True), (1000, 1300, 0.3, 2000, 0.08, True),
              (6000, 6100, 0.2, 300, 0.99, True)]
    flags = {"default": {}, "full-pass2": dict(ransac_pass2=1), "bounded-pass2": dict(ransac_pass2=2), "nolane": dict(ransac_nolane=1),
             "f64score": dict(ransac_f64score=1), "fused-tiled": dict(ransac_fused=1), "resident-f64": dict(ransac_resident_f64=1),
             "walk-no-handover": dict(ransac_pass2=2, ransac_bhand=1)}
    norefine = [s[:5] + (False,) for s in shapes]

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_ransac_workspace(s[0], s[3])

    def call(self, s, ws, ws_bytes, new):
        from test_gpu_ransac_bound import _dev_ransac
        p1, p2 = _ransac_scene(*s[:3])
        return _dev_ransac(p1, p2, _ransac_coef(*s[3:]), 31, ws=(ws, ws_bytes), alloc=new)

    def expect(self, s, got):
        from test_gpu_ransac_bound import _check
        ref = _ransac_ref(*s, 31)
        assert bool(ref["failed"]) == (s[4] > 0.9), "the premise of the scene"
        _check(got, got, ref)


# ---- pcreg_dev_ransac_batched ------------------------------------------------------------------------------------------
def ransac_batched_call(sizes, cap, iters, seed, ws, ws_bytes, new):
    """registration b = rigid_case(sizes[b], 700 + sizes[b]) -> per registration T, the counts and the inlier list"""
    from conftest import rigid_case
    from pcreg_amd._lib import DevRansacResult, RansacOpts, check, lib
    B = len(sizes)
    cases = [rigid_case(n, 700 + n, noise=0.05, outlier_frac=0.3) for n in sizes]
    off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ld = int(off_h[-1])
    p1 = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in cases]).T)).to(dev())
    p2 = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[1] for c in cases]).T)).to(dev())
    off = torch.from_numpy(off_h).to(dev())
    o = RansacOpts(3, iters, 0.1, 0.1, 1, 0, seed)
    res = new((B, C.sizeof(DevRansacResult)), torch.uint8); inl = new(ld, torch.int32)
    check(lib().pcreg_dev_ransac_batched(ptr(p1), ptr(p2), ld, ptr(off), B, cap, C.byref(o), ptr(res), ptr(inl), ptr(ws), C.c_size_t(ws_bytes),
                                         stream()))
    raw, inl_h = host(res), host(inl)
    out = []
    for b in range(B):
        r = DevRansacResult.from_buffer_copy(raw[b].tobytes())
        out.append(dict(T=np.array(r.T[:]), counts=np.array([r.n_inliers, r.num_success, r.max_inliers, r.failed, r.n, r.winner]),
                        inl=inl_h[off_h[b]:off_h[b] + r.n_inliers]))
    return out


@functools.lru_cache(maxsize=None)
def _batched_ref(n, iters, seed):
    from conftest import rigid_case
    p1, p2, _ = rigid_case(n, 700 + n, noise=0.05, outlier_frac=0.3)
    return oracle_c().ransac(p1, p2, dict(minPtNum=3, iterNum=iters, thDist=0.1, thInlrRatio=0.1, REFINE=True, VERBOSE=0), seed=seed)


@register
class RansacBatched(Case):
    """(n_cap, sizes): the fp32 launch plus the fp64 launch; tiled; one registration"""
    name, size_fn = "ransac_batched", "pcreg_dev_ransac_batched_workspace"
    shapes = [(3000, (500, 1500, 2500, 3000)), (4000, (1000, 4000, 2500)), (1000, (1000,))]
    ITERS, SEED = 500, 11

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_ransac_batched_workspace(s[0], self.ITERS, len(s[1]))

    def call(self, s, ws, ws_bytes, new):
        return ransac_batched_call(s[1], s[0], self.ITERS, self.SEED, ws, ws_bytes, new)

    def expect(self, s, got):
        for b, (n, r) in enumerate(zip(s[1], got)):
            ref = _batched_ref(n, self.ITERS, self.SEED + b)                      # (the built-in sampler is seeded seed + b)
            assert not ref["failed"] and r["counts"][3] == 0 and r["counts"][4] == n
            np.testing.assert_array_equal(r["inl"].astype(np.int64), ref["inlierIdx"])
            assert r["counts"][1] == ref["numSuccess"] and r["counts"][2] == ref["maxInliers"]
            assert np.linalg.norm(r["T"].reshape(4, 4, order="F") - ref["T"]) < 1e-5       # (T_TOL of tests/test_gpu_ransac.py)


# ---- pcreg_dev_get_matches ---------------------------------------------------------------------------------------------
PAR = dict(UNNORMALIZE=True, norm_factor=2, CHANGE_METRIC=True, metric_factor=0.6, Method="Approximate",
           MatchThreshold=20, MaxRatio=0.9, Metric="SAD", Unique=True, VERBOSE=0)


@functools.lru_cache(maxsize=None)
def count_descriptors(Q, M, D, seed):
    """count-like rows, the surface noisy copies of model rows.  With more surface rows than model rows the values are real: short
    rows of small counts are often permutations of one another, equidistant from a third row up to the rounding of the sums, and
    which of the two then wins the Unique back-check is decided by the last bit of two different pow functions (the device's
    and the host libm's: tests/test_gpu_sweep.py, test_segmented_metric_is_the_oracles_division_bit_for_bit).  With Poisson(3)
    counts at (4600, 600, 8), seed 2, exactly one of 596 pairs differed from the oracle's: model row 374 = (5 3 4 3 1 2 1 5)
    went to surface row 2618 = (6 3 4 3 1 2 1 5) on the device -- the certified path, "match_exact", the forced fallback and the
    host tier alike -- and to surface row 1484 = (5 3 4 3 1 2 1 6) in the oracle, which computes bit-equal distances for the two
    and takes the lower index."""
    rng = np.random.default_rng(seed)
    if M == 0:
        return rng.poisson(3.0, (Q, D)).astype(np.float64), np.zeros((0, D))
    if Q > M:
        dM = rng.gamma(3.0, 1.0, (M, D))
        return np.abs(dM[rng.choice(M, Q)] * (1.0 + 0.05 * rng.standard_normal((Q, D)))), dM
    dM = rng.poisson(3.0, (M, D)).astype(np.float64)
    return dM[rng.choice(M, Q, replace=False)] + rng.poisson(0.3, (Q, D)), dM


def get_matches_call(dS, dM, par, ws, ws_bytes, new):
    """feature-major operands -> the pairs (as the oracle's uint32) and their metric"""
    from pcreg_amd import _lib
    from pcreg_amd.api import _match_opts
    (Q, D), M = dS.shape, dM.shape[0]
    up = lambda d: torch.from_numpy(np.ascontiguousarray(d.T)).to(dev()) if len(d) else torch.zeros((d.shape[1], 1), dtype=torch.float64, device=dev())
    tS, tM = up(dS), up(dM)                                               # [D, Q]: feature-major (a set without rows: any address)
    o = _match_opts(par)
    pairs = new((Q, 2), torch.int32); metric = new(Q, torch.float64); n = new(1, torch.int32)
    _lib.check(_lib.lib().pcreg_dev_get_matches(ptr(tS), Q, Q, ptr(tM), M, M, D, _lib.LAYOUT_FEATURE_MAJOR, C.byref(o), ptr(pairs), ptr(metric),
                                                ptr(n), ptr(ws), C.c_size_t(ws_bytes), stream()))
    k = int(n.item())
    return dict(k=k, pairs=host(pairs[:k]).astype(np.uint32), metric=host(metric[:k]))


@register
class GetMatches(Case):
    """(Q, M, D, Unique): the existing shape; tiny; ragged against every tile; more surface rows than model rows with Unique (the
    back-search is sized by a count the call reads)"""
    name, size_fn = "get_matches", "pcreg_dev_get_matches_workspace"
    shapes = [(300, 900, 64, True), (3, 2, 5, True), (0, 900, 64, True), (257, 130, 33, True), (300, 0, 64, True), (4600, 600, 8, True),
              (300, 900, 64, False)]
    flags = {"default": {}, "match_exact": dict(match_exact=1), "forced-fallback": dict(match_force_fallback=1)}
    par = PAR

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_get_matches_workspace(*s[:3])

    def call(self, s, ws, ws_bytes, new):
        dS, dM = count_descriptors(s[0], s[1], s[2], 2)
        return get_matches_call(dS, dM, dict(self.par, Unique=s[3]), ws, ws_bytes, new)

    def expect(self, s, got):
        if s[0] == 0 or s[1] == 0:
            assert got["k"] == 0, "no rows on one side: n_pairs is 0 (and the guards show that no pair was written)"
            return
        np.testing.assert_array_equal(got["pairs"], _matches_ref(self.name, s))
        if s[0] >= 257 and self.par["Metric"] == "SAD":
            assert got["k"] > 0, "the premise: the shape matches something"


@functools.lru_cache(maxsize=None)
def _matches_ref(name, s):
    dS, dM = count_descriptors(s[0], s[1], s[2], 2)
    return oracle_c().getMatches(dS, dM, dict(CASES[name].par, Unique=s[3]))


@register
class GetMatchesSsd(GetMatches):
    name = "get_matches_ssd"
    shapes = [(300, 900, 64, True), (0, 900, 64, True), (3, 2, 5, True), (257, 130, 33, False)]
    flags = {"default": {}}
    par = dict(PAR, Metric="SSD", MatchThreshold=1.0)


# ---- pcreg_dev_get_matches_segmented, _prepared ------------------------------------------------------------------------
SEG_PAR = dict(PAR, MatchThreshold=10, MaxRatio=0.99)                      # (tests/test_gpu_sweep.py's)


@functools.lru_cache(maxsize=None)
def _seg_scene(kind):
    """-> descS, descM, rows_list, par: the scenes of tests/test_gpu_sweep.py"""
    if kind == "ragged":                              # test_segmented_get_matches_equals_one_call_per_segment
        rng = np.random.default_rng(11)
        VM, Q, D = 1500, 300, 120
        descM = rng.poisson(3.0, (VM, D)).astype(np.float64)
        pick = rng.choice(VM, Q, replace=False)
        descS = descM[pick] + rng.poisson(0.2, (Q, D))
        descS[5] = descS[4]
        descM[7] = 0.0
        rows = [np.sort(rng.choice(VM, 700, replace=False)), np.sort(rng.choice(VM, 130, replace=False)), np.array([7]), np.zeros(0, np.int64),
                np.arange(VM), np.sort(rng.choice(VM, 2, replace=False)), np.sort(pick[:200])]
        return descS, descM, rows, SEG_PAR
    if kind == "tied":                                # test_segmented_get_matches_with_many_tied_candidates, copies (20, 12)
        cm, cs = 20, 12
        rng = np.random.default_rng(33)
        D = 90
        base = rng.poisson(3.0, (40, D)).astype(np.float64)
        descM = np.repeat(base, cm, axis=0)[rng.permutation(40 * cm)]
        descS = np.repeat(base[:25] + rng.poisson(0.1, (25, D)), cs, axis=0)[rng.permutation(25 * cs)]
        VM = descM.shape[0]
        rows = [np.arange(VM), np.sort(rng.choice(VM, VM // 2, replace=False)), np.sort(rng.choice(VM, 5, replace=False))]
        return descS, descM, rows, dict(SEG_PAR, MatchThreshold=50.0, MaxRatio=1.0)
    if kind == "none":                                # S = 0 on the ragged scene's descriptors
        descS, descM, _, par = _seg_scene("ragged")
        return descS, descM, [], par
    if kind == "long_surface":                        # test_segmented_get_matches_other_shapes
        rng = np.random.default_rng(21)
        VM, Q, D = 2600, 2300, 24
        descM = rng.poisson(3.0, (VM, D)).astype(np.float64)
        descS = descM[rng.choice(VM, Q, replace=False)] + rng.poisson(0.2, (Q, D))
        rows = [np.sort(rng.choice(VM, VM // 2, replace=False)), np.arange(VM), np.sort(rng.choice(VM, 70, replace=False))]
        return descS, descM, rows, SEG_PAR
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _seg_ref(kind):
    from test_gpu_sweep import _oracle_get_matches_with_metric
    oracle_c()
    descS, descM, rows, par = _seg_scene(kind)
    return [_oracle_get_matches_with_metric(descS, descM[r], par) if len(r) else None for r in rows]


def _seg_dims(kind):
    descS, descM, rows, _ = _seg_scene(kind)
    return descS.shape[0], descM.shape[0], descS.shape[1], len(rows), sum(len(r) for r in rows), max([len(r) for r in rows] + [0])


def _seg_expect(kind, got):
    """the pairs are the oracle's, bit for bit; the metric within the bound tests/test_gpu_sweep.py holds it to where the powered
    rows come from two different pow functions"""
    ref = _seg_ref(kind)
    assert len(got) == len(ref)
    for z, (g, r) in enumerate(zip(got, ref)):
        if r is None:
            assert g[0].shape[0] == 0, f"segment {z}"
            continue
        np.testing.assert_array_equal(g[0], r[0], err_msg=f"segment {z}")
        np.testing.assert_allclose(g[1], r[1], rtol=1e-12, atol=1e-14)


@register
class Segmented(Case):
    name, size_fn = "get_matches_segmented", "pcreg_dev_get_matches_segmented_workspace"
    shapes = ["ragged", "tied", "none", "long_surface"]
    flags = {"default": {}, "seg_batched": dict(seg_batched=1), "seg_wave_finalize": dict(seg_wave_finalize=1),
             "forced-fallback-1": dict(match_force_fallback=1), "forced-fallback-2": dict(match_force_fallback=2)}

    def need(self, kind):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_get_matches_segmented_workspace(*_seg_dims(kind))

    def call(self, kind, ws, ws_bytes, new):
        from test_gpu_sweep import _segments_direct
        descS, descM, rows, par = _seg_scene(kind)
        return [list(z) for z in _segments_direct(descS, descM, rows, par, metric=True, ws=(ws, ws_bytes), alloc=new)]

    def expect(self, kind, got):
        _seg_expect(kind, got)

    def shapes_for(self, flag):
        """"seg_batched" forces the bounded-workspace form into a workspace of the one-chain size: the fixed head, the gathered
        sub-model and a batch's one-chain workspace must fit where one chain does.  The ragged scene fits (the existing test runs
        it so); the tied scene and the long surface, whose largest segment is the whole model against as many or more queries,
        do not, and are refused with PCREG_E_WORKSPACE as the header says of a segment that does not fit the bound."""
        return ["ragged", "none"] if flag == "seg_batched" else list(self.shapes)

    def untouched(self, kind, bufs):
        assert (inner(bufs, 2) >= 0).all(), "n_pairs of every segment is written"


@register
class SegmentedPrepared(Segmented):
    """the same scenes through a model prepared with OTHER options than the call's (metric_factor 0.8): the call makes its own
    powered rows, and leaves none behind for the next"""
    name = "get_matches_segmented_prepared"
    flags = {"default": {}, "forced-fallback-1": dict(match_force_fallback=1)}
    _prep = {}

    def _prepared(self, kind):
        from pcreg_amd._lib import check, lib
        from pcreg_amd.api import _match_opts
        descS, descM, _, par = _seg_scene(kind)
        key = id(descM)
        if key not in self._prep:
            VM, D = descM.shape
            dM = torch.from_numpy(descM).to(dev())
            o = _match_opts(dict(par, metric_factor=0.8))
            nb = lib().pcreg_dev_segmented_model_bytes(VM, D)
            prep = torch.empty(nb, dtype=torch.uint8, device=dev())
            check(lib().pcreg_dev_segmented_model_prepare(ptr(dM), VM, D, C.byref(o), ptr(prep), C.c_size_t(nb), stream()))
            torch.cuda.synchronize()
            self._prep[key] = (dM, prep, o, host(prep).copy())
        return self._prep[key]

    def call(self, kind, ws, ws_bytes, new):
        from pcreg_amd._lib import check, lib
        from pcreg_amd.api import _match_opts
        descS, descM, rows_list, par = _seg_scene(kind)
        dM, prep, o_prep, prep_bytes = self._prepared(kind)
        Q, VM, D, S, tot, n_max = _seg_dims(kind)
        off = np.zeros(S + 1, dtype=np.int32); off[1:] = np.cumsum([len(r) for r in rows_list])
        dS = torch.from_numpy(np.ascontiguousarray(descS)).to(dev())
        rows = torch.from_numpy(np.concatenate([np.asarray(r, np.int32) for r in rows_list] + [np.zeros(1, np.int32)])).to(dev())
        seg_off = torch.from_numpy(off).to(dev())
        o = _match_opts(par)
        pairs = new((S, Q, 2), torch.int32); met = new((S, Q), torch.float64); n_pairs = new(S, torch.int32)
        check(lib().pcreg_dev_get_matches_segmented_prepared(ptr(dS), Q, ptr(dM), VM, D, ptr(prep), int(o_prep.change_metric),
                                                             C.c_double(o_prep.metric_factor), ptr(rows), ptr(seg_off), S, tot, n_max, C.byref(o),
                                                             ptr(pairs), ptr(met), ptr(n_pairs), ptr(ws), C.c_size_t(ws_bytes), stream()))
        n = host(n_pairs); ph = host(pairs).astype(np.uint32); mh = host(met)
        same_bits(host(prep), prep_bytes, "the prepared model is read-only")
        return [[ph[z, :n[z]], mh[z, :n[z]]] for z in range(S)]


# ---- pcreg_dev_spatial_histogram_descriptors ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _desc_scene(P, S, align, min_pts):
    from test_gpu_descriptors import OPT, keypoints, strips
    return strips(P, 0), keypoints(S, 1), dict(OPT, ALIGN_POINTS=align, min_pts=min_pts)


@functools.lru_cache(maxsize=None)
def _desc_ref(s):
    return oracle_c().getSpacialHistogramDescriptors(*_desc_scene(*s))


def descriptors_call(pts_h, kp_h, opt, ws, ws_bytes, new):
    from pcreg_amd._lib import check, lib
    from pcreg_amd.api import _desc_opts
    from pcreg_amd.device import soa
    pts = soa(torch.from_numpy(pts_h).to(dev())); kp = soa(torch.from_numpy(kp_h).to(dev()))
    P, S = pts.shape[1], kp.shape[1]
    o = _desc_opts(opt)
    feat = new((S, 3), torch.float64); desc = new((S, 980), torch.float64); counters = new(2, torch.int32)
    check(lib().pcreg_dev_spatial_histogram_descriptors(ptr(pts), P, pts.stride(0), ptr(kp), S, kp.stride(0), C.byref(o), ptr(feat), ptr(desc),
                                                        ptr(counters), ptr(ws), C.c_size_t(ws_bytes), stream()))
    V = int(counters[0].item())
    return dict(counters=host(counters), feat=host(feat[:V]), desc=host(desc[:V]))


@register
class Descriptors(Case):
    """(P, S, ALIGN_POINTS, min_pts): the existing shape; a small one with ALIGN_POINTS flipped; a minimum no keypoint survives"""
    name, size_fn = "descriptors", "pcreg_dev_spatial_histogram_descriptors_workspace"
    shapes = [(40000, 300, True, 150), (12000, 40, False, 100), (12000, 40, True, 10 ** 6)]

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_spatial_histogram_descriptors_workspace(s[0], s[1])

    def call(self, s, ws, ws_bytes, new):
        return descriptors_call(*_desc_scene(*s), ws, ws_bytes, new)

    def expect(self, s, got):
        rfeat, rdesc = _desc_ref(s)
        assert (len(rfeat) > 50) if s[3] == 150 else (len(rfeat) == 0) == (s[3] > 1000)
        assert got["counters"][0] == len(rfeat) and got["counters"][1] == 0
        np.testing.assert_array_equal(got["feat"], rfeat)
        np.testing.assert_array_equal(got["desc"], rdesc)


# ---- the point searches: pcreg_dev_knn2_points_f32, pcreg_dev_model_search_f32 (+ _match_f32), _knn_f32, _range_* ------------
@functools.lru_cache(maxsize=None)
def _points(M, Q, seed):
    rng = np.random.default_rng(seed)
    model = (rng.random((M, 3)) * [100, 56, 99]).astype(np.float32)
    surf = (model[rng.choice(M, Q, replace=Q > M)] + rng.normal(0, 0.05, (Q, 3))).astype(np.float32)
    return model, surf


_PREPARED = {}


def prepared(key, make):
    """one PreparedModel per model of the registry, kept for the session: every case and every handle check shares it"""
    if key not in _PREPARED:
        from pcreg_amd.device import PreparedModel
        t = soa32(make())
        _PREPARED[key] = (PreparedModel(t), t)
    return _PREPARED[key][0]


def _search_model(M):
    return prepared(("points", M), lambda: _points(M, min(M, 3000), 3)[0])


@functools.lru_cache(maxsize=None)
def _knn_ref(M, Q, k):
    import knn_k_ref
    model, surf = _points(M, Q, 3)
    return knn_k_ref.knn(surf, model, k, threads=8)


def _knn_expect(M, Q, k, idx, dist):
    """the brute-force fp32 reference, bit for bit; past M rows: -1 and +inf"""
    ri, rd = _knn_ref(M, Q, min(k, M))
    np.testing.assert_array_equal(idx[:, :min(k, M)], ri)
    np.testing.assert_array_equal(dist[:, :min(k, M)].view(np.uint32), rd.view(np.uint32))
    assert (idx[:, M:] == -1).all() and np.isposinf(dist[:, M:]).all()


@register
class Knn2Points(Case):
    """(M, Q): the model given as points, no handle"""
    name, size_fn = "knn2_points", "pcreg_dev_knn2_points_f32_workspace"
    shapes = [(50000, 3000), (50000, 1100), (50000, 1), (5, 3000)]
    flags = {"default": {}, "knn_exact": dict(knn_exact=1), "knn_nocull": dict(knn_nocull=1)}

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_knn2_points_f32_workspace(s[1], s[0])

    def call(self, s, ws, ws_bytes, new):
        from pcreg_amd._lib import check, lib
        M, Q = s
        model, surf = _points(M, Q, 3)
        m, q = soa32(model), soa32(surf)
        idx = new((Q, 2), torch.int32); dist = new((Q, 2), torch.float32)
        check(lib().pcreg_dev_knn2_points_f32(ptr(q), Q, Q, ptr(m), M, M, C.c_int32(0), ptr(idx), ptr(dist), ptr(ws), C.c_size_t(ws_bytes), stream()))
        return [host(idx), host(dist)]

    def expect(self, s, got):
        _knn_expect(s[0], s[1], 2, *got)


@register
class ModelSearch(Case):
    """(M, Q): the top-2 search of a prepared model, then pcreg_dev_model_match_f32 on the same workspace, as the header prescribes"""
    name, size_fn = "model_search", "pcreg_dev_model_search_workspace"
    shapes = [(50000, 3000), (50000, 1100), (50000, 1), (5, 3000)]
    flags = {"default": {}, "tile-walk": dict(knn_direct=1), "seed-then-direct": dict(knn_seed_fused=1), "knn_nocull": dict(knn_nocull=1)}
    THR, RATIO = np.float32(0.25), np.float32(0.8)

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_model_search_workspace(s[1], s[0])

    def call(self, s, ws, ws_bytes, new):
        from pcreg_amd._lib import check, lib
        M, Q = s
        pm = _search_model(M)
        q = soa32(_points(M, Q, 3)[1])
        idx = new((Q, 2), torch.int32); dist = new((Q, 2), torch.float32)
        check(lib().pcreg_dev_model_search_f32(pm.handle, ptr(q), Q, Q, C.c_int32(0), ptr(idx), ptr(dist), ptr(ws), C.c_size_t(ws_bytes), stream()))
        pairs = new((Q, 2), torch.int32); n = new(1, torch.int32)
        check(lib().pcreg_dev_model_match_f32(pm.handle, ptr(q), Q, Q, ptr(idx), ptr(dist), C.c_float(self.THR), C.c_float(self.RATIO), 1, ptr(ws),
                                              C.c_size_t(ws_bytes), ptr(pairs), None, None, ptr(n), stream()))
        k = int(n.item())
        return dict(idx=host(idx), dist=host(dist), pairs=host(pairs[:k]).astype(np.uint32))

    def expect(self, s, got):
        _knn_expect(s[0], s[1], 2, got["idx"], got["dist"])
        if s[0] > 5:
            model, surf = _points(*s, 3)
            np.testing.assert_array_equal(got["pairs"], oracle_c().match_points_f32(surf, model, float(self.THR), float(self.RATIO), True))


@register
class ModelKnn(Case):
    """(M, Q, k)"""
    name, size_fn = "model_knn", "pcreg_dev_model_knn_workspace"
    shapes = [(50000, 3000, 8), (50000, 3000, 1), (50000, 70, 32), (50000, 70, 8), (5, 70, 8)]
    flags = {"default": {}, "knn_tail_cap": dict(knn_tail_cap=64), "knn_nocull": dict(knn_nocull=1)}

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_model_knn_workspace(s[1], s[0], s[2])

    def call(self, s, ws, ws_bytes, new):
        M, Q, k = s
        idx = new((Q, k), torch.int32); dist = new((Q, k), torch.float32)
        _search_model(M).knn(soa32(_points(M, Q, 3)[1]), k, out=(idx, dist, ws[:max(ws_bytes, 1)]))
        return [host(idx), host(dist)]

    def expect(self, s, got):
        _knn_expect(s[0], s[1], s[2], *got)


@functools.lru_cache(maxsize=None)
def _range_ref(M, Q, r2):
    import range_ref
    model, surf = _points(M, Q, 3)
    return range_ref.rangesearch(surf, model, np.float32(r2), threads=8)


@register
class ModelRange(Case):
    """(M, Q, r2): a count and then a fill; the two share nothing but the workspace's address (the fill is told the count's seg_off)"""
    name, size_fn = "model_range", "pcreg_dev_model_range_workspace"
    shapes = [(50000, 3000, 9.0), (50000, 3000, 0.0), (50000, 40, float("inf")), (50000, 1100, 9.0)]
    flags = {"default": {}, "range_sort_cap": dict(range_sort_cap=8)}

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_model_range_workspace(s[1], s[0])

    def call(self, s, ws, ws_bytes, new):
        M, Q, r2 = s
        pm, q = _search_model(M), soa32(_points(M, Q, 3)[1])
        counts = new(Q, torch.int32); seg_off = new(Q + 1, torch.int64)
        pm.rangesearch_count(q, r2, out=(counts, seg_off, ws[:ws_bytes]))
        total = int(seg_off[-1].item())
        ws[:ws_bytes].fill_(0xFF)                      # the fill forms its own query order: it may use nothing the count left
        idx = new(total, torch.int32); dist = new(total, torch.float32)
        pm.rangesearch_fill(q, r2, seg_off, idx, dist, ws=ws[:ws_bytes])
        return dict(counts=host(counts), seg_off=host(seg_off), idx=host(idx), dist=host(dist))

    def expect(self, s, got):
        rso, ri, rd = _range_ref(*s)
        np.testing.assert_array_equal(got["seg_off"], rso)
        np.testing.assert_array_equal(got["counts"], np.diff(rso))
        np.testing.assert_array_equal(got["idx"], ri)
        np.testing.assert_array_equal(got["dist"].view(np.uint32), rd.view(np.uint32))


# ---- pcreg_dev_sphere_select ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere_feat(V):
    return np.random.default_rng(5).uniform([0, 0, 0], [40, 30, 20], (V, 3))


def sphere_select_call(feat_h, centre, R, ws, ws_bytes, new):
    from pcreg_amd._lib import check, lib
    V = len(feat_h)
    feat = torch.from_numpy(feat_h).to(dev()) if V else torch.zeros((1, 3), dtype=torch.float64, device=dev())
    idx = new(V, torch.int32); n = new(1, torch.int32)
    check(lib().pcreg_dev_sphere_select(ptr(feat), V, (C.c_double * 3)(*centre), C.c_double(R), ptr(idx), ptr(n), ptr(ws), C.c_size_t(ws_bytes),
                                        stream()))
    k = int(n.item())
    return dict(k=k, idx=host(idx[:k]))


@register
class SphereSelect(Case):
    """(V, R): the existing shape; a tenth of it; a radius that holds no row"""
    name, size_fn = "sphere_select", "pcreg_dev_sphere_select_workspace"
    shapes = [(6000, 8.0), (600, 8.0), (6000, 0.0)]
    CENTRE = (22.0, 14.0, 9.0)

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_sphere_select_workspace(s[0])

    def call(self, s, ws, ws_bytes, new):
        return sphere_select_call(_sphere_feat(s[0]), self.CENTRE, s[1], ws, ws_bytes, new)

    def expect(self, s, got):
        from oracle.pcreg_oracle import getDescriptorMask
        want = np.flatnonzero(getDescriptorMask(_sphere_feat(s[0]), self.CENTRE, s[1])).astype(np.int32)
        assert (100 < len(want) < s[0]) or s[1] == 0.0 or s[0] < 1000
        np.testing.assert_array_equal(got["idx"], want)

    def untouched(self, s, bufs):
        k = int(inner(bufs, 1)[0])
        assert 0 < k < s[0]


# ---- candidate transforms against a prepared model: score, the four refits, and the NDT refit ----------------------------------
def t16(T):
    """[B, 4, 4] -> the [B, 16] block on the device, each transform column-major"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    return torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)).to(dev())


def m44(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))


R15 = np.float32(1.5) ** 2
_TORCH = {np.int32: torch.int32, np.float64: torch.float64}


def _scene_model():
    import plane_ref
    return prepared("plane_ref.scene", lambda: plane_ref.scene()["model"])


class _Refit(Case):
    """What the refits share.  A shape is (name, steps): "full", the six candidates of plane_ref.scene() (four rigid ones, the empty
    transform and one with a NaN entry) on its 2500 queries; "one", the first candidate on three queries; "dead", the empty and the
    NaN candidate alone.  steps = 3 alternates T_tmp and T_out.  Under "batches" the transforms go through in three batches."""
    shapes = [("full", 1), ("one", 1), ("dead", 1), ("full", 3)]
    flags = {"default": {}, "batches": dict(score_batch_slots=5000)}
    kinds = ()                     # the dtypes of the [B] outputs behind T_out and T_step

    def inputs(self, s):
        import plane_ref
        sc = plane_ref.scene()
        T, surf = sc["T"], sc["surf"]
        return {"full": (T, surf), "one": (T[:1], surf[:3]), "dead": (T[4:], surf)}[s[0]]

    def need(self, s):
        from pcreg_amd._lib import lib
        T, surf = self.inputs(s)
        return getattr(lib(), self.size_fn)(len(surf), len(T), _scene_model().M)

    def call(self, s, ws, ws_bytes, new):
        T, surf = self.inputs(s)
        return self.run_steps(T, surf, s[1], ws, ws_bytes, new)

    def run_steps(self, T, surf, steps, ws, ws_bytes, new, **more):
        B = len(T)
        out = [new((B, 16), torch.float64), new((B, 16), torch.float64)] + [new(B, _TORCH[k]) for k in self.kinds]
        tmp = new((B, 16), torch.float64) if steps > 1 else None
        self.invoke(_scene_model(), soa32(surf), t16(T), steps, tuple(out) + (ws[:ws_bytes], tmp), **more)
        torch.cuda.synchronize()
        return [m44(host(out[0])), m44(host(out[1]))] + [host(t) for t in out[2:]]

    def expect(self, s, got):
        """one step: the operation's own comparator against its reference's step on these inputs.  Three steps: the same call as three
        single steps on fresh workspaces, each fed the transforms the step before it returned and each held to the reference's
        step on exactly those transforms (the references step from the DEVICE's intermediate transforms); the third single step's
        outputs are the three-step call's, bit for bit."""
        T, surf = self.inputs(s)
        if s[1] == 1:
            self.compare(s, got, T, surf)
            return
        cur, one, more = T, None, {}
        for step in range(s[1]):
            outs = Outputs()
            one = self.run_steps(cur, surf, 1, workspace(self.need((s[0], 1)), 0x00), int(self.need((s[0], 1))), outs.new, **more)
            outs.check_guards(f"{self.name} single step {step}")
            more = self.single_step_check((s[0], 1, step), one, cur, surf)
            cur = one[0]
        same_bits(got, one, f"{self.name}: three steps against three single steps")
        assert got[-1].tolist() == [0, 0, 0, 0, 1, 1]

    def single_step_check(self, key, one, cur, surf):
        """holds one step of a chain to the reference; -> what the next single step must be given beside the transforms"""
        self.compare(key, one, cur, surf)
        return {}


@register
class RefitRigid(_Refit):
    name, size_fn = "model_refit", "pcreg_dev_model_refit_workspace"
    kinds = (np.int32, np.float64, np.int32)

    def invoke(self, pm, q, Td, steps, out):
        pm.refit_transforms(q, Td, R15, steps=steps, out=out)

    def compare(self, s, got, T, surf):
        import plane_ref
        import refit_ref
        from test_gpu_refit import _check
        model = plane_ref.scene()["model"]
        _check(tuple(got), T, _cached(self.name, s, lambda: refit_ref.step(surf, model, T, R15, threads=8)), model, R15, str(s))


_REFS = {}


def _cached(name, s, make):
    if (name, s) not in _REFS:
        _REFS[(name, s)] = make()
    return _REFS[(name, s)]


@register
class RefitPlane(_Refit):
    name, size_fn = "model_refit_plane", "pcreg_dev_model_refit_plane_workspace"
    kinds = (np.int32, np.float64, np.int32, np.float64, np.int32)

    def invoke(self, pm, q, Td, steps, out):
        import plane_ref
        pm.refit_plane(q, Td, R15, soa32(plane_ref.scene()["normals"]), steps=steps, out=out)

    def compare(self, s, got, T, surf):
        import plane_ref
        from test_gpu_refit_plane import _check
        sc = plane_ref.scene()
        _check(tuple(got), T, _cached(self.name, s, lambda: plane_ref.step(surf, sc["model"], sc["normals"], T, R15, threads=8)), str(s))


@register
class RefitGicp(_Refit):
    name, size_fn = "model_refit_gicp", "pcreg_dev_model_refit_gicp_workspace"
    kinds = (np.int32, np.float64, np.int32, np.float64, np.int32)

    def invoke(self, pm, q, Td, steps, out):
        import gicp_ref
        import plane_ref
        Q = q.shape[1]
        pm.refit_gicp(q, Td, R15, soa32(plane_ref.scene()["normals"]), soa32(gicp_ref.surface_normals()[:Q]), steps=steps, out=out)

    def compare(self, s, got, T, surf):
        import gicp_ref
        import plane_ref
        from test_gpu_refit_gicp import _check
        sc = plane_ref.scene()
        sn = gicp_ref.surface_normals()[:len(surf)]
        _check(tuple(got), T, _cached(self.name, s, lambda: gicp_ref.step(surf, sc["model"], sc["normals"], sn, T, R15, threads=8)), str(s))


@register
class RefitCpd(_Refit):
    """sigma2 = 1, w = 0.1: one of the main scene's cases of tests/test_gpu_cpd.py"""
    name, size_fn = "model_refit_cpd", "pcreg_dev_model_refit_cpd_workspace"
    kinds = (np.float64, np.float64, np.float64, np.float64, np.int32, np.int32)

    def invoke(self, pm, q, Td, steps, out, sigma2=1.0):
        pm.refit_cpd(q, Td, sigma2=sigma2, outlier=0.1, steps=steps, out=out)

    def single_step_check(self, key, one, cur, surf):
        """a later step takes the variance the step before it returned, per candidate; the reference (one variance for all
        candidates) is compared at the first step only"""
        if key[2] == 0:
            self.compare(key, one, cur, surf)
        return dict(sigma2=torch.from_numpy(np.ascontiguousarray(one[2])).to(dev()))

    def compare(self, s, got, T, surf):
        import cpd_ref
        import plane_ref
        from test_gpu_cpd import _check
        model = plane_ref.scene()["model"]
        ld, s32 = _cached(self.name, s, lambda: (cpd_ref.step_ld(surf, model, T, 1.0, 0.1), cpd_ref.step32(surf, model, T, 1.0, 0.1)))
        _check(tuple(got), T, ld, s32, str(s))


@register
class NdtRefit(_Refit):
    name, size_fn = "ndt_refit", "pcreg_dev_ndt_refit_workspace"
    kinds = (np.int32, np.float64, np.int32)
    flags = {"default": {}}
    STEP = 4.0
    _nm = []

    def model(self):
        if not self._nm:
            import plane_ref
            from pcreg_amd.device import NdtModel
            self._nm.append(NdtModel(soa32(plane_ref.scene()["model"]), self.STEP, 6))
        return self._nm[0]

    def need(self, s):
        from pcreg_amd._lib import lib
        T, surf = self.inputs(s)
        return lib().pcreg_dev_ndt_refit_workspace(len(surf), len(T))

    def invoke(self, pm, q, Td, steps, out):
        self.model().refit(q, Td, steps=steps, out=out)

    def compare(self, s, got, T, surf):
        import ndt_ref
        import plane_ref
        from test_gpu_ndt import _check
        tab = _cached(self.name, "table", lambda: ndt_ref.table(plane_ref.scene()["model"], self.STEP, 6))
        _check(tuple(got), T, _cached(self.name, s, lambda: ndt_ref.step(surf, tab, T)), str(s))


@register
class ModelScore(Case):
    """(candidates, queries) of tests/test_gpu_score.py's "synth" case: all eight transforms on its 3000 queries; one on three; the
    empty and the NaN transform alone"""
    name, size_fn = "model_score", "pcreg_dev_model_score_workspace"
    shapes = [((0, 8), 3000), ((1, 2), 3), ((6, 8), 3000)]
    flags = {"default": {}, "batches": dict(score_batch_slots=7000), "knn_nocull": dict(knn_nocull=1)}

    def scene(self):
        from test_gpu_score import _case
        return _case("synth")

    def model(self):
        return prepared("score.synth", lambda: self.scene()[0])

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_model_score_workspace(s[1], s[0][1] - s[0][0], self.model().M)

    def call(self, s, ws, ws_bytes, new):
        _, surf, T, _ = self.scene()
        (b0, b1), Q = s
        B = b1 - b0
        out = (new(B, torch.int32), new(B, torch.float64), new((B, Q), torch.int32), new((B, Q), torch.float32))
        self.model().score_transforms(soa32(surf[:Q]), t16(T[b0:b1]), R15, rows=True, out=out + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return [host(t) for t in out]

    def expect(self, s, got):
        from test_gpu_score import _check
        _, surf, T, nn = self.scene()
        (b0, b1), Q = s
        assert len(surf) == 3000 and len(T) == 8
        pick = lambda a: np.ascontiguousarray(np.asarray(a).reshape(8, 3000)[b0:b1, :Q]).reshape(-1)
        _check(tuple(got), (pick(nn[0]), pick(nn[1])), R15, Q)


# ---- operations over a prepared model's own rows ------------------------------------------------------------------------------
class _SelfJoin(Case):
    """A shape is (M, ...): the first M rows of the operation's family cloud -- its existing test's M, 513 (one row past a tile), 3,
    and 0 where the header allows a model without rows.  One PreparedModel per (cloud, M), shared by every check."""
    cloud_key = None

    def cloud(self, M):
        raise NotImplementedError

    def model(self, M):
        return prepared((self.cloud_key or self.name, M), lambda: self.cloud(M))

    def sized(self, *args):
        from pcreg_amd._lib import lib
        return getattr(lib(), self.size_fn)(*args)

    def need(self, s):
        return self.sized(s[0])


def _sheet(M):
    import normals_ref
    return normals_ref.family("sheet")[:M]


@functools.lru_cache(maxsize=None)
def _sheet_normals(M, k=8):
    """the reference's normals of the first M rows of the sheet, oriented by the contract's rule (rows without one: NaN)"""
    import normals_ref
    model = _sheet(M)
    if M < 3:
        return np.full((M, 3), np.nan, np.float32)
    return normals_ref.oriented(normals_ref.normals(model, min(k, M)), model).astype(np.float32)


@register
class ModelCluster(_SelfJoin):
    """(M, radius) on the lattice cloud of tests/dbscan_ref.py"""
    name, size_fn, cloud_key = "model_cluster", "pcreg_dev_model_cluster_workspace", "lattice"
    shapes = [(4100, 1.5), (513, 1.5), (4100, 0.0), (3, 1.5), (0, 1.5)]
    flags = {"default": {}, "cluster_noskip": dict(cluster_noskip=1), "knn_nocull": dict(knn_nocull=1)}

    def cloud(self, M):
        import dbscan_ref
        return dbscan_ref.lattice_cloud(500 + 4100, 4100)[:M]

    def call(self, s, ws, ws_bytes, new):
        M = s[0]
        out = (new(M, torch.int32), new(1, torch.int32), new(M, torch.int32), new(M, torch.int32))
        self.model(M).cluster(np.float32(s[1]) ** 2, out=out + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return [host(out[0]), int(out[1].item()), host(out[2]), host(out[3])]

    def expect(self, s, got):
        import cluster_ref
        from test_gpu_cluster import _equal_ref
        if s[0]:
            _equal_ref(tuple(got), _cached(self.name, s, lambda: cluster_ref.cluster(self.cloud(s[0]), np.float32(s[1]) ** 2)), str(s))
        else:
            assert got[1] == 0


@register
class ModelDbscan(ModelCluster):
    """(M, radius, minpts)"""
    name, size_fn = "model_dbscan", "pcreg_dev_model_dbscan_workspace"
    shapes = [(4100, 1.5, 4), (513, 1.5, 4), (4100, 1.0, 12), (3, 1.5, 1), (0, 1.5, 4)]

    def call(self, s, ws, ws_bytes, new):
        from test_gpu_dbscan import KEYS
        M = s[0]
        out = (new(M, torch.int32), new(1, torch.int32), new(M, torch.uint8), new(M, torch.int32), new(M, torch.int32), new(M, torch.int32))
        self.model(M).dbscan(np.float32(s[1]) ** 2, s[2], out=out + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        got = {k: host(v) for k, v in zip(KEYS, out)}
        got["n_clusters"] = int(got["n_clusters"][0])
        return got

    def expect(self, s, got):
        import dbscan_ref
        from test_gpu_dbscan import _equal_ref
        if s[0]:
            _equal_ref(got, _cached(self.name, s, lambda: dbscan_ref.dbscan(self.cloud(s[0]), np.float32(s[1]) ** 2, s[2])), str(s))
        else:
            assert got["n_clusters"] == 0


@register
class ModelNormals(_SelfJoin):
    """(M, k)"""
    name, size_fn, cloud_key = "model_normals", "pcreg_dev_model_normals_workspace", "sheet"
    shapes = [(2048, 8), (513, 32), (2048, 3), (3, 3)]
    flags = {"default": {}, "knn_nocull": dict(knn_nocull=1)}
    cloud = staticmethod(_sheet)

    def need(self, s):
        return self.sized(*s)

    def call(self, s, ws, ws_bytes, new):
        M, k = s
        nrm, var = new((3, M), torch.float32), new(M, torch.float32)
        self.model(M).normals(k, variation=True, out=(nrm, var, ws[:ws_bytes]))
        torch.cuda.synchronize()
        return [np.ascontiguousarray(host(nrm).T), host(var)]

    def expect(self, s, got):
        import normals_ref
        from test_gpu_normals import _check_against
        _check_against(got[0], got[1], _cached(self.name, s, lambda: normals_ref.normals(_sheet(s[0]), s[1])), str(s))


@register
class ModelDenoise(_SelfJoin):
    """(M, k, threshold)"""
    name, size_fn = "model_denoise", "pcreg_dev_model_denoise_workspace"
    shapes = [(2048, 4, 1.0), (513, 31, 1.0), (2048, 1, 0.0), (3, 2, 1.0)]
    flags = {"default": {}, "knn_nocull": dict(knn_nocull=1)}

    def cloud(self, M):
        import denoise_ref
        return denoise_ref.family("sheet")[:M]

    def need(self, s):
        return self.sized(s[0], s[1])

    def call(self, s, ws, ws_bytes, new):
        M, k, t = s
        md, inl, n_inl, stats = new(M, torch.float64), new(M, torch.int32), new(1, torch.int32), new(4, torch.float64)
        self.model(M).denoise(k, t, out=(md, inl, n_inl, stats, ws[:ws_bytes]))
        torch.cuda.synchronize()
        return dict(mean_dist=host(md), inliers=host(inl)[:int(n_inl.item())], stats=host(stats))

    def expect(self, s, got):
        import denoise_ref
        from test_gpu_denoise import _check_against
        _check_against(got, _cached(self.name, s, lambda: denoise_ref.denoise(self.cloud(s[0]), s[1], s[2])), s[1], s[2], str(s))


@register
class ModelFps(_SelfJoin):
    """(M, K)"""
    name, size_fn = "model_fps", "pcreg_dev_model_fps_workspace"
    shapes = [(4000, 300), (513, 600), (4000, 1), (3, 2), (0, 5)]

    def cloud(self, M):
        import fps_ref
        return fps_ref.family("surface", 4000)[:M]

    def need(self, s):
        return self.sized(*s)

    def call(self, s, ws, ws_bytes, new):
        M, K = s
        out = (new(K, torch.int32), new(K, torch.float32), new(1, torch.int32), new(1, torch.float32), new(M, torch.float32), new(M, torch.int32),
               new(1, torch.int32))
        self.model(M).farthest_points(K, out=out + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        n = int(out[2].item())
        return dict(idx=host(out[0])[:n], dist=host(out[1])[:n], n_out=n, cover_d2=host(out[3]), min_dist=host(out[4]), label=host(out[5]),
                    info=host(out[6]))

    def expect(self, s, got):
        import fps_ref
        want = _cached(self.name, s, lambda: fps_ref.fps(self.cloud(s[0]), s[1]))
        assert got["n_out"] == want["n_out"] == min(s) and got["info"][0] == want["info"] == 0
        np.testing.assert_array_equal(got["idx"], want["idx"])
        same_bits(got["dist"], np.asarray(want["dist"], np.float32), "dist")
        if s[0]:
            same_bits(got["cover_d2"], np.asarray(want["cover_d2"], np.float32).reshape(1), "cover_d2")
            same_bits(got["min_dist"], np.asarray(want["min_dist"], np.float32), "min_dist")
            np.testing.assert_array_equal(got["label"], want["label"])


@register
class ModelFpfh(_SelfJoin):
    """(M, k)"""
    name, size_fn, cloud_key = "model_fpfh", "pcreg_dev_model_fpfh_workspace", "sheet"
    shapes = [(2048, 8), (513, 32), (2048, 3), (3, 3)]
    flags = {"default": {}, "knn_nocull": dict(knn_nocull=1)}
    cloud = staticmethod(_sheet)

    def need(self, s):
        return self.sized(*s)

    def call(self, s, ws, ws_bytes, new):
        M, k = s
        desc, cnt = new((M, 33), torch.float64), new((M, 33), torch.uint8)
        self.model(M).fpfh(k, soa32(_sheet_normals(M)), spfh=True, out=(desc, cnt, ws[:ws_bytes]))
        torch.cuda.synchronize()
        return [host(desc), host(cnt)]

    def expect(self, s, got):
        import fpfh_ref
        from test_gpu_fpfh import _check_against
        _check_against(got[0], got[1], _cached(self.name, s, lambda: fpfh_ref.fpfh(_sheet(s[0]), _sheet_normals(s[0]), s[1])), str(s))


@register
class ModelFpfhRadius(_SelfJoin):
    """(M, radius, max_neighbors): the count on a workspace of fpfh_radius_workspace(M, 0) bytes, one read of the total, the second
    call on one of fpfh_radius_workspace(M, total) bytes at the same address"""
    name, size_fn, cloud_key = "model_fpfh_radius", "pcreg_dev_model_fpfh_radius_workspace", "sheet"
    shapes = [(2048, 8.0, 0), (513, 8.0, 50), (2048, 4.0, 50), (3, 8.0, 0)]
    flags = {"default": {}, "4-lanes": dict(fpfh_radius_lanes=4), "16-lanes": dict(fpfh_radius_lanes=16)}
    cloud = staticmethod(_sheet)

    def need(self, s):
        full = (s[0], s[1], 0)                                    # every row within the radius, the row itself included
        return self.sized(s[0], int(_cached(self.name, full, lambda: self.reference(full))["n"].sum()) + s[0])

    def reference(self, s):
        import fpfh_radius_ref
        return fpfh_radius_ref.fpfh(_sheet(s[0]), _sheet_normals(s[0]), fpfh_radius_ref.r2_of(s[1]), s[2])

    def call(self, s, ws, ws_bytes, new):
        import fpfh_radius_ref
        M, radius, mx = s
        pm, r2 = self.model(M), fpfh_radius_ref.r2_of(radius)
        counts, seg = new(M, torch.int32), new(M + 1, torch.int64)
        pm.fpfh_radius_count(r2, out=(counts, seg, ws[:self.sized(M, 0)]))
        total = int(seg[-1].item())
        need = int(self.sized(M, total))
        assert need <= ws.numel(), (need, ws.numel())
        ws[:need].fill_(0xFF)                          # the second call may use nothing the count left in the workspace
        desc, cnt, nn = new((M, 33), torch.float64), new((M, 33), torch.int32), new(M, torch.int32)
        pm.fpfh_radius(r2, soa32(_sheet_normals(M)), seg, total, max_neighbors=mx, spfh=True, out=(desc, cnt, nn, ws[:need]))
        torch.cuda.synchronize()
        return [host(desc), host(cnt).astype(np.int64), host(nn), total, host(counts), host(seg)]

    def expect(self, s, got):
        from test_gpu_fpfh_radius import _check_against
        _check_against(tuple(got[:4]), _cached(self.name, s, lambda: self.reference(s)), str(s))
        np.testing.assert_array_equal(np.diff(got[5]), got[4])


@register
class ModelIss(_SelfJoin):
    """(M, salient radius, non-maximum radius): the radii of tests/iss_ref.py's cases"""
    name, size_fn, cloud_key = "model_iss", "pcreg_dev_model_iss_workspace", "sheet"
    flags = {"default": {}, "knn_nocull": dict(knn_nocull=1)}
    cloud = staticmethod(_sheet)

    @property
    def shapes(self):
        import iss_ref
        (a, b), (c, d) = iss_ref.RADII[0], iss_ref.RADII[-1]
        return [(2048, a, b), (513, c, d), (2048, c, d), (3, a, b)]

    def call(self, s, ws, ws_bytes, new):
        M = s[0]
        out = (new(M, torch.int32), new((M, 3), torch.float64), new(M, torch.float64), new(M, torch.int32), new(1, torch.int32))
        self.model(M).iss_keypoints(s[1], s[2], out=out + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return dict(n=host(out[0]), eig=host(out[1]), s=host(out[2]), keypoints=host(out[3])[:int(out[4].item())])

    def expect(self, s, got):
        import iss_ref
        from test_gpu_iss import _check_against
        model = _sheet(s[0])
        _check_against(got, _cached(self.name, s, lambda: iss_ref.iss(model, iss_ref.r2_of(s[1]), iss_ref.r2_of(s[2]))), model, s[2], str(s))


class _Msac(_SelfJoin):
    """(M, n_trials, min_inliers): the scene of the fitter's reference at its two sizes, 513 rows of it and 3"""
    P = 5
    names = ()                    # the out= order of the fitter, with the dtype and the trailing shape of every output

    def need(self, s):
        return self.sized(s[0], s[1])

    def outs(self, M, new):
        return [new((M if lead == "M" else (1 if lead == 1 else self.P),) + tail, dt) for _, lead, tail, dt in self.names]

    def result(self, out, count_key):
        got = {k: host(t) for (k, _, _, _), t in zip(self.names, out)}
        got[count_key] = int(got[count_key][0])
        return got


_F64, _I32, _I64 = torch.float64, torch.int32, torch.int64


@register
class FitPlanes(_Msac):
    name, size_fn = "model_fit_planes", "pcreg_dev_model_fit_planes_workspace"
    shapes = [(4096, 256, 200), (1030, 128, 40), (513, 300, 20), (3, 128, 3)]
    names = (("labels", "M", (), _I32), ("planes", "P", (4,), _F64), ("centres", "P", (3,), _F64), ("counts", "P", (), _I32), ("rmse", "P", (), _F64),
             ("n_planes", 1, (), _I32), ("best_trial", "P", (), _I32), ("best_cost", "P", (), _I64), ("best_count", "P", (), _I32))

    def cloud(self, M):
        import planes_ref
        return planes_ref.scene(M) if M >= 1030 else planes_ref.scene(1030)[:M]

    def call(self, s, ws, ws_bytes, new):
        M, B, mi = s
        out = self.outs(M, new)
        self.model(M).fit_planes(0.08, max_planes=self.P, n_trials=B, min_inliers=mi, seed=7, out=tuple(out) + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return self.result(out, "n_planes")

    def expect(self, s, got):
        from test_gpu_planes import _check
        _check(self.cloud(s[0]), got, 0.08, self.P, s[1], s[2], 7, what=str(s))
        assert got["n_planes"] == 3 or s[0] < 1030


@register
class FitSpheres(_Msac):
    name, size_fn = "model_fit_spheres", "pcreg_dev_model_fit_spheres_workspace"
    shapes = [(4096, 256, 200), (1030, 256, 40), (513, 300, 20), (3, 128, 4)]
    names = (("labels", "M", (), _I32), ("spheres", "P", (4,), _F64), ("counts", "P", (), _I32), ("rmse", "P", (), _F64), ("refit_used", "P", (), _I32),
             ("n_spheres", 1, (), _I32), ("best_trial", "P", (), _I32), ("best_cost", "P", (), _I64), ("best_count", "P", (), _I32))

    def cloud(self, M):
        import spheres_ref
        return spheres_ref.scene(M) if M >= 1030 else spheres_ref.scene(1030)[:M]

    def call(self, s, ws, ws_bytes, new):
        import spheres_ref as ref
        M, B, mi = s
        out = self.outs(M, new)
        self.model(M).fit_spheres(ref.SCENE_T, max_spheres=ref.SCENE_P, n_trials=B, min_inliers=mi, seed=ref.SCENE_SEED, out=tuple(out) + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return self.result(out, "n_spheres")

    def expect(self, s, got):
        import spheres_ref as ref
        from test_gpu_fit_spheres import _check
        assert ref.SCENE_P == self.P
        _check(self.cloud(s[0]), got, ref.SCENE_T, ref.SCENE_P, s[1], s[2], ref.SCENE_SEED, what=str(s))
        assert got["n_spheres"] == 3 or s[0] < 1030


@register
class FitCylinders(_Msac):
    name, size_fn = "model_fit_cylinders", "pcreg_dev_model_fit_cylinders_workspace"
    shapes = [(4096, 256, 200), (1030, 256, 60), (513, 300, 20), (3, 128, 4)]
    names = (("labels", "M", (), _I32), ("cylinders", "P", (7,), _F64), ("extents", "P", (2,), _F64), ("counts", "P", (), _I32), ("rmse", "P", (), _F64),
             ("refit_used", "P", (), _I32), ("n_cylinders", 1, (), _I32), ("best_trial", "P", (), _I32), ("best_cost", "P", (), _I64),
             ("best_count", "P", (), _I32))

    def both(self, M):
        import cylinders_ref
        m, n, _ = cylinders_ref.scene(M) if M >= 1030 else cylinders_ref.scene(1030)
        return m[:M], n[:M]

    def cloud(self, M):
        return self.both(M)[0]

    def call(self, s, ws, ws_bytes, new):
        import cylinders_ref as ref
        from test_gpu_fit_cylinders import RMAX, T
        M, B, mi = s
        out = self.outs(M, new)
        self.model(M).fit_cylinders(T, soa32(self.both(M)[1]), max_radius=RMAX, max_cylinders=ref.SCENE_P, n_trials=B, min_inliers=mi,
                                    seed=ref.SCENE_SEED, out=tuple(out) + (ws[:ws_bytes],))
        torch.cuda.synchronize()
        return self.result(out, "n_cylinders")

    def expect(self, s, got):
        import cylinders_ref as ref
        from test_gpu_fit_cylinders import RMAX, T, _check
        assert ref.SCENE_P == self.P
        m, nrm = self.both(s[0])
        _check(m, nrm, got, T, ref.SCENE_P, s[1], s[2], ref.SCENE_SEED, max_radius=RMAX, what=str(s))
        assert got["n_cylinders"] == 2 or s[0] < 1030


# ---- unique rows, the aggregated matches, the voxel grid, fast global registration ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_case(kind, n):
    from test_gpu_unique_rows import _make, _pairs_case
    rng = np.random.default_rng(100 + n)
    return _pairs_case(n, rng) if kind == "pairs" else _make(kind, n, rng)


def _cols(A, ld):
    """n x 3 rows -> the [3, ld] column-major block on the device, the rows past n holding values that would sort first"""
    buf = np.full((3, max(ld, 1)), -1e300)
    buf[:, :len(A)] = np.asarray(A).T
    return torch.from_numpy(buf).to(dev())


@register
class UniqueRows(Case):
    """(kind, n): three merge passes; a tenth of it; one row past a tile of equal rows; no row at all.  n is read on the device
    and lies 7 below the capacity."""
    name, size_fn = "unique_rows3", "pcreg_dev_unique_rows3_workspace"
    shapes = [("pool", 3 * 2048 + 5), ("distinct", 615), ("equal", 2049), ("pool", 0)]

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_unique_rows3_workspace(s[1] + 7)

    def call(self, s, ws, ws_bytes, new):
        from pcreg_amd._lib import check, lib
        A = _rows_case(*s)
        n, n_cap, ld = len(A), len(A) + 7, len(A) + 11
        a, n_dev = _cols(A, ld), torch.tensor([n], dtype=torch.int32, device=dev())
        ia, nu = new(n_cap, torch.int32), new(1, torch.int32)
        check(lib().pcreg_dev_unique_rows3_f64(ptr(a), ptr(n_dev), n_cap, ld, 0, ptr(ia), ptr(nu), ptr(ws), C.c_size_t(ws_bytes), stream()))
        k = int(nu.item())
        return dict(n_unique=k, ia=host(ia)[:k])

    def expect(self, s, got):
        from unique_rows_ref import unique_rows_ref
        want, nw = unique_rows_ref(_rows_case(*s))
        assert got["n_unique"] == nw
        np.testing.assert_array_equal(got["ia"].astype(np.int64), want)


@register
class AggregateMatches(Case):
    """n stacked pairs of which both unique steps remove rows: the existing size; a tenth; none"""
    name, size_fn = "aggregate_matches", "pcreg_dev_aggregate_matches_workspace"
    shapes = [3 * 2048 + 5, 615, 2049, 0]

    def need(self, n):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_aggregate_matches_workspace(n + 7)

    def call(self, n, ws, ws_bytes, new):
        from pcreg_amd._lib import check, lib
        p1, p2 = _rows_case("pairs", n)
        n_cap, ld, ldo = n + 7, n + 11, n + 9
        d1, d2, n_dev = _cols(p1, ld), _cols(p2, ld), torch.tensor([n], dtype=torch.int32, device=dev())
        o1, o2, ia, no = new((3, ldo), torch.float64), new((3, ldo), torch.float64), new(n_cap, torch.int32), new(1, torch.int32)
        check(lib().pcreg_dev_aggregate_matches(ptr(d1), ptr(d2), ptr(n_dev), n_cap, ld, ptr(o1), ptr(o2), ldo, 1, ptr(ia), ptr(no), ptr(ws),
                                                C.c_size_t(ws_bytes), stream()))
        u = int(no.item())
        return dict(n_out=u, out1=np.ascontiguousarray(host(o1)[:, :u].T), out2=np.ascontiguousarray(host(o2)[:, :u].T), ia=host(ia)[:u])

    def expect(self, n, got):
        from unique_rows_ref import aggregate_ref
        w1, w2, wia = aggregate_ref(*_rows_case("pairs", n))
        assert got["n_out"] == len(wia)
        assert got["out1"].tobytes() == w1.tobytes() and got["out2"].tobytes() == w2.tobytes()
        np.testing.assert_array_equal(got["ia"].astype(np.int64) - 1, wia)


@register
class DownsampleGrid(Case):
    """(n, rows per voxel): several chunks of the sort; a tenth; a ragged second chunk of single-row voxels; an empty cloud"""
    name, size_fn = "downsample_grid", "pcreg_dev_downsample_grid_workspace"
    shapes = [(20000, 8), (2000, 4), (2048 + 77, 1), (0, 4)]

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_downsample_grid_workspace(s[0])

    def call(self, s, ws, ws_bytes, new):
        from pcreg_amd.device import downsample_grid
        from test_gpu_downsample import cloud
        p, step = cloud(s[0], s[1], 41) if s[0] else (np.zeros((0, 3), np.float32), 1.0)
        n = s[0]
        out = (new((3, n), torch.float32), new(n, torch.int32), new(n, torch.int32), new(1, torch.int32), new(1, torch.int32))
        downsample_grid(soa32(p), step, out=out + (ws[:max(ws_bytes, 1)],))
        torch.cuda.synchronize()
        u = int(out[3].item())
        return dict(n_out=u, info=int(out[4].item()), out=np.ascontiguousarray(host(out[0])[:, :u].T), count=host(out[1])[:u], label=host(out[2]))

    def expect(self, s, got):
        import downsample_ref
        from test_gpu_downsample import cloud
        if not s[0]:
            assert got["n_out"] == 0 and got["info"] == 0
            return
        p, step = cloud(s[0], s[1], 41)
        ro, rc, rl = downsample_ref.downsample_ref(p, step)
        assert got["n_out"] == len(ro) and got["info"] == 0
        same_bits(got["out"], ro, "out")
        np.testing.assert_array_equal(got["count"], rc)
        np.testing.assert_array_equal(got["label"], rl)


@register
class FgrBatched(Case):
    """the three scenes of tests/fgr_ref.py at the defaults; one registration of a tenth of the rows; a batch with a registration
    without rows"""
    name, size_fn = "fgr_batched", "pcreg_dev_fgr_batched_workspace"
    shapes = ["scenes", "tenth", "with_empty"]
    flags = {"default": {}, "fgr_chain": dict(fgr_chain=1)}

    @functools.lru_cache(maxsize=None)
    def batch(self, kind):
        import fgr_ref
        if kind == "scenes":
            scs = fgr_ref.scenes()
            return [s["p1"] for s in scs], [s["p2"] for s in scs], {"delta2": fgr_ref.DELTA ** 2}
        quick = dict(iterations=12, decrease_every=2, delta2=fgr_ref.DELTA ** 2)
        a, b = fgr_ref.scene(100, 0.3, 1.0, 5), fgr_ref.scene(25, 0.3, 2.0, 6)
        if kind == "tenth":
            return [a["p1"]], [a["p2"]], quick
        return [b["p1"], np.zeros((0, 3)), a["p1"]], [b["p2"], np.zeros((0, 3)), a["p2"]], quick

    def need(self, kind):
        import fgr_ref
        from pcreg_amd._lib import lib
        p1s, _, opts = self.batch(kind)
        return lib().pcreg_dev_fgr_batched_workspace(max(len(p) for p in p1s), len(p1s), fgr_ref.options(**opts)["iterations"])

    def call(self, kind, ws, ws_bytes, new):
        from pcreg_amd._lib import FgrResult
        from pcreg_amd.device import fgr_batched_dev, fgr_results
        from test_gpu_fgr import _as_dict
        p1s, p2s, opts = self.batch(kind)
        sizes = [len(p) for p in p1s]
        offs = np.zeros(len(sizes) + 1, np.int32); offs[1:] = np.cumsum(sizes)
        ld = int(offs[-1]) + 5
        a1, a2 = np.full((3, ld), np.nan), np.full((3, ld), np.nan)
        a1[:, :offs[-1]], a2[:, :offs[-1]] = np.concatenate(p1s).T, np.concatenate(p2s).T
        out = (new((len(sizes), C.sizeof(FgrResult)), torch.uint8), new(ld, torch.int32), new(ld, torch.uint8))
        fgr_batched_dev(torch.from_numpy(a1).to(dev()), torch.from_numpy(a2).to(dev()), torch.from_numpy(offs).to(dev()), max(sizes), opts, kept=True,
                        ws=ws[:ws_bytes], out=out)
        torch.cuda.synchronize()
        rs, hi, hk = fgr_results(host(out[0])), host(out[1]), host(out[2])
        return [_as_dict(r, hi, hk, int(offs[b]), sizes[b]) for b, r in enumerate(rs)]

    def expect(self, kind, got):
        import fgr_ref
        from test_gpu_fgr import _same
        p1s, p2s, opts = self.batch(kind)
        for b, g in enumerate(got):
            want = _cached(self.name, (kind, b), lambda: fgr_ref.run_tree(p1s[b], p2s[b], fgr_ref.options(**opts), b=b))
            _same(g, want, f"{kind} registration {b}")
            assert g["failed"] == (len(p1s[b]) == 0)


def top2(pm, q, idx, dist, ws):
    """pcreg_dev_model_search_f32 enqueued on torch's current stream, nothing read back -> (idx, dist)"""
    from pcreg_amd._lib import check, lib
    Q = q.shape[1]
    check(lib().pcreg_dev_model_search_f32(pm.handle, ptr(q), Q, Q, C.c_int32(0), ptr(idx), ptr(dist), ptr(ws), C.c_size_t(ws.numel()), stream()))
    return idx, dist
