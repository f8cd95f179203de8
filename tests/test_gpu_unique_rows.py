"""unique(A, 'rows') on the device (pcreg_amd/csrc/unique_rows.hip), aggregate_matches and the indexed estimateTransform against
tests/unique_rows_ref.py and the oracle.  ia and the counts must equal the reference EXACTLY, at the device tier (n read from
device memory, a leading dimension, garbage past n, guarded buffers) and at the host tier, at every size at which the chain
takes another shape: below / at / past a wave, a tile (T = 2048), one, two and three merge passes."""
import ctypes as C

import numpy as np
import pytest

from unique_rows_ref import aggregate_ref, unique_rows_ref

pytestmark = pytest.mark.gpu

T = 2048
SIZES = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 8 * T + 17]
SPECIAL = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308, 1.0, np.inf])


def _make(kind, n, rng):
    if kind == "pool":                                   # heavy duplication, zeros of both signs
        A = rng.integers(-2, 3, (n, 3)).astype(np.float64) * 0.5
        A[(A == 0) & (rng.random((n, 3)) < 0.5)] = -0.0
    elif kind == "equal":
        A = np.tile(np.array([1.5, -2.0, 0.0]), (n, 1))
    elif kind == "distinct":
        A = rng.uniform(-50, 50, (n, 3))
    elif kind == "col3":                                 # rows that differ only in column 3
        A = np.tile(np.array([3.25, -7.5, 0.0]), (n, 1))
        A[:, 2] = rng.integers(0, n // 3 + 1, n) * 0.125 - 1.0
    elif kind == "special":                              # negative values, subnormals, +-inf, -0 / +0 mixed
        A = SPECIAL[rng.integers(0, len(SPECIAL), (n, 3))]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(A, dtype=np.float64)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev_unique(A, n_cap=None, ld=None, idx_base=0, garbage=None):
    """pcreg_dev_unique_rows3_f64 on A's n rows inside a [3, ld] buffer with capacity n_cap; rows past n hold `garbage`.  The
    workspace and ia carry guards that must come back untouched.  -> (ia [n_unique], n_unique)"""
    import torch
    from pcreg_amd._lib import check, lib
    L = lib()
    dev = torch.device("cuda", 0)
    n = A.shape[0]
    n_cap = n if n_cap is None else n_cap
    ld = max(n_cap, 1) if ld is None else ld
    buf = np.full((3, ld), -1e300 if garbage is None else garbage, dtype=np.float64)
    buf[:, :n] = A.T
    a = torch.from_numpy(buf).to(dev)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    ia = torch.full((n_cap + 64,), -7, dtype=torch.int32, device=dev)
    nu = torch.full((1,), -1, dtype=torch.int32, device=dev)
    wsb = L.pcreg_dev_unique_rows3_workspace(n_cap)
    ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device=dev)
    check(L.pcreg_dev_unique_rows3_f64(_p(a), _p(n_dev), n_cap, ld, idx_base, _p(ia), _p(nu), _p(ws), C.c_size_t(wsb),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    ia_h, nu_h, guard = ia.cpu().numpy(), int(nu.cpu()[0]), ws[wsb:].cpu().numpy()
    assert 0 <= nu_h <= n
    assert (ia_h[nu_h:] == -7).all(), "ia written past n_unique"
    assert (guard == 0xA5).all(), "workspace written past its size"
    return ia_h[:nu_h].astype(np.int64) - idx_base, nu_h


def _host_unique(A, ld=None):
    """pcreg_unique_rows3 (1-based) -> 0-based ia"""
    from pcreg_amd._lib import check, lib
    n = A.shape[0]
    ld = max(n, 1) if ld is None else ld
    buf = np.full((ld, 3), np.nan, order="F")            # (past n: never read -- a NaN there would be refused)
    buf[:n] = A
    ia = np.full(max(n, 1) + 8, -7, dtype=np.int32)
    nu = C.c_int(-1)
    check(lib().pcreg_unique_rows3(C.c_void_p(buf.ctypes.data), n, ld, C.c_void_p(ia.ctypes.data), C.byref(nu)))
    assert (ia[max(n, 1):] == -7).all()
    return ia[:nu.value].astype(np.int64) - 1, nu.value


@pytest.mark.parametrize("kind", ["pool", "equal", "distinct", "col3", "special"])
def test_unique_rows_equals_the_reference_at_both_tiers(kind):
    import pcreg_amd as pc
    rng = np.random.default_rng(11)
    for n in SIZES:
        A = _make(kind, n, rng)
        want, nw = unique_rows_ref(A)
        got, ng = _dev_unique(A)
        assert ng == nw, (kind, n)
        np.testing.assert_array_equal(got, want, err_msg=f"device tier, {kind}, n = {n}")
        goth, nh = _host_unique(A)
        assert nh == nw, (kind, n)
        np.testing.assert_array_equal(goth, want, err_msg=f"host tier, {kind}, n = {n}")
    # the Python entry: C carries the representative's bits (the sign of a zero included)
    A = _make(kind, 3 * T + 5, rng)
    want, _ = unique_rows_ref(A)
    Cm, ia = pc.unique_rows(A)
    np.testing.assert_array_equal(ia, want)
    assert Cm.tobytes() == A[want].tobytes()


@pytest.mark.parametrize("n, n_cap, ld", [(0, 5, 9), (1, 1, 4), (65, 100, 131), (T, T + 1, T + 1), (T + 1, 2 * T, 2 * T + 3), (2 * T + 1, 8 * T + 17, 8 * T + 20),
                                           (3 * T + 5, 4 * T + 1, 5 * T)])
def test_n_is_read_on_the_device_and_rows_past_it_are_not(n, n_cap, ld):
    """*n_dev < n_cap <= ld: the grid and the number of merge passes follow n_cap, the result follows n; the rows past n hold values
    that would sort FIRST (and then NaN / +inf) and must not reach the result; a 1-based ia."""
    rng = np.random.default_rng(n + 1)
    A = _make("pool", n, rng)
    want, nw = unique_rows_ref(A)
    for garbage in (-1e300, np.nan, np.inf):
        got, ng = _dev_unique(A, n_cap=n_cap, ld=ld, idx_base=1, garbage=garbage)
        assert ng == nw
        np.testing.assert_array_equal(got, want)
    if n:
        goth, nh = _host_unique(A, ld=n + 3)
        assert nh == nw
        np.testing.assert_array_equal(goth, want)


def test_nan_rows_terminate_and_stay_in_bounds_on_the_device():
    """The device tier orders a NaN by its mapped bit pattern (documented, not MATLAB's rule): the call ends, writes inside its
    buffers, and the rows WITHOUT a NaN keep the reference's order among themselves."""
    rng = np.random.default_rng(5)
    n = 2 * T + 9
    A = _make("pool", n, rng)
    bad = rng.random(n) < 0.2
    A[bad, rng.integers(0, 3, bad.sum())] = np.nan
    A[bad & (rng.random(n) < 0.5)] *= -1.0               # NaNs of both signs
    got, ng = _dev_unique(A)
    assert len(set(got.tolist())) == ng and ((got >= 0) & (got < n)).all()
    # a run of equal clean rows stays contiguous whatever the NaN rows do, and its first row still leads it
    clean = got[~bad[got]]
    want, _ = unique_rows_ref(A[~bad])
    np.testing.assert_array_equal(clean, np.nonzero(~bad)[0][want])


def _pairs_case(n, rng, k1=300, k2=120):
    """n stacked pairs: surface points from a pool of k1 (so the first unique removes rows), each bound to a model point from a pool
    of k2 at its FIRST use only -- later uses of a surface point may name another model point, as two spheres may -- and k2 < k1,
    so the second unique removes rows too"""
    s_pool = rng.uniform(-30, 30, (k1, 3))
    m_pool = rng.uniform(0, 60, (k2, 3))
    return s_pool[rng.integers(0, k1, n)], m_pool[rng.integers(0, k2, n)]


@pytest.mark.parametrize("n", [0, 1, 65, T + 1, 3 * T + 5])
def test_aggregate_matches_equals_the_reference(n):
    import torch
    import pcreg_amd as pc
    from pcreg_amd._lib import check, lib
    rng = np.random.default_rng(100 + n)
    p1, p2 = _pairs_case(n, rng)
    w1, w2, wia = aggregate_ref(p1, p2)
    n1 = unique_rows_ref(p1)[1]
    if n > 1000:
        assert n > n1 > len(wia) >= 3                     # both uniques remove rows
    # host tier, through the Python entry
    g1, g2, gia = pc.aggregate_matches(p1, p2)
    np.testing.assert_array_equal(gia, wia)
    assert g1.tobytes() == w1.tobytes() and g2.tobytes() == w2.tobytes()
    # device tier: a capacity and leading dimensions past n, garbage behind n, 1-based composed ia, and ia = NULL
    L = lib()
    dev = torch.device("cuda", 0)
    n_cap, ld, ldo = n + 7, n + 11, n + 9
    b1 = np.full((3, ld), -1e300); b1[:, :n] = p1.T
    b2 = np.full((3, ld), -1e300); b2[:, :n] = p2.T
    d1, d2 = torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    wsb = L.pcreg_dev_aggregate_matches_workspace(n_cap)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_ia in (True, False):
        o1 = torch.full((3, ldo), -3.0, dtype=torch.float64, device=dev); o2 = torch.full((3, ldo), -3.0, dtype=torch.float64, device=dev)
        ia = torch.full((n_cap,), -7, dtype=torch.int32, device=dev)
        no = torch.full((1,), -1, dtype=torch.int32, device=dev)
        ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device=dev)
        check(L.pcreg_dev_aggregate_matches(_p(d1), _p(d2), _p(n_dev), n_cap, ld, _p(o1), _p(o2), ldo, 1, _p(ia) if with_ia else None, _p(no),
                                            _p(ws), C.c_size_t(wsb), sp))
        u = int(no.cpu()[0])
        assert u == len(wia)
        assert (ws[wsb:].cpu().numpy() == 0xA5).all()
        h1, h2, hia = o1.cpu().numpy(), o2.cpu().numpy(), ia.cpu().numpy()
        assert np.ascontiguousarray(h1[:, :u].T).tobytes() == w1.tobytes() and np.ascontiguousarray(h2[:, :u].T).tobytes() == w2.tobytes()
        assert (h1[:, u:] == -3.0).all() and (h2[:, u:] == -3.0).all()
        if with_ia:
            np.testing.assert_array_equal(hia[:u].astype(np.int64) - 1, wia)
            assert (hia[u:] == -7).all()
        else:
            assert (hia == -7).all()
        off = 2 * ((4 * max(n_cap, 1) + 255) // 256 * 256)                     # include/pcreg.h: the first unique's count
        assert int(ws[off:off + 4].view(torch.int32).cpu()[0]) == n1


def test_estimate_transform_indexed_against_the_oracle(oracle_py):
    """The 1200-pair scene of test_quicktf_inverttf_and_distance_refine (restated), index lists of length 0, 2, 3 and 840: empty
    exactly when the oracle's estimateTransform is, else within the bound that test uses."""
    import torch
    from pcreg_amd._lib import check, lib
    rng = np.random.default_rng(1)
    pts = rng.uniform(-20, 20, (5000, 3))
    T2 = np.eye(4); T2[:3, :3] = oracle_py.eul2rotm(np.array([0.01, -0.02, 0.015])).T; T2[3, :3] = [0.05, -0.02, 0.03]
    p2 = pts[:1200]
    p1 = oracle_py.quickTF(p2, T2) + rng.normal(0, 0.01, p2.shape)
    p1[:360] += rng.uniform(3, 6, (360, 3))
    _, inl = oracle_py.refine_by_distance(p1, p2, 1.5)
    inl0 = np.asarray(inl, dtype=np.int64)                                        # 0-based rows
    assert len(inl0) == 840
    L = lib()
    dev = torch.device("cuda", 0)
    cap, ld = 1200, 1207
    b1 = np.zeros((3, ld)); b1[:, :cap] = p1.T
    b2 = np.zeros((3, ld)); b2[:, :cap] = p2.T
    d1, d2 = torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in (0, 2, 3, 840):
        rows = rng.permutation(inl0)[:k] if k < 840 else inl0
        want = oracle_py.estimateTransform(p1[rows], p2[rows]) if k else None
        lst = np.full(cap, 2**30, dtype=np.int32)                                  # entries past the count: never used
        lst[:k] = rows + 1
        idx = torch.from_numpy(lst).to(dev)
        n_idx = torch.tensor([k], dtype=torch.int32, device=dev)
        T16 = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
        info = torch.full((2,), -1, dtype=torch.int32, device=dev)
        check(L.pcreg_dev_estimate_transform_indexed(_p(d1), _p(d2), ld, _p(idx), 1, _p(n_idx), cap, _p(T16), _p(info), sp))
        cnt, empty = (int(v) for v in info.cpu())
        assert cnt == k
        assert bool(empty) == (want is None), k
        Tg = T16.cpu().numpy().reshape(4, 4, order="F")
        if want is None:
            assert (Tg == 0).all()
        else:
            assert np.linalg.norm(Tg - want) < 1e-9, (k, np.linalg.norm(Tg - want))
    assert k == 840 and np.linalg.norm(Tg - T2) < 0.01
