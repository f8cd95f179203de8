"""Voxel-grid average downsampling on the device (pcreg_downsample_grid_f32 and pcreg_dev_downsample_grid_f32)
against tests/downsample_ref.py.  Every comparison is exact: the bits of out, count, label and n_out.  T is the number of
records one workgroup of the sort handles (kDsT in pcreg_amd/csrc/downsample.hip, read through pcreg_dev_downsample_grid_chunk)."""
import ctypes as C

import numpy as np
import pytest

import downsample_ref as ref

pytestmark = pytest.mark.gpu

T = 2048                                              # kDsT of downsample.hip; test_T_is_the_librarys holds the two together
NAN, INF = float("nan"), float("inf")
SENT_F, SENT_I = np.float32(-12345.0), np.int32(-777)


def _L():
    from pcreg_amd import _lib
    return _lib, _lib.lib()


def host_call(pts, step, ld=None, ldo=None, want_count=True, want_label=True):
    """pcreg_downsample_grid_f32 on buffers full of sentinels -> (rc, n_out, out [ldo, 3] F-order, count [n], label [n])"""
    _l, L = _L()
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    n = p.shape[0]
    ld = max(n, 1) if ld is None else ld
    ldo = max(n, 1) if ldo is None else ldo
    pin = np.full((ld, 3), SENT_F, np.float32, order="F"); pin[:n] = p
    out = np.full((ldo, 3), SENT_F, np.float32, order="F")
    count = np.full(max(n, 1), SENT_I, np.int32); label = np.full(max(n, 1), SENT_I, np.int32)
    no = C.c_int(-9)
    rc = L.pcreg_downsample_grid_f32(pin.ctypes.data, n, ld, float(step), out.ctypes.data, ldo, count.ctypes.data if want_count else None,
                                     label.ctypes.data if want_label else None, C.byref(no))
    return rc, no.value, out, count, label


def check_case(pts, step, res=None, want_count=True, want_label=True):
    """the result equals the reference bit for bit, the padding and the rows past n_out keep their sentinels, the invariants hold"""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    n = p.shape[0]
    rc, n_out, out, count, label = host_call(p, step, want_count=want_count, want_label=want_label) if res is None else res
    assert rc == 0, _L()[1].pcreg_last_error()
    ro, rc_, rl = ref.downsample_ref(p, step)
    u = ro.shape[0]
    assert n_out == u
    np.testing.assert_array_equal(np.ascontiguousarray(out[:u]).view(np.uint32), ro.view(np.uint32))
    assert (out[u:] == SENT_F).all()
    if want_count:
        np.testing.assert_array_equal(count[:u], rc_)
        assert (count[u:] == SENT_I).all()
    else:
        assert (count == SENT_I).all()
    live = ref.live_rows(p)
    if want_label and u > 0:
        np.testing.assert_array_equal(label[:n], rl)
        assert ((label[:n] == 0) == ~live).all()
        # out[label - 1]'s voxel is the row's voxel
        lo, cells = ref.cells_of(p, step, live)
        mean = out[label[:n][live] - 1]
        mc = np.floor((mean.astype(np.float64) - lo.astype(np.float64)) / np.float64(step)).astype(np.int64)
        np.testing.assert_array_equal(mc, cells)
    elif u == 0 or not want_label:
        assert (label == SENT_I).all()                # no live row: nothing is written
    if want_count:
        assert int(count[:u].astype(np.int64).sum()) == int(live.sum())
    return n_out, out[:u], count[:u], label[:n]


def cloud(n, per_voxel, seed, box=100.0):
    """n uniformly random points in a cube and the step that gives about per_voxel of them per voxel"""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * box - box / 3).astype(np.float32)       # negative coordinates among them
    step = box / max((n / per_voxel) ** (1.0 / 3.0), 1.0)
    return p, step


def spread(n, seed):
    """n values in (0, 1) whose double sum depends on the order: 24-bit mantissas over 40 binades"""
    rng = np.random.default_rng(seed)
    return (rng.random(n) * np.exp2(-rng.integers(0, 40, n).astype(np.float64))).astype(np.float32)


def test_T_is_the_librarys():
    assert _L()[1].pcreg_dev_downsample_grid_chunk() == T


def test_n_0_and_n_1():
    rc, n_out, out, count, label = host_call(np.zeros((0, 3)), 1.0)
    assert rc == 0 and n_out == 0 and (out == SENT_F).all() and (count == SENT_I).all() and (label == SENT_I).all()
    n_out, out, count, label = check_case([[3.0, -4.0, 5.0]], 0.25)
    assert n_out == 1 and out.tolist() == [[3.0, -4.0, 5.0]] and count.tolist() == [1] and label.tolist() == [1]


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_sizes_around_the_workgroup(n):
    p, step = cloud(n, 4, n)
    n_out, *_ = check_case(p, step)
    assert n / 8 < n_out < n


def test_one_voxel_across_workgroups():
    """3T + 7 rows in one voxel: one run across workgroups; the sum's order shows in the bits"""
    n = 3 * T + 7
    p = np.stack([spread(n, 1), spread(n, 2), spread(n, 3)], axis=1)
    x = p[:, 0].astype(np.float64)
    fwd = rev = 0.0
    for v in x: fwd += v
    for v in x[::-1]: rev += v
    assert fwd != rev                                                   # the order matters for these values
    n_out, out, count, _ = check_case(p, 2.0)
    assert n_out == 1 and count[0] == n
    # the same run behind live sort passes: a few rows elsewhere give the keys bits, the long run of equal digits is ranked stably
    far = (np.random.default_rng(4).random((50, 3)) * 95 + 5).astype(np.float32)
    q = np.concatenate([p[:T + 3], far[:20], p[T + 3:], far[20:]])
    n_out, out, count, _ = check_case(q, 2.0)
    assert count[0] == n and n_out > 40


def test_every_row_its_own_voxel_in_descending_key_order():
    n = 3 * T + 7
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = (np.arange(n)[::-1] // 64) * 2.0 + 0.5
    p[:, 1] = (np.arange(n)[::-1] % 64) * 2.0 + 0.25
    p[:, 2] = 1.0
    n_out, out, count, label = check_case(p, 2.0)
    assert n_out == n and (count == 1).all() and (label == np.arange(n, 0, -1)).all()


def test_a_permuted_cloud():
    p, step = cloud(3 * T + 7, 6, 11)
    a = check_case(p, step)
    perm = np.random.default_rng(12).permutation(len(p))
    b = check_case(p[perm], step)                                      # against the reference on the permuted input
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[2], b[2])                           # the voxels and their counts do not depend on the row order
    np.testing.assert_array_equal(a[3][perm], b[3])                     # ... nor does a row's voxel
    np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=1e-5)                   # the means may differ in their last bit: another order of adds


def test_dead_rows():
    p, step = cloud(2 * T + 100, 4, 21)
    rng = np.random.default_rng(22)
    bad = rng.choice(np.arange(1, len(p) - 1), 60, replace=False)
    for j, r in enumerate(bad):
        p[r, j % 3] = (NAN, INF, -INF)[(j // 3) % 3]
    p[0, 1] = NAN; p[-1, 2] = -INF
    n_out, out, count, label = check_case(p, step)
    assert (label == 0).sum() == 62
    dead = np.full((T + 5, 3), NAN, np.float32); dead[::3, 0] = INF; dead[::3, 1:] = 1.0
    rc, n_out, out, count, label = host_call(dead, 1.0)
    assert rc == 0 and n_out == 0 and (out == SENT_F).all() and (count == SENT_I).all() and (label == SENT_I).all()


def test_negative_flat_duplicates():
    p, step = cloud(T + 77, 4, 31)
    check_case(-np.abs(p) - 1000.0, step)
    flat = p.copy(); flat[:, 1] = -3.5
    check_case(flat, step)
    dup = np.tile(np.array([[1.5, -2.5, 3.25]], np.float32), (T + 9, 1))
    n_out, out, count, _ = check_case(dup, 0.125)
    assert n_out == 1 and count[0] == T + 9 and out.tolist() == [[1.5, -2.5, 3.25]]


def test_leading_dimensions_keep_their_padding():
    p, step = cloud(T + 300, 4, 41)
    n = len(p)
    res = host_call(p, step, ld=n + 13, ldo=n + 29)
    check_case(p, step, res=res)                                       # (checks the sentinels of every row past n_out, the padding included)


def test_more_than_32_key_bits():
    rng = np.random.default_rng(51)
    n = 4000
    p = np.stack([rng.random(n) * 2 ** 20, rng.random(n) * 2 ** 20, rng.random(n) * 8], axis=1).astype(np.float32)
    p[0] = 0.0; p[1] = (2 ** 20 - 0.5, 2 ** 20 - 0.5, 7.5)
    p[10:14] = p[20:24]                                               # some voxels with two rows
    n_out, *_ = check_case(p, 1.0)
    assert n - 10 < n_out < n
    # all 63 key bits, and the bit above them for a dead row: every digit pass is live
    q = (rng.random((n, 3)) * (2 ** 21 - 1)).astype(np.float32)
    q[0] = 0.0; q[1] = 2 ** 21 - 0.5
    q[30:40] = q[50:60]; q[5, 1] = NAN
    n_out, *_ = check_case(q, 1.0)
    assert n - 20 < n_out < n


def dev_call(pts, step, stream=None, ws_fill=0, want_count=True, want_label=True):
    """pcreg_dev_downsample_grid_f32 on sentinel-filled device buffers -> host copies (rc, n_out, info, out [n, 3], count, label)"""
    import torch
    _l, L = _L()
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    n = p.shape[0]
    dev = torch.device("cuda")
    d_p = torch.from_numpy(np.ascontiguousarray(p.T)).to(dev)
    d_out = torch.full((3, max(n, 1)), float(SENT_F), dtype=torch.float32, device=dev)
    d_cnt = torch.full((max(n, 1),), int(SENT_I), dtype=torch.int32, device=dev)
    d_lab = torch.full((max(n, 1),), int(SENT_I), dtype=torch.int32, device=dev)
    d_w = torch.full((2,), -9, dtype=torch.int32, device=dev)
    ws = torch.full((max(int(L.pcreg_dev_downsample_grid_workspace(n)), 256),), ws_fill, dtype=torch.uint8, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = L.pcreg_dev_downsample_grid_f32(vp(d_p), n, max(n, 1), float(step), vp(d_out), max(n, 1), vp(d_cnt) if want_count else None,
                                         vp(d_lab) if want_label else None, vp(d_w), C.c_void_p(d_w.data_ptr() + 4), vp(ws), C.c_size_t(ws.numel()),
                                         C.c_void_p(s.cuda_stream))
    s.synchronize()
    w = d_w.cpu().numpy()
    return rc, int(w[0]), int(w[1]), np.asfortranarray(d_out.cpu().numpy().T), d_cnt.cpu().numpy(), d_lab.cpu().numpy()


def test_one_axis_past_the_cell_limit_is_refused():
    _l, L = _L()
    rng = np.random.default_rng(61)
    p = (rng.random((4000, 3)) * 2 ** 20).astype(np.float32)
    p[0] = 0.0; p[1, 1] = 2 ** 21
    rc, n_out, out, count, label = host_call(p, 1.0)
    assert rc == _l.PCREG_E_ARG and b"2^21" in L.pcreg_last_error()
    assert n_out == -9 or n_out == 0
    assert (out == SENT_F).all() and (count == SENT_I).all() and (label == SENT_I).all()
    rc, n_out, info, out, count, label = dev_call(p, 1.0)
    assert rc == 0 and info == 1 and n_out == 0
    assert (out == SENT_F).all() and (count == SENT_I).all() and (label == SENT_I).all()
    # a step so small that the quotient overflows
    rc, *_ = host_call(np.array([[0, 0, 0], [3e38, 0, 0]], np.float32), 1e-300)
    assert rc == _l.PCREG_E_ARG


@pytest.fixture(scope="module")
def big():
    """200 000 uniformly random points and the reference at about 8 and about 1 per voxel, computed once"""
    p, s8 = cloud(200_000, 8, 71)
    _, s1 = cloud(200_000, 1, 71)
    return p, {8: s8, 1: s1}


@pytest.mark.parametrize("per_voxel", [8, 1])
def test_200k_points(big, per_voxel):
    p, steps = big
    n_out, _, count, _ = check_case(p, steps[per_voxel])
    assert 0.5 * per_voxel < len(p) / n_out < 2.5 * max(per_voxel, 1.3)


def test_streams_and_workspace_contents_change_no_bit():
    import torch
    p, step = cloud(3 * T + 7, 4, 81)
    p[5, 0] = NAN
    a = dev_call(p, step, stream=torch.cuda.Stream(), ws_fill=0)
    b = dev_call(p, step, stream=torch.cuda.Stream(), ws_fill=0xFF)
    assert a[0] == b[0] == 0 and a[1] == b[1] and a[2] == b[2] == 0
    for x, y in zip(a[3:], b[3:]):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    check_case(p, step, res=(a[0], a[1], a[3], a[4], a[5]))


@pytest.mark.parametrize("want_count, want_label", [(False, True), (True, False), (False, False)])
def test_count_and_label_may_be_null(want_count, want_label):
    p, step = cloud(T + 40, 4, 91)
    p[3, 2] = INF
    check_case(p, step, want_count=want_count, want_label=want_label)
    rc, n_out, info, out, count, label = dev_call(p, step, want_count=want_count, want_label=want_label)
    check_case(p, step, res=(rc, n_out, out, count, label), want_count=want_count, want_label=want_label)


def test_the_python_tiers():
    import torch
    import pcreg_amd as pc
    from pcreg_amd.device import PreparedModel, downsample_grid, soa
    p, step = cloud(20_000, 8, 101)
    p[7, 1] = NAN
    ro, rc_, rl = ref.downsample_ref(p, step)
    out, count, label = pc.pcdownsample(p, step)
    np.testing.assert_array_equal(out.view(np.uint32), ro.view(np.uint32))
    np.testing.assert_array_equal(count, rc_)
    np.testing.assert_array_equal(label, rl - 1)
    # the resident form: the same bits, and a prepared model straight from its output
    d_out, d_count, d_label, d_n, d_info = downsample_grid(soa(torch.from_numpy(p).cuda()), step)
    u = int(d_n.item())
    assert u == len(ro) and int(d_info.item()) == 0
    np.testing.assert_array_equal(d_out[:, :u].cpu().numpy().T.copy().view(np.uint32), ro.view(np.uint32))
    np.testing.assert_array_equal(d_count[:u].cpu().numpy(), rc_)
    np.testing.assert_array_equal(d_label.cpu().numpy(), rl)
    q = soa(torch.from_numpy(p[:500][np.isfinite(p[:500]).all(axis=1)]).cuda())
    i1, d1 = PreparedModel(d_out[:, :u]).knn(q, 1)
    i2, d2 = PreparedModel(soa(torch.from_numpy(out).cuda())).knn(q, 1)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    with pytest.raises(pc._lib.PcregError):
        pc.pcdownsample(np.array([[0, 0, 0], [2.0 ** 21, 0, 0]]), 1.0)
