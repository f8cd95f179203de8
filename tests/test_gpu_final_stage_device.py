"""The final stage's batched device pieces bit for bit against the per-cluster device calls they replace: K moved copies in one
launch (pcreg_dev_quick_tf_batched), the close-match / refine kernel over K clusters (pcreg_dev_final_close_refine_batched), the
pick of the best cluster and the final surface without a host read (pcreg_dev_final_pick_apply)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rigid(rng, ang=0.05, sh=0.3):
    import oracle.pcreg_oracle as o
    T = np.eye(4); T[:3, :3] = o.eul2rotm(rng.normal(0, ang, 3)); T[3, :3] = rng.normal(0, sh, 3)
    return T


def test_quick_tf_batched_equals_k_single_calls():
    import torch
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import _p, _stream
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    N, K = 5003, 5
    pts = torch.from_numpy(np.ascontiguousarray((rng.random((N, 3)) * [40, 30, 20]).T)).to(dev)          # [3, N]
    Ts = [_rigid(rng, 0.8, 5.0) for _ in range(K)]
    T_dev = torch.from_numpy(np.ascontiguousarray([T.ravel(order="F") for T in Ts])).to(dev)
    out = torch.empty((K, 3, N), dtype=torch.float64, device=dev)
    lim = torch.empty((K, 6), dtype=torch.float64, device=dev)
    check(lib().pcreg_dev_quick_tf_batched(_p(pts), N, N, _p(T_dev), K, _p(out), N, _p(lim), _stream()))
    for k, T in enumerate(Ts):
        one = torch.empty_like(pts)
        Th = (C.c_double * 16)(*T.ravel(order="F"))
        check(lib().pcreg_dev_quick_tf(_p(pts), N, N, Th, _p(one), N, _stream()))
        assert torch.equal(out[k], one), f"copy {k}"
        mn, mx = one.min(dim=1).values, one.max(dim=1).values
        assert torch.equal(lim[k], torch.stack([mn[0], mx[0], mn[1], mx[1], mn[2], mx[2]])), f"limits {k}"


def _cluster(rng, n, cap, M):
    """feat [cap, 3] / featCur [M, 3] and n 1-based pairs; about 70 % of the pairs close (a slightly moved copy), the rest far."""
    featCur = rng.random((M, 3)) * 30.0
    T = _rigid(rng, 0.01, 0.05)
    b = rng.integers(0, M, n)
    a = rng.permutation(cap)[:n]
    feat = rng.random((cap, 3)) * 30.0
    close = rng.random(n) < 0.7
    moved = (np.hstack([featCur[b], np.ones((n, 1))]) @ T)[:, :3] + rng.normal(0, 0.1, (n, 3))
    feat[a[close]] = moved[close]
    pairs = np.column_stack([a + 1, b + 1]).astype(np.int32)
    return feat, featCur, pairs


@pytest.mark.parametrize("seed", [0, 1])
def test_final_close_refine_batched_equals_gather_and_refine(seed):
    import torch
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import _p, _stream
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    ns = [0, 2, 3, 4, 65, 2000, 0]
    caps = [5, 4, 3, 9, 100, 2100, 0]
    Ms = [7, 5, 6, 8, 50, 900, 3]
    maxDist = 1.5
    cl = [_cluster(rng, n, cap, M) for n, cap, M in zip(ns, caps, Ms)]
    K = len(cl)
    kp_off = np.zeros(K + 1, np.int32); kp_off[1:] = np.cumsum(caps)
    seg_off = np.zeros(K + 1, np.int32); seg_off[1:] = np.cumsum(Ms)
    tot = int(kp_off[-1])
    pairs = np.zeros((tot, 2), np.int32); feat = np.zeros((tot, 3))
    for k, (f, fc, pr) in enumerate(cl):
        feat[kp_off[k]:kp_off[k + 1]] = f
        pairs[kp_off[k]:kp_off[k] + len(pr)] = pr
    featCur = np.vstack([c[1] for c in cl])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pairs, d_feat, d_fc, d_kp, d_seg = t(pairs), t(feat), t(featCur), t(kp_off), t(seg_off)
    d_np = t(np.array(ns, np.int32))
    n_close = torch.full((K,), -1, dtype=torch.int32, device=dev)
    prec = torch.zeros(K, dtype=torch.float64, device=dev)
    T16 = torch.full((K, 16), 7.0, dtype=torch.float64, device=dev)
    empty = torch.full((K,), -1, dtype=torch.int32, device=dev)
    check(lib().pcreg_dev_final_close_refine_batched(_p(d_pairs), _p(d_np), _p(d_feat), _p(d_kp), _p(d_fc), _p(d_seg), K, C.c_double(maxDist),
                                                     _p(n_close), _p(prec), _p(T16), _p(empty), _stream()))
    hits = 0
    for k in range(K):
        cap = max(caps[k], 1)
        p1 = torch.zeros((3, cap), dtype=torch.float64, device=dev); p2 = torch.zeros((3, cap), dtype=torch.float64, device=dev)
        fk = d_feat[kp_off[k]:kp_off[k] + max(caps[k], 1)] if caps[k] else d_feat
        pk = d_pairs[kp_off[k]:] if caps[k] else d_pairs                    # (an empty slice has no data pointer)
        check(lib().pcreg_dev_gather_matched_rows(_p(pk), _p(d_np[k:k + 1]), caps[k], _p(fk),
                                                  _p(d_fc[seg_off[k]:]), _p(p1), _p(p2), _stream()))
        T_ref = torch.zeros(16, dtype=torch.float64, device=dev); info = torch.zeros(2, dtype=torch.int32, device=dev)
        check(lib().pcreg_dev_refine_by_distance(_p(p1), _p(p2), _p(d_np[k:k + 1]), caps[k], cap, C.c_double(maxDist), _p(T_ref), _p(info), _stream()))
        inf = info.cpu().numpy()
        assert n_close[k].item() == inf[0] and empty[k].item() == inf[1], f"cluster {k} (n = {ns[k]})"
        assert np.array_equal(T16[k].cpu().numpy().view(np.uint64), T_ref.cpu().numpy().view(np.uint64)), f"cluster {k} (n = {ns[k]})"
        p = prec[k].item()
        if ns[k] == 0:
            assert math.isnan(p)
        else:
            assert p == inf[0] / ns[k] * 100.0
        hits += inf[1] == 0
    assert hits >= 3                                       # the 4-, 65- and 2000-pair clusters were refined


def _invert_tf_left_to_right(T):
    """invertTF.m with every dot product summed left to right in Python floats."""
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    t = [float(T[3, c]) for c in range(3)]
    U = np.eye(4)
    for r in range(3):
        for c in range(3):
            U[r, c] = R[c][r]
    for j in range(3):
        U[3, j] = ((-t[0]) * R[j][0] + (-t[1]) * R[j][1]) + (-t[2]) * R[j][2]
    return U


@pytest.mark.parametrize("precisions,expect", [([float("nan"), 5.0, 5.0, 3.0], 1), ([float("nan")] * 3, 0), ([2.0, float("nan"), 7.0, 7.0], 2),
                                               ([0.0, 0.0], 0), ([1.0, 4.0, float("nan"), 4.5], 3)])
def test_final_pick_apply_follows_matlab_max(precisions, expect):
    import torch
    from pcreg_amd._lib import check, lib
    from pcreg_amd.device import _p, _stream
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(len(precisions) + expect)
    K, N = len(precisions), 1500
    copies = torch.from_numpy(rng.random((K, 3, N)) * 20).to(dev)
    Ts = [_rigid(rng, 0.02, 0.2) for _ in range(K)]
    T16 = torch.from_numpy(np.ascontiguousarray([T.ravel(order="F") for T in Ts])).to(dev)
    for empty_best in (0, 1):
        empty = torch.zeros(K, dtype=torch.int32, device=dev); empty[expect] = empty_best
        prec = torch.tensor(precisions, dtype=torch.float64, device=dev)
        out = torch.empty((3, N), dtype=torch.float64, device=dev)
        best = torch.full((1,), -1, dtype=torch.int32, device=dev)
        check(lib().pcreg_dev_final_pick_apply(_p(prec), _p(T16), _p(empty), K, _p(copies), N, N, _p(out), N, _p(best), _stream()))
        assert best.item() == expect
        if empty_best:
            assert torch.equal(out, copies[expect])
        else:
            U = _invert_tf_left_to_right(Ts[expect])
            ref = torch.empty_like(out)
            Uh = (C.c_double * 16)(*U.ravel(order="F"))
            check(lib().pcreg_dev_quick_tf(_p(copies[expect].contiguous()), N, N, Uh, _p(ref), N, _stream()))
            assert torch.equal(out, ref)
