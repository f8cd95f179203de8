"""AlignPoints_KNN on the GPU (pcreg_amd/csrc/align.hip) against tests/align_ref.py: every scene under every instantiation of the
kernel that holds it and every flag pair it is defined for, at the bounds align_ref.tolerances derives a priori (signs and counts
exact); the three tiers bit for bit; the device tier's edges; the f32 entry's contract; the refusal of a support larger than the
launch holds.  What a scene determines is asserted in full: nothing here skips a case or drops a comparison.  Which branch of the
selection each scene takes is proved without a GPU by tests/test_align_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_ref as ref

pytestmark = pytest.mark.gpu
SCENES = ref.SCENES
MARK = -7.0
PCREG_E_ARG = 1


def _dev():
    return torch.device("cuda", 0)


def _check_scene(name, C1, C2, c, coeff, aligned):
    return ref.compare(SCENES[name].X, ref.scene_ref(name, C1, C2), ref.scene_tol(name, C1, C2), c, coeff, aligned)


# ---- 1. scenes x instantiations x flags -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C1,C2", ref.FLAGS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("pt,nt", ref.INSTANTIATIONS)
def test_every_scene_under_every_instantiation(pt, nt, C1, C2):
    """one host batched call: every scene the instantiation holds, and the plain filler of its largest size that selects it"""
    import pcreg_amd as pc
    cap = pt * nt
    names = [n for n, s in SCENES.items() if s.holds(pt, nt) and (C1, C2) in s.flags]
    assert f"filler_{cap}" in names and max(SCENES[n].n for n in names) == cap
    lower = max([p * t for p, t in ref.INSTANTIATIONS if p * t < cap], default=0)
    assert cap > lower                                               # max_n = cap selects <pt, nt> and no smaller one
    al, co, c, status = pc.AlignPoints_KNN_batched([SCENES[n].X for n in names], C1, C2)
    assert list(status) == [0] * len(names)
    worst = dict(c=0.0, coeff=0.0, aligned=0.0)
    for b, name in enumerate(names):
        try:
            got = _check_scene(name, C1, C2, c[b], co[b], al[b])
        except AssertionError as e:
            raise AssertionError(f"{name} under <{pt}, {nt}> C1 = {int(C1)} C2 = {int(C2)}: {e}") from e
        for k, v in got.items():
            worst[k] = max(worst[k], v)
    print(f"<{pt}, {nt}> C1 = {int(C1)} C2 = {int(C2)}: {len(names)} scenes, largest error / bound  centroid {worst['c']:.2e}  "
          f"coeff {worst['coeff']:.2e}  aligned {worst['aligned']:.2e}")


def test_boxes_give_exact_signed_permutations():
    import pcreg_amd as pc
    names = [n for n in SCENES if n.startswith("box_")]
    for C1, C2 in ref.FLAGS:
        al, co, c, status = pc.AlignPoints_KNN_batched([SCENES[n].X for n in names], C1, C2)
        for b, name in enumerate(names):
            r = ref.scene_ref(name, C1, C2)
            assert status[b] == 0 and np.array_equal(co[b], r["coeff"]) and np.array_equal(c[b], r["c"]), (name, C1, C2)
            assert np.array_equal(al[b], SCENES[name].X @ r["coeff"])


def test_identical_points_give_what_is_determined():
    import pcreg_amd as pc
    for name in ("identical_100", "identical_300"):
        X = SCENES[name].X
        for C1, C2 in ref.FLAGS:
            al, co, c = pc.AlignPoints_KNN(X, C1, C2)
            assert np.array_equal(c.ravel(), X[0])                    # the centroid is exact
            assert np.isfinite(co).all() and np.isfinite(al).all()
            assert np.abs(co.T @ co - np.eye(3)).max() <= 8 * ref.U
            assert (np.abs(al - X @ co).max(axis=1) <= ref.scene_tol(name, C1, C2)["aligned_self"]).all()
            _check_scene(name, C1, C2, c, co, al)


# ---- the device tier, called as bench.py calls it ------------------------------------------------------------------------------
def _device_call(sups, max_n, C1, C2, pad=0, stream=None, B=None):
    """pcreg_dev_align_points_knn_batched through ctypes on torch tensors.  pts has NaN padding rows, every output holds MARK.
    Returns rc and host copies: aligned [3, ld], coeff [B, 9], c [B, 3], status [B], and the offsets."""
    from pcreg_amd._lib import lib
    sizes = [len(x) for x in sups]
    off = np.zeros(len(sups) + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    total = int(off[-1])
    ld = total + pad
    host = np.full((3, max(ld, 1)), np.nan)
    if total:
        host[:, :total] = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in sups]).T
    nb = len(sups) if B is None else B
    pts = torch.from_numpy(host).to(_dev())
    offsets = torch.from_numpy(off).to(_dev())
    al = torch.full((3, max(ld, 1)), MARK, dtype=torch.float64, device=_dev())
    co = torch.full((max(len(sups), 1), 9), MARK, dtype=torch.float64, device=_dev())
    c = torch.full((max(len(sups), 1), 3), MARK, dtype=torch.float64, device=_dev())
    st = torch.full((max(len(sups), 1),), int(MARK), dtype=torch.int32, device=_dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib().pcreg_dev_align_points_knn_batched(p(pts), C.c_int(total), C.c_int(ld), p(offsets), C.c_int(nb), C.c_int(max_n),
                                                      C.c_int(int(C1)), C.c_int(int(C2)), p(al), p(co), p(c), p(st),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, al.cpu().numpy(), co.cpu().numpy(), c.cpu().numpy(), st.cpu().numpy(), off


def _support_of(out, b):
    """(c, coeff [3, 3] with columns as columns, aligned [n, 3]) of support b of a _device_call"""
    _, al, co, c, _, off = out
    return c[b], co[b].reshape(3, 3, order="F"), al[:, off[b]:off[b + 1]].T


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


TIER_SCENES = ("split_tie_small", "crowded_split_interleaved", "plain_500", "far", "tiny_5", "equal_distances_720", "filler_1024")


@pytest.mark.parametrize("C1,C2", [(False, False), (True, True)], ids=lambda v: str(int(v)))
def test_tiers_agree_bit_for_bit(C1, C2):
    """host single, host batched and device tier on the same supports (every one of a size the <4, 256> instantiation is chosen
    for, alone or in the batch: the summation tree is the instantiation's); the device tier twice and on a second stream"""
    import pcreg_amd as pc
    sups = [SCENES[n].X for n in TIER_SCENES]
    assert all(len(x) <= 1024 for x in sups)
    al, co, c, status = pc.AlignPoints_KNN_batched(sups, C1, C2)
    first = _device_call(sups, 1024, C1, C2)
    again = _device_call(sups, 1024, C1, C2)
    other = _device_call(sups, 1024, C1, C2, stream=torch.cuda.Stream())
    assert first[0] == again[0] == other[0] == 0 and list(status) == list(first[4]) == [0] * len(sups)
    for k in (1, 2, 3, 4):
        assert np.array_equal(_bits(first[k]), _bits(again[k])) and np.array_equal(_bits(first[k]), _bits(other[k]))
    for b, name in enumerate(TIER_SCENES):
        dc, dco, dal = _support_of(first, b)
        assert np.array_equal(_bits(dc), _bits(c[b])) and np.array_equal(_bits(dco), _bits(co[b])) and np.array_equal(_bits(dal), _bits(al[b])), name
        sal, sco, sc = pc.AlignPoints_KNN(sups[b], C1, C2)
        assert np.array_equal(_bits(sc.ravel()), _bits(c[b])) and np.array_equal(_bits(sco), _bits(co[b])) and np.array_equal(_bits(sal), _bits(al[b])), name
        _check_scene(name, C1, C2, dc, dco, dal)


def test_a_larger_instantiation_repeats_its_bits_too():
    sups = [SCENES[n].X for n in ("crowded_split_large", "plain_500", "filler_3072", "crowded_split_last")]
    a = _device_call(sups, 3072, False, False)
    b = _device_call(sups, 3072, False, False, stream=torch.cuda.Stream())
    assert a[0] == b[0] == 0
    for k in (1, 2, 3, 4):
        assert np.array_equal(_bits(a[k]), _bits(b[k]))
    _check_scene("crowded_split_large", False, False, *_support_of(a, 0))


# ---- 3. device tier edges ---------------------------------------------------------------------------------------------------------
def test_device_tier_padding_empty_supports_and_sentinels():
    names = ["plain_500", None, "split_tie_small", "one", "tiny_5", None, "crowded_split_first"]
    one = np.array([[1.0, 2.0, 3.0]])
    sups = [np.zeros((0, 3)) if n is None else one if n == "one" else SCENES[n].X for n in names]
    for C1, C2 in ((False, False), (True, True)):
        out = _device_call(sups, 1024, C1, C2, pad=37)
        rc, al, co, c, st, off = out
        assert rc == 0 and list(st) == [0, 1, 0, 1, 0, 1, 0]
        assert (al[:, off[-1]:] == MARK).all() and al.shape[1] == off[-1] + 37          # the padding of aligned is left alone
        for b, name in enumerate(names):
            if st[b] == 0:
                _check_scene(name, C1, C2, *_support_of(out, b))
        dead = np.flatnonzero(st != 0)                                # a support with a status keeps every mark
        assert (co[dead] == MARK).all() and (c[dead] == MARK).all() and (al[:, off[3]:off[4]] == MARK).all()


def test_device_tier_no_supports_is_a_no_op():
    rc, al, co, c, st, _ = _device_call([SCENES["plain_500"].X], 1024, False, False, B=0)
    assert rc == 0 and (al == MARK).all() and (co == MARK).all() and (c == MARK).all() and (st == int(MARK)).all()


def test_device_tier_refuses_max_n_beyond_the_limit():
    from pcreg_amd._lib import lib
    rc, al, co, c, st, _ = _device_call([SCENES["plain_500"].X], 8193, False, False)
    assert rc == PCREG_E_ARG and b"8192" in lib().pcreg_last_error()
    assert (al == MARK).all() and (co == MARK).all() and (c == MARK).all() and (st == int(MARK)).all()


# ---- 4. the f32 entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["split_tie_small", "crowded_split_interleaved", "plain_500", "tiny_5", "box_zxy"])
def test_f32_entry_is_the_fp64_entry_rounded_once(name):
    """api.hip: the float input is widened exactly, the double kernel runs, the outputs are rounded once to float"""
    import pcreg_amd as pc
    X32 = SCENES[name].X.astype(np.float32)
    wide = X32.astype(np.float64)
    if name != "plain_500":
        assert np.array_equal(wide, SCENES[name].X)                  # the lattices are the same scene in float
    for C1, C2 in SCENES[name].flags:
        al32, co32, c32 = pc.AlignPoints_KNN(X32, C1, C2)
        al, co, c = pc.AlignPoints_KNN(wide, C1, C2)
        assert al32.dtype == co32.dtype == c32.dtype == np.float32
        for a32, a64 in ((al32, al), (co32, co), (c32, c)):
            assert np.array_equal(a32.view(np.uint32), a64.astype(np.float32).view(np.uint32)), (name, C1, C2)
        r = ref.align(wide, C1, C2)
        ref.compare(wide, r, ref.tolerances(wide, C1, C2, r), c, co, al)


# ---- 5. a support larger than the launch holds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_n,n_big", [(1000, 1500), (2000, 2100), (3000, 3100), (4000, 4100), (8192, 8193)])
def test_device_tier_refuses_a_support_the_launch_does_not_hold(max_n, n_big):
    """max_n is trusted and chooses the launch; a support beyond PT * NT has status 2 and nothing else written"""
    big = np.tile(SCENES["filler_8192"].X, (2, 1))[:n_big]
    names = ["plain_500", None, "split_tie_small"]
    sups = [SCENES["plain_500"].X, big, SCENES["split_tie_small"].X]
    out = _device_call(sups, max_n, False, False, pad=5)
    rc, al, co, c, st, off = out
    assert rc == 0 and list(st) == [0, 2, 0]
    assert (co[1] == MARK).all() and (c[1] == MARK).all() and (al[:, off[1]:off[2]] == MARK).all() and (al[:, off[3]:] == MARK).all()
    for b in (0, 2):
        _check_scene(names[b], False, False, *_support_of(out, b))


def test_host_tier_reports_zero_or_one_only():
    import pcreg_amd as pc
    sups = [SCENES["plain_500"].X, np.array([[1.0, 2.0, 3.0]]), SCENES["filler_2048"].X[:1500], np.zeros((0, 3)), SCENES["filler_8192"].X]
    al, co, c, status = pc.AlignPoints_KNN_batched(sups)
    assert list(status) == [0, 1, 0, 1, 0]
    _check_scene("plain_500", False, False, c[0], co[0], al[0])
    _check_scene("filler_8192", False, False, c[4], co[4], al[4])
