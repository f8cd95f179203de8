"""The radius search writes nowhere but where it may: both calls on exactly the reported workspace size in front of a guard
pattern (one byte less is refused), idx / dist of exactly `total` elements in front of a guard, and the fill's clamps -- a seg_off
made with a smaller radius, and a capacity below the total, truncate segments and never write past them.  The guards are sized
so that an unclamped fill would still land in memory the test owns: a defect shows in the pattern."""
import os

import numpy as np
import pytest
import torch

import range_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
PATTERN = 0xA5
SENT = 0x5A5A5A5A                                       # the guard word behind idx / dist (as int32, and as the bits of a float)
CORES = min(len(os.sched_getaffinity(0)), 16)


def _dev():
    return torch.device("cuda", 0)


def _soa(x):
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T)))
    return t


def _same(a, b):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _check_bounds(need, call, refuse=True):
    """call(ws) -> outputs (nested lists of arrays); ws = (workspace tensor, the workspace_bytes to pass)"""
    from pcreg_amd._lib import PCREG_E_WORKSPACE, PcregError
    need = int(need)
    assert need > 0
    tight = torch.empty(need + GUARD, dtype=torch.uint8, device=_dev())
    tight[need:] = PATTERN
    out = call((tight, need))
    torch.cuda.synchronize()
    assert bool((tight[need:] == PATTERN).all()), "a write past the reported workspace size"
    roomy = torch.empty(2 * need + GUARD, dtype=torch.uint8, device=_dev())
    _same(out, call((roomy, roomy.numel())))
    if refuse:
        with pytest.raises(PcregError) as e:
            call((tight, need - 1))
        assert e.value.code == PCREG_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((tight[need:] == PATTERN).all())


class _Case:
    def __init__(self):
        from bench import synth
        from pcreg_amd.device import PreparedModel
        model, surf, _ = synth(1_000_000, 50_000)
        self.model, self.surf = model, surf[np.sort(np.random.default_rng(17).choice(len(surf), 4000, replace=False))]
        self.t = _soa(model)
        self.pm = PreparedModel(self.t)
        self.q = _soa(self.surf)
        self.Q = len(self.surf)


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.pm.close()


def _count(c, r2, ws):
    from pcreg_amd._lib import check, lib
    counts = torch.empty(c.Q, dtype=torch.int32, device=_dev())
    so = torch.empty(c.Q + 1, dtype=torch.int64, device=_dev())
    check(lib().pcreg_dev_model_range_count_f32(c.pm.handle.value, c.q.data_ptr(), c.Q, c.Q, float(r2), counts.data_ptr(), so.data_ptr(),
                                                ws[0].data_ptr(), ws[1], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return counts, so


def _fill(c, r2, so, capacity, room, ws):
    """idx / dist of `room` elements, all set to the guard word; the call is told `capacity`"""
    from pcreg_amd._lib import check, lib
    idx = torch.full((room,), SENT, dtype=torch.int32, device=_dev())
    dist = torch.full((room,), SENT, dtype=torch.int32, device=_dev()).view(torch.float32)
    check(lib().pcreg_dev_model_range_fill_f32(c.pm.handle.value, c.q.data_ptr(), c.Q, c.Q, float(r2), 0, so.data_ptr(), int(capacity),
                                               idx.data_ptr(), dist.data_ptr(), ws[0].data_ptr(), ws[1], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.view(torch.int32).cpu().numpy()


def test_both_calls_stay_inside_the_reported_workspace_and_the_result(case):
    from pcreg_amd._lib import lib
    c = case
    need = lib().pcreg_dev_model_range_workspace(c.Q, c.pm.M)
    assert need == lib().pcreg_dev_model_range_workspace(c.Q, 0)
    r2 = 1.0
    rso, ri, rd = ref.rangesearch(c.surf, c.model, r2, threads=CORES)
    total = int(rso[-1])
    tail = GUARD // 4

    def count(ws):
        counts, so = _count(c, r2, ws)
        return [counts.cpu().numpy(), so.cpu().numpy()]
    _check_bounds(need, count)
    so = _count(c, r2, (torch.empty(need, dtype=torch.uint8, device=_dev()), need))[1]
    np.testing.assert_array_equal(so.cpu().numpy(), rso)

    def fill(ws):
        idx, dist = _fill(c, r2, so, total, total + tail, ws)            # exactly `total` elements in front of a guard
        assert np.all(idx[total:] == SENT) and np.all(dist[total:] == SENT), "a write past idx / dist [total]"
        return [idx[:total], dist[:total]]
    _check_bounds(need, fill)
    idx, dist = fill((torch.empty(need, dtype=torch.uint8, device=_dev()), need))
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist.view(np.uint32), rd.view(np.uint32))


def test_the_fill_is_clamped_to_the_segments_and_the_capacity(case):
    from pcreg_amd._lib import lib
    c = case
    need = lib().pcreg_dev_model_range_workspace(c.Q, c.pm.M)
    ws = (torch.empty(need, dtype=torch.uint8, device=_dev()), need)
    rso1, ri1, rd1 = ref.rangesearch(c.surf, c.model, 1.0, threads=CORES)
    rso2, ri2, rd2 = ref.rangesearch(c.surf, c.model, 4.0, threads=CORES)
    t1, t2 = int(rso1[-1]), int(rso2[-1])
    assert t2 > 5 * t1 > 0
    room = t1 + t2 + 4096                                   # an unclamped fill (t2 rows from any segment start) stays inside
    so1 = torch.from_numpy(rso1).to(_dev())
    # (a) segments sized by r = 1, filled with r = 2: truncated, every row kept belongs to the r = 2 result, nothing past t1
    idx, dist = _fill(c, 4.0, so1, t1, room, ws)
    assert np.all(idx[t1:] == SENT) and np.all(dist[t1:] == SENT), "a write past the segments"
    qid = np.repeat(np.arange(c.Q), np.diff(rso1))
    assert np.all(idx[:t1] != SENT), "a query with more rows than its segment fills the segment"
    key2 = np.repeat(np.arange(c.Q), np.diff(rso2)).astype(np.int64) * (1 << 32) + ri2
    order = np.argsort(key2)
    pos = np.searchsorted(key2[order], qid.astype(np.int64) * (1 << 32) + idx[:t1])
    assert np.all(key2[order][np.minimum(pos, t2 - 1)] == qid.astype(np.int64) * (1 << 32) + idx[:t1]), "a row outside the r = 2 result"
    np.testing.assert_array_equal(dist[:t1].view(np.uint32), rd2.view(np.uint32)[order][pos])
    for a, b in zip(rso1[:-1], rso1[1:]):                  # each truncated segment is still in (distance, row) order
        k = (dist[a:b].astype(np.int64) << 32) | idx[a:b]
        assert np.all(np.diff(k) > 0)
    # (b) the right seg_off, half the capacity: nothing at or past the capacity, every segment that ends inside it is right
    cap = t1 // 2
    idx, dist = _fill(c, 1.0, so1, cap, room, ws)
    assert np.all(idx[cap:] == SENT) and np.all(dist[cap:] == SENT), "a write past the capacity"
    whole = int(rso1[np.searchsorted(rso1, cap, side="right") - 1])        # the end of the last segment that is complete
    assert 0 < whole <= cap
    np.testing.assert_array_equal(idx[:whole], ri1[:whole])
    np.testing.assert_array_equal(dist[:whole].view(np.uint32), rd1.view(np.uint32)[:whole])
    # (c) a seg_off that is no running sum at all (descending, negative, beyond the capacity): still nothing outside [0, capacity)
    rng = np.random.default_rng(5)
    wild = torch.from_numpy(rng.integers(-1000, 2 * t1, c.Q + 1).astype(np.int64)).to(_dev())
    idx, dist = _fill(c, 4.0, wild, t1, room, ws)
    assert np.all(idx[t1:] == SENT) and np.all(dist[t1:] == SENT), "a write past the capacity"
