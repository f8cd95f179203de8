"""The clustering call writes nowhere but where it may: the device entry on exactly pcreg_dev_model_cluster_workspace(M) bytes in
front of a guard pattern (one byte less is refused), label / first / sizes of exactly M elements and n_clusters of one element in
front of guard words.  The guards are memory the test owns: a defect shows in the pattern."""
import numpy as np
import pytest
import torch

import cluster_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
PATTERN = 0xA5
SENT = 0x5A5A5A5A
TAIL = 4096


def _dev():
    return torch.device("cuda", 0)


def _soa(x):
    t = torch.empty((3, len(x)), dtype=torch.float32, device=_dev())
    if len(x):
        t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T)))
    return t


def _call(pm, r2, ws, ws_bytes, with_lists=True):
    """-> label [M], n_clusters, first [M], sizes [M] as numpy; asserts the guard words behind every output"""
    from pcreg_amd._lib import check, lib
    M = pm.M
    outs = [torch.full((n + TAIL,), SENT, dtype=torch.int32, device=_dev()) for n in (M, 1, M, M)]
    check(lib().pcreg_dev_model_cluster_f32(pm.handle.value, float(r2), outs[0].data_ptr(), outs[1].data_ptr(),
                                            outs[2].data_ptr() if with_lists else None, outs[3].data_ptr() if with_lists else None,
                                            ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = [o.cpu().numpy() for o in outs]
    for o, n in zip(h, (M, 1, M, M)):
        assert np.all(o[n:] == SENT), "a write past an output"
    if not with_lists:
        assert np.all(h[2] == SENT) and np.all(h[3] == SENT)
    return h[0][:M], int(h[1][0]), h[2][:M], h[3][:M]


@pytest.mark.parametrize("M, r", [(1_000_000, 0.75), (513, 0.8), (512, 0.8), (1, 1.0), (100_003, 1.2)])
def test_the_call_stays_inside_the_reported_workspace_and_its_outputs(M, r):
    from pcreg_amd._lib import PCREG_E_WORKSPACE, PcregError, lib
    from pcreg_amd.device import PreparedModel
    if M == 1_000_000:
        from bench import synth
        model = synth(1_000_000, 50_000)[0]
    else:
        model = (np.random.default_rng(M).random((M, 3)) * (M ** (1 / 3))).astype(np.float32)
    r2 = np.float32(r) ** 2
    t = _soa(model)
    pm = PreparedModel(t)
    try:
        need = int(lib().pcreg_dev_model_cluster_workspace(M))
        assert need > 0
        tight = torch.empty(need + GUARD, dtype=torch.uint8, device=_dev())
        tight[need:] = PATTERN
        got = _call(pm, r2, tight, need)
        assert bool((tight[need:] == PATTERN).all()), "a write past the reported workspace size"
        label, off, members = ref.cluster(model, r2)
        rf, rs = ref.first_and_sizes(label, off, members)
        nc = len(off) - 1
        assert got[1] == nc
        np.testing.assert_array_equal(got[0], label)
        np.testing.assert_array_equal(got[2][:nc], rf)
        np.testing.assert_array_equal(got[3][:nc], rs)
        assert not got[2][nc:].any() and not got[3][nc:].any()
        roomy = torch.empty(2 * need + GUARD, dtype=torch.uint8, device=_dev())
        again = _call(pm, r2, roomy, roomy.numel())
        for a, b in zip(got, again):
            np.testing.assert_array_equal(a, b)
        lab_only = _call(pm, r2, tight, need, with_lists=False)           # first / sizes NULL
        np.testing.assert_array_equal(lab_only[0], label)
        assert lab_only[1] == nc and bool((tight[need:] == PATTERN).all())
        with pytest.raises(PcregError) as e:
            _call(pm, r2, tight, need - 1)
        assert e.value.code == PCREG_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((tight[need:] == PATTERN).all())
    finally:
        pm.close()
