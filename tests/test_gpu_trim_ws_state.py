"""The trimmed entries under the three checks of tests/ws_state.py -- fills, sequence, outputs -- that
tests/test_gpu_ws_state.py gives every entry with a size function of its own.  The trimmed entries have none: they run in their
untrimmed twins' workspaces and keep their select state in blocks of it that are dead between the walk and the sums, which is
exactly what a stale or dirtied workspace would show up.  The cases are the registry's score and refit cases at keep_ratio 0.6."""
import numpy as np
import pytest
import torch

import ws_state
from ws_state import R15, ModelScore, Outputs, _cached, _Refit, _scene_model, host, m44, same_bits, soa32, t16, workspace

pytestmark = pytest.mark.gpu
_DT = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}


KEEP = 0.6


def _trim_want(name, s, surf, model, T, method, **kw):
    """trim_ref's step on these inputs; the candidate pairs (the expensive part) are shared by the four cases"""
    import trim_ref
    T = np.asarray(T, np.float64)
    cand = _cached("trim.pairs", (name.split(".")[0], len(surf), T.tobytes()), lambda: trim_ref.pairs(surf, model, T, R15, threads=8))
    return _cached(name, (s, T.tobytes()), lambda: trim_ref.step_of_pairs(cand, model, T, KEEP, method, **kw))


class _TrimmedRefit(_Refit):
    """_Refit with n_within and d2_cut behind the untrimmed outputs; `empty` is third from the end"""
    method = None

    def run_steps(self, T, surf, steps, ws, ws_bytes, new, **more):
        B = len(T)
        out = [new((B, 16), torch.float64), new((B, 16), torch.float64)] + [new(B, _DT[k]) for k in self.kinds]
        tmp = new((B, 16), torch.float64) if steps > 1 else None
        self.invoke(_scene_model(), soa32(surf), t16(T), steps, tuple(out) + (ws[:ws_bytes], tmp), **more)
        torch.cuda.synchronize()
        return [m44(host(out[0])), m44(host(out[1]))] + [host(t) for t in out[2:]]

    def expect(self, s, got):
        T, surf = self.inputs(s)
        if s[1] == 1:
            self.compare(s, got, T, surf)
            return
        cur, one = T, None
        for step in range(s[1]):
            outs = Outputs()
            one = self.run_steps(cur, surf, 1, workspace(self.need((s[0], 1)), 0x00), int(self.need((s[0], 1))), outs.new)
            outs.check_guards(f"{self.name} single step {step}")
            self.compare((s[0], 1, step), one, cur, surf)
            cur = one[0]
        same_bits(got, one, f"{self.name}: three steps against three single steps")
        assert got[-3].tolist() == [0, 0, 0, 0, 1, 1]

    def normals(self, Q):
        import gicp_ref
        import plane_ref
        return plane_ref.scene()["normals"], gicp_ref.surface_normals()[:Q]

    def compare(self, s, got, T, surf):
        import plane_ref
        import test_gpu_trim as t
        model = plane_ref.scene()["model"]
        nrm, nq = self.normals(len(surf))
        kw = {"rigid": {}, "plane": dict(normals=nrm), "gicp": dict(normals=nrm, qnormals=nq)}[self.method]
        want = _trim_want("sheet." + self.method, s, surf, model, T, self.method, **kw)
        got = tuple(got)
        if self.method == "rigid":
            t.check_refit(got, T, want, model, str(s))
        else:
            t.check_trim_outputs(got[7], got[8], want)
            (t._check_plane if self.method == "plane" else t._check_gicp)(got[:7], T, want, str(s))


class RefitRigidTrimmed(_TrimmedRefit):
    name, size_fn, method = "model_refit_trimmed", "pcreg_dev_model_refit_workspace", "rigid"
    kinds = (np.int32, np.float64, np.int32, np.int32, np.float32)

    def invoke(self, pm, q, Td, steps, out):
        pm.refit_transforms(q, Td, R15, steps=steps, out=out, keep_ratio=KEEP)


class RefitPlaneTrimmed(_TrimmedRefit):
    name, size_fn, method = "model_refit_plane_trimmed", "pcreg_dev_model_refit_plane_workspace", "plane"
    kinds = (np.int32, np.float64, np.int32, np.float64, np.int32, np.int32, np.float32)

    def invoke(self, pm, q, Td, steps, out):
        pm.refit_plane(q, Td, R15, soa32(self.normals(0)[0]), steps=steps, out=out, keep_ratio=KEEP)


class RefitGicpTrimmed(_TrimmedRefit):
    name, size_fn, method = "model_refit_gicp_trimmed", "pcreg_dev_model_refit_gicp_workspace", "gicp"
    kinds = (np.int32, np.float64, np.int32, np.float64, np.int32, np.int32, np.float32)

    def invoke(self, pm, q, Td, steps, out):
        nrm, nq = self.normals(q.shape[1])
        pm.refit_gicp_trimmed(q, Td, R15, KEEP, soa32(nrm), soa32(nq), steps=steps, out=out)


class ModelScoreTrimmed(ModelScore):
    name, size_fn = "model_score_trimmed", "pcreg_dev_model_score_workspace"

    def need(self, s):
        from pcreg_amd._lib import lib
        return lib().pcreg_dev_model_score_workspace(s[1], s[0][1] - s[0][0], self.model().M)

    def call(self, s, ws, ws_bytes, new):
        _, surf, T, _ = self.scene()
        (b0, b1), Q = s
        B = b1 - b0
        out = (new(B, torch.int32), new(B, torch.float64), new((B, Q), torch.int32), new((B, Q), torch.float32), new(B, torch.int32),
               new(B, torch.float32))
        self.model().score_transforms(soa32(surf[:Q]), t16(T[b0:b1]), R15, rows=True, out=out + (ws[:ws_bytes],), keep_ratio=KEEP)
        torch.cuda.synchronize()
        return [host(t) for t in out]

    def expect(self, s, got):
        import score_ref
        import test_gpu_trim as t
        import trim_ref
        _, surf, T, nn = self.scene()
        (b0, b1), Q = s
        B = b1 - b0
        pick = lambda a: np.ascontiguousarray(np.asarray(a).reshape(8, 3000)[b0:b1, :Q]).reshape(-1)
        idx, dist = score_ref.within(pick(nn[0]), pick(nn[1]), R15)
        idx, dist, n_within, d2_cut = trim_ref.trim(idx.reshape(B, Q), dist.reshape(B, Q), KEEP)
        n_close, sum_d2 = score_ref.sums(idx, dist)
        t.check_score(tuple(got), dict(idx=idx, dist=dist, n_close=n_close, sum_d2=sum_d2, n_within=n_within, d2_cut=d2_cut), Q)


CASES = {c.name: c for c in (ModelScoreTrimmed(), RefitRigidTrimmed(), RefitPlaneTrimmed(), RefitGicpTrimmed())}


@pytest.mark.parametrize("name,k", [(n, k) for n, c in CASES.items() for k in range(len(c.shapes))])
def test_fills(name, k):
    ws_state.fills(CASES[name], CASES[name].shapes[k])


@pytest.mark.parametrize("name,flag", [(n, f) for n, c in CASES.items() for f in c.flags])
def test_sequence(name, flag, debug_set):
    case = CASES[name]
    for key, value in case.flags[flag].items():
        debug_set(key, value)
    ws_state.sequence(case, case.shapes_for(flag))


@pytest.mark.parametrize("name", list(CASES))
def test_outputs(name):
    ws_state.outputs(CASES[name])
