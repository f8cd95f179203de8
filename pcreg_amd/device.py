"""Device tier: the resident correspondence-search + RANSAC pipeline on torch tensors.

torch is plumbing only (device memory, streams, torch.distributed over RCCL); every
operation of HipOps is one pcreg_dev_* entry point of include/pcreg.h launching
hand-written HIP kernels on torch's current stream.  Layout: point sets are [3, N]
contiguous tensors, i.e. MATLAB's column-major N x 3 with ld = N.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from ._lib import DevRansacResult, RansacOpts, check, lib
from . import _lib as _l
from .sharded import ShardedMatcher, gather_ransac_parts, hypothesis_share


def _p(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def soa(points: torch.Tensor) -> torch.Tensor:
    """N x 3 row-major -> [3, N] contiguous (column-major N x 3, ld = N)."""
    return points.t().contiguous()


def _keep_ratio(keep_ratio) -> float:
    """The trimmed entries' ratio: a number in (0, 1]."""
    keep_ratio = float(keep_ratio)
    if not 0.0 < keep_ratio <= 1.0:
        raise ValueError(f"keep_ratio must lie in (0, 1], got {keep_ratio}")
    return keep_ratio


_TRIM_KINDS = (torch.int32, torch.float32)         # n_within, d2_cut: what a trimmed refit returns beyond its untrimmed twin


class _RefitSteps:
    """What the five "B transforms refitted `steps` times" methods share (PreparedModel.refit_transforms, refit_plane, refit_gicp,
    refit_cpd and NdtModel.refit).  Creating one checks q_soa, T_dev and steps; the method then checks its own arguments, and
    run() finds the buffers and runs the steps."""

    def __init__(self, q_soa: torch.Tensor, T_dev: torch.Tensor, steps: int, empty_any_stride: bool = False):
        Q = int(q_soa.shape[1]) if q_soa.dim() == 2 else 0
        if q_soa.dtype != torch.float32 or q_soa.dim() != 2 or q_soa.shape[0] != 3 or ((Q or not empty_any_stride) and q_soa.stride(1) != 1):
            raise TypeError("queries are a [3, Q] float32 tensor with contiguous rows (column-major Q x 3)")
        if T_dev.dtype != torch.float64 or not T_dev.is_contiguous() or T_dev.numel() % 16 or T_dev.device != q_soa.device:
            raise TypeError("transforms are a contiguous float64 tensor of B x 16 numbers on the queries' device")
        self.steps = int(steps)
        if self.steps < 1:
            raise ValueError(f"steps must be at least 1, got {self.steps}")
        self.T_dev, self.dev, self.Q, self.B = T_dev, q_soa.device, Q, T_dev.numel() // 16
        self.q_args = (_p(q_soa) if Q else None, Q, max(int(q_soa.stride(0)), Q, 1))      # (an empty tensor has no address to pass)

    def run(self, owner, ws_attr: str, need: int, kinds, out, call):
        """-> (T_out, T_step, one [B] tensor per dtype of `kinds`): allocated here with the workspace of `need` bytes cached on
        owner.ws_attr and grown on demand, or unpacked from out=(T_out, T_step, ..., ws, T_tmp).  Then call(src, dst, T_step, ...,
        ws) once per step, a step's dst the next one's src: the last step writes T_out, the blocks alternate backwards from it."""
        dev, B, steps = self.dev, self.B, self.steps
        need = max(int(need), 256)
        if out is not None:
            *res, ws, T_tmp = out
            if len(res) != 2 + len(kinds):
                raise ValueError(f"out holds {2 + len(kinds)} outputs, ws and T_tmp; got {len(out)} entries")
            if steps > 1 and T_tmp is None:
                raise ValueError("more than one step needs the second transform block, T_tmp")
        else:
            res = [torch.empty((B, 16), dtype=torch.float64, device=dev) for _ in range(2)] + [torch.empty(B, dtype=k, device=dev) for k in kinds]
            T_tmp = torch.empty((B, 16), dtype=torch.float64, device=dev) if steps > 1 else None
            ws = getattr(owner, ws_attr, None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                setattr(owner, ws_attr, ws)
        if B:                                          # (an empty tensor has no address to pass)
            with torch.cuda.device(dev):
                src = self.T_dev
                for s in range(steps):
                    dst = res[0] if (steps - 1 - s) % 2 == 0 else T_tmp
                    call(src, dst, *res[1:], ws)
                    src = dst
        return tuple(res)


class PreparedModel:
    """A model shard prepared ONCE for any number of searches (pcreg_dev_model_create: bounding box, matrix-core operand
    tiles, model-wide seeding grid) -- one model, many surfaces is the reference's shape (completeExperimentFast.m:131-149).
    Keeps the [3, M] float32 tensor alive; the handle is only valid while that tensor is unchanged."""

    def __init__(self, model_soa: torch.Tensor):
        if model_soa.dtype != torch.float32 or model_soa.dim() != 2 or model_soa.shape[0] != 3 or model_soa.stride(1) != 1:
            raise TypeError("a model is a [3, M] float32 tensor with contiguous rows (column-major M x 3)")
        self.tensor, self.version = model_soa, model_soa._version
        self.key = _model_key(model_soa)
        self.M, self.ld = int(model_soa.shape[1]), int(model_soa.stride(0)) if model_soa.shape[1] > 0 else 1
        self.handle = C.c_void_p()
        with torch.cuda.device(model_soa.device):
            check(lib().pcreg_dev_model_create(_p(model_soa), self.M, max(self.ld, 1), _stream(), C.byref(self.handle)))

    def knn(self, q_soa: torch.Tensor, k: int, idx_base: int = 0, out=None):
        """knnsearch(model, q, 'K', k) on torch's current stream (pcreg_dev_model_knn_f32): q_soa a [3, Q] float32 tensor with
        contiguous rows -> (idx [Q, k] int32, idx_base + 0-based row, -1 past M; dist [Q, k] float32 squared, +inf past M),
        ordered by (distance, row).  The workspace is cached on the model and grown on demand; calls that may overlap on two
        streams pass buffers of their own, out=(idx, dist, ws) with ws of pcreg_dev_model_knn_workspace(Q, M, k) bytes."""
        if q_soa.dtype != torch.float32 or q_soa.dim() != 2 or q_soa.shape[0] != 3 or q_soa.stride(1) != 1:
            raise TypeError("queries are a [3, Q] float32 tensor with contiguous rows (column-major Q x 3)")
        if not 1 <= int(k) <= _l.KNN_MAX_K:
            raise ValueError(f"k must lie in [1, {_l.KNN_MAX_K}], got {k}")
        k, Q = int(k), int(q_soa.shape[1])
        L = lib()
        if Q == 0:
            return (torch.empty((0, k), dtype=torch.int32, device=q_soa.device), torch.empty((0, k), dtype=torch.float32, device=q_soa.device))
        need = max(int(L.pcreg_dev_model_knn_workspace(Q, self.M, k)), 256)
        if out is not None:
            idx, dist, ws = out
        else:
            idx = torch.empty((Q, k), dtype=torch.int32, device=q_soa.device)
            dist = torch.empty((Q, k), dtype=torch.float32, device=q_soa.device)
            ws = getattr(self, "_knn_ws", None)
            if ws is None or ws.numel() < need or ws.device != q_soa.device:
                ws = self._knn_ws = torch.empty(need, dtype=torch.uint8, device=q_soa.device)
        with torch.cuda.device(q_soa.device):
            check(L.pcreg_dev_model_knn_f32(self.handle, _p(q_soa), Q, int(q_soa.stride(0)), k, C.c_int32(idx_base), _p(idx), _p(dist), _p(ws),
                                            C.c_size_t(ws.numel()), _stream()))
        return idx, dist

    def _range_args(self, q_soa, r2):
        if q_soa.dtype != torch.float32 or q_soa.dim() != 2 or q_soa.shape[0] != 3 or q_soa.stride(1) != 1:
            raise TypeError("queries are a [3, Q] float32 tensor with contiguous rows (column-major Q x 3)")
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        Q = int(q_soa.shape[1])
        return r2, Q, max(int(lib().pcreg_dev_model_range_workspace(Q, self.M)), 256)

    def _range_ws(self, need, device):
        ws = getattr(self, "_range_ws_t", None)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = self._range_ws_t = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def rangesearch_count(self, q_soa: torch.Tensor, r2: float, out=None):
        """The first half of rangesearch(model, q, r) with r2 = r^2, on torch's current stream (pcreg_dev_model_range_count_f32):
        -> (counts [Q] int32, seg_off [Q + 1] int64, the exclusive running sums; seg_off[Q] is the number of rows).  Nothing
        synchronises.  The workspace is cached on the model and grown on demand; calls that may overlap on two streams pass
        buffers of their own, out=(counts, seg_off, ws) with ws of pcreg_dev_model_range_workspace(Q, M) bytes."""
        r2, Q, need = self._range_args(q_soa, r2)
        if out is not None:
            counts, seg_off, ws = out
        else:
            counts = torch.empty(Q, dtype=torch.int32, device=q_soa.device)
            seg_off = torch.empty(Q + 1, dtype=torch.int64, device=q_soa.device)
            ws = self._range_ws(need, q_soa.device)
        if Q == 0:                                     # (an empty tensor has no address to pass)
            seg_off.zero_()
            return counts, seg_off
        with torch.cuda.device(q_soa.device):
            check(lib().pcreg_dev_model_range_count_f32(self.handle, _p(q_soa), Q, max(int(q_soa.stride(0)), Q), r2, _p(counts), _p(seg_off), _p(ws),
                                                        ws.numel(), _stream()))
        return counts, seg_off

    def rangesearch_fill(self, q_soa: torch.Tensor, r2: float, seg_off: torch.Tensor, idx: torch.Tensor, dist: torch.Tensor, idx_base: int = 0,
                         ws=None):
        """The second half (pcreg_dev_model_range_fill_f32): query i's rows into idx / dist [seg_off[i], seg_off[i + 1]), in
        (distance, row) order, never outside those bounds or past len(idx).  No synchronisation."""
        r2, Q, need = self._range_args(q_soa, r2)
        if ws is None:
            ws = self._range_ws(need, q_soa.device)
        if Q == 0 or min(idx.numel(), dist.numel()) == 0:
            return idx, dist
        with torch.cuda.device(q_soa.device):
            check(lib().pcreg_dev_model_range_fill_f32(self.handle, _p(q_soa), Q, max(int(q_soa.stride(0)), Q), r2, int(idx_base), _p(seg_off),
                                                       min(idx.numel(), dist.numel()), _p(idx), _p(dist), _p(ws), ws.numel(), _stream()))
        return idx, dist

    def rangesearch(self, q_soa: torch.Tensor, r2: float, idx_base: int = 0):
        """rangesearch(model, q, r) with r2 = r^2 -> (seg_off [Q + 1] int64, idx [total] int32 = idx_base + 0-based row, dist
        [total] float32 squared); query i's rows are seg_off[i] .. seg_off[i + 1], ordered by (distance, row).  Reads the total
        (seg_off[Q]) on the host ONCE, between the count and the fill, to size idx / dist: the only synchronisation."""
        _, seg_off = self.rangesearch_count(q_soa, r2)
        total = int(seg_off[-1].item())
        idx = torch.empty(total, dtype=torch.int32, device=q_soa.device)
        dist = torch.empty(total, dtype=torch.float32, device=q_soa.device)
        if total:
            self.rangesearch_fill(q_soa, r2, seg_off, idx, dist, idx_base)
        return seg_off, idx, dist

    def score_transforms(self, q_soa: torch.Tensor, T_dev: torch.Tensor, r2: float, rows: bool = False, out=None, keep_ratio=None):
        """How well B transforms put a cloud on the model, on torch's current stream (pcreg_dev_model_score_f32): q_soa a [3, Q]
        float32 tensor with contiguous rows, T_dev a contiguous float64 tensor of B x 16 numbers (each transform column-major
        4 x 4, used as quickTF uses it; all zeros: the empty transform, which scores nothing), r2 the squared radius ->
        (n_close [B] int32, the queries with a model row within r2 of their transformed place; sum_d2 [B] float64, the sum of
        those squared distances), and with rows=True also (idx [B, Q] int32, the nearest such row, -1 for none; dist [B, Q]
        float32, +inf for none).  Fitness is n_close / Q and the inlier RMSE sqrt(sum_d2 / n_close).  Nothing synchronises.
        The workspace is cached on the model and grown on demand; calls that may overlap on two streams pass buffers of
        their own, out=(n_close, sum_d2, idx, dist, ws) with ws of pcreg_dev_model_score_workspace(Q, B, M) bytes (idx and
        dist None without rows).
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_dev_model_score_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query -- and two more tensors
        end the tuple: n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B] float32, the largest kept squared
        distance (+inf where nothing is kept); `out` then holds them too, before ws, which is the size it is without keep_ratio.  idx / dist hold -1 / +inf at trimmed slots."""
        if q_soa.dtype != torch.float32 or q_soa.dim() != 2 or q_soa.shape[0] != 3 or q_soa.stride(1) != 1:
            raise TypeError("queries are a [3, Q] float32 tensor with contiguous rows (column-major Q x 3)")
        if T_dev.dtype != torch.float64 or not T_dev.is_contiguous() or T_dev.numel() % 16 or T_dev.device != q_soa.device:
            raise TypeError("transforms are a contiguous float64 tensor of B x 16 numbers on the queries' device")
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        dev, Q, B = q_soa.device, int(q_soa.shape[1]), T_dev.numel() // 16
        if keep_ratio is not None:
            keep_ratio = _keep_ratio(keep_ratio)
        need = max(int(lib().pcreg_dev_model_score_workspace(Q, B, self.M)), 256)
        n_within = d2_cut = None
        if out is not None and keep_ratio is not None:
            n_close, sum_d2, idx, dist, n_within, d2_cut, ws = out
        elif out is not None:
            n_close, sum_d2, idx, dist, ws = out
        else:
            if keep_ratio is not None:
                n_within = torch.empty(B, dtype=torch.int32, device=dev)
                d2_cut = torch.empty(B, dtype=torch.float32, device=dev)
            n_close = torch.empty(B, dtype=torch.int32, device=dev)
            sum_d2 = torch.empty(B, dtype=torch.float64, device=dev)
            idx = torch.empty((B, Q), dtype=torch.int32, device=dev) if rows else None
            dist = torch.empty((B, Q), dtype=torch.float32, device=dev) if rows else None
            ws = getattr(self, "_score_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._score_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if B and keep_ratio is not None:
            with torch.cuda.device(dev):
                check(lib().pcreg_dev_model_score_trimmed_f32(self.handle, _p(q_soa) if Q else None, Q, max(int(q_soa.stride(0)), Q, 1), _p(T_dev), B, r2,
                                                              keep_ratio, _p(n_close), _p(sum_d2), _p(idx) if idx is not None and Q else None,
                                                              _p(dist) if dist is not None and Q else None, _p(ws), ws.numel(), _stream(),
                                                              _p(n_within), _p(d2_cut)))
        elif B:                                        # (an empty tensor has no address to pass)
            with torch.cuda.device(dev):
                check(lib().pcreg_dev_model_score_f32(self.handle, _p(q_soa) if Q else None, Q, max(int(q_soa.stride(0)), Q, 1), _p(T_dev), B, r2,
                                                      _p(n_close), _p(sum_d2), _p(idx) if idx is not None and Q else None,
                                                      _p(dist) if dist is not None and Q else None, _p(ws), ws.numel(), _stream()))
        res = (n_close, sum_d2, idx, dist) if rows else (n_close, sum_d2)
        return res + (n_within, d2_cut) if keep_ratio is not None else res

    def refit_transforms(self, q_soa: torch.Tensor, T_dev: torch.Tensor, r2: float, steps: int = 1, out=None, keep_ratio=None):
        """B transforms refitted on their close pairs, `steps` times over, on torch's current stream (pcreg_dev_model_refit_f32
        once per step, a step's T_out the next one's input, no host synchronisation in between): q_soa, T_dev and r2 as
        score_transforms takes them -> (T_out [B, 16] float64, each transform column-major 4 x 4; T_step [B, 16], the last step's
        estimateTransform(model rows, moved points), T_out = T_in * T_step; n_close [B] int32 and sum_d2 [B] float64, the bits
        score_transforms gives for the transform that went INTO the last step; empty [B] int32, 1 where there is no fit -- fewer
        than three pairs, an empty estimateTransform, an all-zero input -- and both matrices are zeros).  T_dev is not written.
        The workspace and the second transform block are cached on the model; calls that may overlap on two streams pass
        buffers of their own, out=(T_out, T_step, n_close, sum_d2, empty, ws, T_tmp) with ws of
        pcreg_dev_model_refit_workspace(Q, B, M) bytes and T_tmp [B, 16] float64 (None with steps = 1).
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_dev_model_refit_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query -- and two more tensors
        end the tuple: n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B] float32, the largest kept squared
        distance (+inf where nothing is kept); `out` then holds them too, before ws, which is the size it is without keep_ratio.  Every step trims anew."""
        st = _RefitSteps(q_soa, T_dev, steps)
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        if keep_ratio is not None:
            keep_ratio = _keep_ratio(keep_ratio)

            def call_trimmed(src, dst, T_step, n_close, sum_d2, empty, n_within, d2_cut, ws):
                check(lib().pcreg_dev_model_refit_trimmed_f32(self.handle, *st.q_args, _p(src), st.B, r2, keep_ratio, _p(dst), _p(T_step), _p(n_close),
                                                              _p(sum_d2), _p(empty), _p(ws), ws.numel(), _stream(), _p(n_within), _p(d2_cut)))
            return st.run(self, "_refit_ws_t", lib().pcreg_dev_model_refit_workspace(st.Q, st.B, self.M),
                          (torch.int32, torch.float64, torch.int32) + _TRIM_KINDS, out, call_trimmed)

        def call(src, dst, T_step, n_close, sum_d2, empty, ws):
            check(lib().pcreg_dev_model_refit_f32(self.handle, *st.q_args, _p(src), st.B, r2, _p(dst), _p(T_step), _p(n_close), _p(sum_d2), _p(empty),
                                                  _p(ws), ws.numel(), _stream()))
        return st.run(self, "_refit_ws_t", lib().pcreg_dev_model_refit_workspace(st.Q, st.B, self.M), (torch.int32, torch.float64, torch.int32), out, call)

    def refit_plane(self, q_soa: torch.Tensor, T_dev: torch.Tensor, r2: float, normals: torch.Tensor, steps: int = 1, out=None, keep_ratio=None):
        """B transforms refitted by the linearised point-to-plane step, `steps` times over, on torch's current stream
        (pcreg_dev_model_refit_plane_f32 once per step, a step's T_out the next one's input, no host synchronisation in between;
        the contract is pcreg_model_refit_plane_f32's): q_soa, T_dev, r2 and steps as refit_transforms takes them; normals the
        [3, M] float32 tensor PreparedModel.normals returns (by ORIGINAL row; a row with a non-finite component offers no plane;
        the sign is immaterial) -> (T_out [B, 16], T_step [B, 16], n_close [B] int32, sum_d2 [B] float64, n_plane [B] int32,
        sum_res2 [B] float64, empty [B] int32), the counts and sums for the transform that went INTO the last step.  T_dev and
        normals are not written.  The workspace and the second transform block are cached on the model; calls that may overlap
        on two streams pass buffers of their own, out=(T_out, T_step, n_close, sum_d2, n_plane, sum_res2, empty, ws, T_tmp) with
        ws of pcreg_dev_model_refit_plane_workspace(Q, B, M) bytes and T_tmp [B, 16] float64 (None with steps = 1).
        keep_ratio (None: this call, untouched): a number in (0, 1] takes the trimmed entry (pcreg_dev_model_refit_plane_trimmed_f32) -- of each
        transform's pairs within r2 only the closest keep_ratio share is kept, ties to the lower query -- and two more tensors
        end the tuple: n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B] float32, the largest kept squared
        distance (+inf where nothing is kept); `out` then holds them too, before ws, which is the size it is without keep_ratio.  Every step trims anew."""
        st = _RefitSteps(q_soa, T_dev, steps)
        M = self.M
        if (normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3 or normals.shape[1] != M or (M and normals.stride(1) != 1)
                or normals.device != q_soa.device):
            raise TypeError("normals are a [3, M] float32 tensor with contiguous rows on the queries' device (the row stride is the leading dimension)")
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        nrm = normals if M else torch.zeros((3, 1), dtype=torch.float32, device=st.dev)      # (no rows: any address, never read)
        if keep_ratio is not None:
            keep_ratio = _keep_ratio(keep_ratio)

            def call_trimmed(src, dst, T_step, n_close, sum_d2, n_plane, sum_res2, empty, n_within, d2_cut, ws):
                check(lib().pcreg_dev_model_refit_plane_trimmed_f32(self.handle, *st.q_args, _p(src), st.B, r2, keep_ratio, _p(nrm),
                                                                    max(int(nrm.stride(0)), M), _p(dst), _p(T_step), _p(n_close), _p(sum_d2), _p(n_plane),
                                                                    _p(sum_res2), _p(empty), _p(ws), ws.numel(), _stream(), _p(n_within), _p(d2_cut)))
            return st.run(self, "_refit_plane_ws_t", lib().pcreg_dev_model_refit_plane_workspace(st.Q, st.B, M),
                          (torch.int32, torch.float64, torch.int32, torch.float64, torch.int32) + _TRIM_KINDS, out, call_trimmed)

        def call(src, dst, T_step, n_close, sum_d2, n_plane, sum_res2, empty, ws):
            check(lib().pcreg_dev_model_refit_plane_f32(self.handle, *st.q_args, _p(src), st.B, r2, _p(nrm), max(int(nrm.stride(0)), M), _p(dst),
                                                        _p(T_step), _p(n_close), _p(sum_d2), _p(n_plane), _p(sum_res2), _p(empty), _p(ws), ws.numel(),
                                                        _stream()))
        return st.run(self, "_refit_plane_ws_t", lib().pcreg_dev_model_refit_plane_workspace(st.Q, st.B, M),
                      (torch.int32, torch.float64, torch.int32, torch.float64, torch.int32), out, call)

    def refit_gicp(self, q_soa: torch.Tensor, T_dev: torch.Tensor, r2: float, normals: torch.Tensor, q_normals: torch.Tensor, epsilon: float = 1e-3,
                   steps: int = 1, out=None):
        """B transforms refitted by the plane-to-plane (generalized ICP) step, `steps` times over, on torch's current stream
        (pcreg_dev_model_refit_gicp_f32 once per step, a step's T_out the next one's input, no host synchronisation in between;
        the contract is pcreg_model_refit_gicp_f32's): q_soa, T_dev, r2, normals and steps as refit_plane takes them; q_normals
        the [3, Q] float32 tensor PreparedModel.normals returns for a model made of the queries (by query; the signs are
        immaterial); epsilon in (0, 1] -> (T_out [B, 16], T_step [B, 16], n_close [B] int32, sum_d2 [B] float64, n_pairs [B]
        int32, sum_res2 [B] float64, empty [B] int32), the counts and sums for the transform that went INTO the last step.
        Nothing given is written.  The workspace and the second transform block are cached on the model; calls that may overlap
        on two streams pass buffers of their own, out=(T_out, T_step, n_close, sum_d2, n_pairs, sum_res2, empty, ws, T_tmp) with
        ws of pcreg_dev_model_refit_gicp_workspace(Q, B, M) bytes and T_tmp [B, 16] float64 (None with steps = 1)."""
        return self._refit_gicp(q_soa, T_dev, r2, normals, q_normals, epsilon, steps, out, None)

    def refit_gicp_trimmed(self, q_soa: torch.Tensor, T_dev: torch.Tensor, r2: float, keep_ratio: float, normals: torch.Tensor, q_normals: torch.Tensor,
                           epsilon: float = 1e-3, steps: int = 1, out=None):
        """refit_gicp with keep_ratio, a number in (0, 1] (pcreg_dev_model_refit_gicp_trimmed_f32): of each transform's
        pairs within r2 every step keeps only the closest keep_ratio share, ties to the lower query, and two more tensors end the
        tuple: n_within [B] int32, the pairs within r2 before the trim, and d2_cut [B] float32, the largest kept squared distance
        (+inf where nothing is kept); `out` holds them too, before ws, which has refit_gicp's size.  (A method of its own where refit_transforms and refit_plane take a keyword: refit_gicp's parameter list is
        pinned by tests/test_refit_gicp_abi.py.)"""
        return self._refit_gicp(q_soa, T_dev, r2, normals, q_normals, epsilon, steps, out, _keep_ratio(keep_ratio))

    def _refit_gicp(self, q_soa, T_dev, r2, normals, q_normals, epsilon, steps, out, keep_ratio):
        st = _RefitSteps(q_soa, T_dev, steps)
        M, Q = self.M, st.Q
        if (normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3 or normals.shape[1] != M or (M and normals.stride(1) != 1)
                or normals.device != q_soa.device):
            raise TypeError("normals are a [3, M] float32 tensor with contiguous rows on the queries' device (the row stride is the leading dimension)")
        if (q_normals.dtype != torch.float32 or q_normals.dim() != 2 or q_normals.shape[0] != 3 or q_normals.shape[1] != Q
                or (Q and q_normals.stride(1) != 1) or q_normals.device != q_soa.device):
            raise TypeError("query normals are a [3, Q] float32 tensor with contiguous rows on the queries' device (the row stride is the leading dimension)")
        r2, epsilon = float(r2), float(epsilon)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        if not 0.0 < epsilon <= 1.0:
            raise ValueError(f"epsilon must lie in (0, 1], got {epsilon}")
        nrm = normals if M else torch.zeros((3, 1), dtype=torch.float32, device=st.dev)      # (no rows: any address, never read)
        if keep_ratio is not None:

            def call_trimmed(src, dst, T_step, n_close, sum_d2, n_pairs, sum_res2, empty, n_within, d2_cut, ws):
                check(lib().pcreg_dev_model_refit_gicp_trimmed_f32(self.handle, *st.q_args, _p(src), st.B, r2, keep_ratio, _p(nrm),
                                                                   max(int(nrm.stride(0)), M), _p(q_normals) if Q else None,
                                                                   max(int(q_normals.stride(0)), Q, 1) if Q else 1, epsilon, _p(dst), _p(T_step),
                                                                   _p(n_close), _p(sum_d2), _p(n_pairs), _p(sum_res2), _p(empty), _p(ws), ws.numel(),
                                                                   _stream(), _p(n_within), _p(d2_cut)))
            return st.run(self, "_refit_gicp_ws_t", lib().pcreg_dev_model_refit_gicp_workspace(Q, st.B, M),
                          (torch.int32, torch.float64, torch.int32, torch.float64, torch.int32) + _TRIM_KINDS, out, call_trimmed)

        def call(src, dst, T_step, n_close, sum_d2, n_pairs, sum_res2, empty, ws):
            check(lib().pcreg_dev_model_refit_gicp_f32(self.handle, *st.q_args, _p(src), st.B, r2, _p(nrm), max(int(nrm.stride(0)), M),
                                                       _p(q_normals) if Q else None, max(int(q_normals.stride(0)), Q, 1) if Q else 1, epsilon, _p(dst),
                                                       _p(T_step), _p(n_close), _p(sum_d2), _p(n_pairs), _p(sum_res2), _p(empty), _p(ws), ws.numel(),
                                                       _stream()))
        return st.run(self, "_refit_gicp_ws_t", lib().pcreg_dev_model_refit_gicp_workspace(Q, st.B, M),
                      (torch.int32, torch.float64, torch.int32, torch.float64, torch.int32), out, call)

    def refit_cpd(self, q_soa: torch.Tensor, T_dev: torch.Tensor, sigma2=0.0, outlier: float = 0.1, steps: int = 1, out=None):
        """B transforms refitted by the coherent-point-drift step (rigid CPD), `steps` times over, on torch's current stream
        (pcreg_dev_model_refit_cpd_f32 once per step, a step's T_out and sigma2_out the next one's inputs, no host
        synchronisation in between; the contract is pcreg_model_refit_cpd_f32's): q_soa and T_dev as refit_transforms takes them;
        sigma2 a number or a [B] float64 tensor on the queries' device, 0 asking for the closed-form initial variance; outlier
        in [0, 1).  The cost is B * Q * M pairs a step: for downsampled clouds.  -> (T_out [B, 16], T_step [B, 16], sigma2_out [B]
        float64, Np [B] float64, sum_res2 [B] float64, sum_d2 [B] float64, n_live [B] int32, empty [B] int32), the sums and
        counts for the transform that went INTO the last step.  Nothing given is written.  The workspace and the second
        transform block are cached on the model; calls that may overlap on two streams pass buffers of their own,
        out=(T_out, T_step, sigma2_out, Np, sum_res2, sum_d2, n_live, empty, ws, T_tmp) with ws of
        pcreg_dev_model_refit_cpd_workspace(Q, B, M) bytes and T_tmp [B, 16] float64 (None with steps = 1)."""
        st = _RefitSteps(q_soa, T_dev, steps)
        outlier = float(outlier)
        if not 0.0 <= outlier < 1.0:
            raise ValueError(f"outlier must lie in [0, 1), got {outlier}")
        if isinstance(sigma2, torch.Tensor):
            if sigma2.dtype != torch.float64 or not sigma2.is_contiguous() or sigma2.numel() != st.B or sigma2.device != st.dev:
                raise TypeError("sigma2 is a number or a contiguous float64 tensor of B numbers on the queries' device")
            sig = sigma2
        else:
            sig = torch.full((max(st.B, 1),), float(sigma2), dtype=torch.float64, device=st.dev)

        def call(src, dst, T_step, sigma2_out, Np, sum_res2, sum_d2, n_live, empty, ws):
            nonlocal sig
            check(lib().pcreg_dev_model_refit_cpd_f32(self.handle, *st.q_args, _p(src), st.B, _p(sig), outlier, _p(dst), _p(T_step), _p(sigma2_out),
                                                      _p(Np), _p(sum_res2), _p(sum_d2), _p(n_live), _p(empty), _p(ws), ws.numel(), _stream()))
            sig = sigma2_out                           # (sigma2_out may alias sigma2_in: a step reads it before its last kernel writes it)
        return st.run(self, "_refit_cpd_ws_t", lib().pcreg_dev_model_refit_cpd_workspace(st.Q, st.B, self.M),
                      (torch.float64, torch.float64, torch.float64, torch.float64, torch.int32, torch.int32), out, call)

    def cluster(self, r2: float, out=None):
        """clusterPoints(model, r) over the model's own rows with r2 = r^2, on torch's current stream
        (pcreg_dev_model_cluster_f32): -> (label [M] int32, the 0-based cluster of every row; n_clusters [1] int32; first [M]
        int32, first[c] the smallest row of cluster c; sizes [M] int32, sizes[c] its rows; both zero at and past n_clusters).
        Clusters are numbered in ascending order of their smallest row.  Nothing synchronises.  The workspace is cached on the
        model and grown on demand; calls that may overlap on two streams pass buffers of their own, out=(label, n_clusters,
        first, sizes, ws) with ws of pcreg_dev_model_cluster_workspace(M) bytes."""
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_cluster_workspace(M)), 256)
        if out is not None:
            label, n_clusters, first, sizes, ws = out
        else:
            label, first, sizes = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3))
            n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
            ws = getattr(self, "_cluster_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._cluster_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if M == 0:                                     # (an empty tensor has no address to pass)
            n_clusters.zero_()
            return label, n_clusters, first, sizes
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_cluster_f32(self.handle, r2, _p(label), _p(n_clusters), _p(first), _p(sizes), _p(ws), ws.numel(), _stream()))
        return label, n_clusters, first, sizes

    def dbscan(self, r2: float, minpts: int, out=None):
        """DBSCAN of the model's own rows with r2 = epsilon^2 and minpts >= 1, on torch's current stream
        (pcreg_dev_model_dbscan_f32; the contract is pcreg_model_dbscan_f32's): -> (label [M] int32, the 0-based cluster of every
        row, -1 for noise; n_clusters [1] int32; core [M] uint8; count [M] int32, the rows within the radius of every row, itself
        included; first [M] int32, first[c] the smallest core row of cluster c; sizes [M] int32, sizes[c] its rows, border rows
        included; both zero at and past n_clusters).  Nothing synchronises.  The workspace is cached on the model and grown on
        demand; calls that may overlap on two streams pass buffers of their own, out=(label, n_clusters, core, count, first,
        sizes, ws) with ws of pcreg_dev_model_dbscan_workspace(M) bytes."""
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        if int(minpts) != minpts or int(minpts) < 1:
            raise ValueError(f"minpts must be a whole number >= 1, got {minpts}")
        minpts = int(minpts)
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_dbscan_workspace(M)), 256)
        if out is not None:
            label, n_clusters, core, count, first, sizes, ws = out
        else:
            label, count, first, sizes = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(4))
            core = torch.empty(M, dtype=torch.uint8, device=dev)
            n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
            ws = getattr(self, "_dbscan_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._dbscan_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if M == 0:                                     # (an empty tensor has no address to pass)
            n_clusters.zero_()
            return label, n_clusters, core, count, first, sizes
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_dbscan_f32(self.handle, r2, minpts, _p(label), _p(n_clusters), _p(core), _p(count), _p(first), _p(sizes),
                                                   _p(ws), ws.numel(), _stream()))
        return label, n_clusters, core, count, first, sizes

    def normals(self, k: int, viewpoint=None, variation: bool = False, out=None):
        """The surface normal of every row of the model from its k nearest rows (3 <= k <= 32), on torch's current stream
        (pcreg_dev_model_normals_f32; the contract is pcreg_model_normals_f32's): -> normals, a [3, M] float32 tensor (row c the
        c-th component of every row's normal: column-major M x 3, by ORIGINAL row), and with variation=True (normals, variation
        [M] float32).  viewpoint: three host numbers, the normals point towards it; None: the component of largest magnitude is
        non-negative.  NaN for a non-finite row, fewer than three finite rows, coincident neighbours.  Nothing synchronises.  The
        workspace is cached on the model and grown on demand; calls that may overlap on two streams pass buffers of their own,
        out=(normals, variation, ws) with ws of pcreg_dev_model_normals_workspace(M, k) bytes (variation None when not wanted)."""
        k = int(k)
        if not 3 <= k <= _l.KNN_MAX_K:
            raise ValueError(f"k must lie in [3, {_l.KNN_MAX_K}], got {k}")
        vp = None
        if viewpoint is not None:
            vp = (C.c_double * 3)(*[float(x) for x in viewpoint])
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_normals_workspace(M, k)), 256)
        if out is not None:
            nrm, var, ws = out
            if nrm.dtype != torch.float32 or nrm.dim() != 2 or nrm.shape[0] != 3 or nrm.shape[1] != M or (M and nrm.stride(1) != 1):
                raise TypeError("normals are a [3, M] float32 tensor with contiguous rows (the row stride is the leading dimension)")
        else:
            nrm = torch.empty((3, M), dtype=torch.float32, device=dev)
            var = torch.empty(M, dtype=torch.float32, device=dev) if variation else None
            ws = getattr(self, "_normals_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._normals_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if M:                                          # (an empty tensor has no address to pass)
            with torch.cuda.device(dev):
                check(lib().pcreg_dev_model_normals_f32(self.handle, k, vp, _p(nrm), max(int(nrm.stride(0)), M), _p(var) if var is not None else None,
                                                        _p(ws), ws.numel(), _stream()))
        return (nrm, var) if variation else nrm

    def fpfh(self, k: int, normals: torch.Tensor, spfh: bool = False, out=None):
        """The FPFH descriptor of every row of the model from its k nearest rows (3 <= k <= 32) and a normal per row, on torch's
        current stream (pcreg_dev_model_fpfh_f32; the contract is pcreg_model_fpfh_f32's): normals the [3, M] float32 tensor
        PreparedModel.normals returns (by ORIGINAL row; THE SIGN matters: orient them with a viewpoint) -> fpfh, an [M, 33] float64
        tensor, row-major by ORIGINAL row (what pcreg_dev_get_matches takes as row-major descriptors), and with spfh=True (fpfh,
        counts [M, 33] uint8).  A non-finite row is NaN.  Nothing synchronises.  The workspace is cached on the model and grown on
        demand; calls that may overlap on two streams pass buffers of their own, out=(fpfh, counts, ws) with ws of
        pcreg_dev_model_fpfh_workspace(M, k) bytes (counts None when not wanted)."""
        k = int(k)
        if not 3 <= k <= _l.KNN_MAX_K:
            raise ValueError(f"k (NumNeighbors) must lie in [3, {_l.KNN_MAX_K}], got {k}")
        dev, M = self.tensor.device, self.M
        if (normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3 or normals.shape[1] != M or (M and normals.stride(1) != 1)
                or normals.device != dev):
            raise TypeError("normals are a [3, M] float32 tensor with contiguous rows on the model's device (the row stride is the leading dimension)")
        need = max(int(lib().pcreg_dev_model_fpfh_workspace(M, k)), 256)
        if out is not None:
            desc, cnt, ws = out
            if desc.dtype != torch.float64 or desc.shape != (M, 33) or not desc.is_contiguous():
                raise TypeError("fpfh is a contiguous [M, 33] float64 tensor")
            if cnt is not None and (cnt.dtype != torch.uint8 or cnt.shape != (M, 33) or not cnt.is_contiguous()):
                raise TypeError("the SPFH counts are a contiguous [M, 33] uint8 tensor")
        else:
            desc = torch.empty((M, 33), dtype=torch.float64, device=dev)
            cnt = torch.empty((M, 33), dtype=torch.uint8, device=dev) if spfh else None
            ws = getattr(self, "_fpfh_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fpfh_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if M:                                          # (an empty tensor has no address to pass)
            with torch.cuda.device(dev):
                check(lib().pcreg_dev_model_fpfh_f32(self.handle, k, _p(normals), max(int(normals.stride(0)), M), _p(desc),
                                                     _p(cnt) if cnt is not None else None, _p(ws), ws.numel(), _stream()))
        return (desc, cnt) if spfh else desc

    def fpfh_radius_count(self, r2: float, out=None):
        """The first of the radius FPFH's two calls, on torch's current stream (pcreg_dev_model_fpfh_radius_count_f32): the rows
        within the SQUARED radius r2 of every row of the model, the row itself included -> (counts [M] int32, seg_off [M + 1]
        int64).  Nothing synchronises: the caller reads seg_off[M], the total, sizes the lists with it and calls fpfh_radius.
        out=(counts, seg_off, ws) with ws of pcreg_dev_model_fpfh_radius_workspace(M, 0) bytes for calls that may overlap."""
        r2 = float(r2)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_fpfh_radius_workspace(M, 0)), 256)
        if out is not None:
            counts, seg_off, ws = out
        else:
            counts = torch.empty(M, dtype=torch.int32, device=dev)
            seg_off = torch.empty(M + 1, dtype=torch.int64, device=dev)
            ws = getattr(self, "_fpfh_radius_cws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fpfh_radius_cws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_fpfh_radius_count_f32(self.handle, r2, _p(counts) if M else None, _p(seg_off), _p(ws), ws.numel(), _stream()))
        return counts, seg_off

    def fpfh_radius(self, r2: float, normals: torch.Tensor, seg_off: torch.Tensor, capacity: int, max_neighbors: int = 0, spfh: bool = False,
                    out=None):
        """The second call (pcreg_dev_model_fpfh_radius_f32; the contract is pcreg_model_fpfh_radius_f32's): r2 and seg_off as
        fpfh_radius_count took and returned them, capacity >= seg_off[M] (the host's copy of the total: a smaller one truncates
        segments and leaves those rows' descriptors unspecified), normals the [3, M] float32 tensor PreparedModel.normals
        returns, max_neighbors = n > 0 to count only the n nearest rows within the radius -> (fpfh [M, 33] float64, n_neighbors [M]
        int32), and with spfh=True (fpfh, counts [M, 33], n_neighbors), row-major by ORIGINAL row; the counts are the library's uint32 in
        an int32 tensor (a count is below M).  Nothing synchronises.  The
        workspace (8 bytes per list entry and the rest) is cached on the model and grown on demand; calls that may overlap on two
        streams pass buffers of their own, out=(fpfh, counts, n_neighbors, ws) with ws of
        pcreg_dev_model_fpfh_radius_workspace(M, capacity) bytes (counts and n_neighbors None when not wanted)."""
        r2, n, capacity = float(r2), int(max_neighbors), int(capacity)
        if not r2 >= 0.0:
            raise ValueError(f"r2 (the squared radius) must be a number >= 0, got {r2}")
        if n < 0 or capacity < 0:
            raise ValueError(f"max_neighbors and capacity must be >= 0, got {n} and {capacity}")
        dev, M = self.tensor.device, self.M
        if (normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3 or normals.shape[1] != M or (M and normals.stride(1) != 1)
                or normals.device != dev):
            raise TypeError("normals are a [3, M] float32 tensor with contiguous rows on the model's device (the row stride is the leading dimension)")
        if seg_off.dtype != torch.int64 or seg_off.shape != (M + 1,) or not seg_off.is_contiguous() or seg_off.device != dev:
            raise TypeError("seg_off is the contiguous [M + 1] int64 tensor fpfh_radius_count returns")
        need = max(int(lib().pcreg_dev_model_fpfh_radius_workspace(M, capacity)), 256)
        if out is not None:
            desc, cnt, nn, ws = out
            if desc.dtype != torch.float64 or desc.shape != (M, 33) or not desc.is_contiguous():
                raise TypeError("fpfh is a contiguous [M, 33] float64 tensor")
            if cnt is not None and (cnt.dtype != torch.int32 or cnt.shape != (M, 33) or not cnt.is_contiguous()):
                raise TypeError("the SPFH counts are a contiguous [M, 33] int32 tensor")
            if nn is not None and (nn.dtype != torch.int32 or nn.shape != (M,) or not nn.is_contiguous()):
                raise TypeError("n_neighbors is a contiguous [M] int32 tensor")
        else:
            desc = torch.empty((M, 33), dtype=torch.float64, device=dev)
            cnt = torch.empty((M, 33), dtype=torch.int32, device=dev) if spfh else None
            nn = torch.empty(M, dtype=torch.int32, device=dev)
            ws = getattr(self, "_fpfh_radius_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fpfh_radius_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        if M:                                          # (an empty tensor has no address to pass)
            with torch.cuda.device(dev):
                check(lib().pcreg_dev_model_fpfh_radius_f32(self.handle, r2, n, _p(normals), max(int(normals.stride(0)), M), _p(seg_off), capacity,
                                                            _p(desc), _p(cnt) if cnt is not None else None, _p(nn) if nn is not None else None,
                                                            _p(ws), ws.numel(), _stream()))
        return (desc, cnt, nn) if spfh else (desc, nn)

    def iss_keypoints(self, salient_radius, nonmax_radius, gamma21: float = 0.975, gamma32: float = 0.975, min_neighbors: int = 5,
                      eig: bool = True, out=None):
        """The ISS keypoints of the model's own rows on torch's current stream (pcreg_dev_model_iss_f32; the contract is
        pcreg_model_iss_f32's; the radii are squared in double and rounded once to float32): -> a dict of device tensors --
        n_neighbors [M] int32, eig [M, 3] float64 descending (None with eig=False) and saliency [M] float64 by ORIGINAL row;
        keypoints, an [M] int32 tensor whose first n_keypoints [1] int32 entries are the 0-based keypoint rows, ascending (the
        rest is not written).  Nothing synchronises: the caller reads n_keypoints when it needs it, and
        fpfh[keypoints[:n].long()] feeds pcreg_dev_get_matches without a trip through the host.  The workspace is cached on the
        model and grown on demand; calls that may overlap on two streams pass buffers of their own,
        out=(n_neighbors, eig, saliency, keypoints, n_keypoints, ws) with ws of pcreg_dev_model_iss_workspace(M) bytes."""
        from .api import iss_args
        a = iss_args(salient_radius, nonmax_radius, gamma21, gamma32, min_neighbors)
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_iss_workspace(M)), 256)
        if out is not None:
            nn, ev, sal, kp, n_kp, ws = out
        else:
            nn = torch.empty(M, dtype=torch.int32, device=dev)
            ev = torch.empty((M, 3), dtype=torch.float64, device=dev) if eig else None
            sal = torch.empty(M, dtype=torch.float64, device=dev)
            kp = torch.empty(M, dtype=torch.int32, device=dev)
            n_kp = torch.empty(1, dtype=torch.int32, device=dev)
            ws = getattr(self, "_iss_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._iss_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda t: _p(t) if t is not None and t.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_iss_f32(self.handle, *a, opt(nn), opt(ev), opt(sal), opt(kp), opt(n_kp), _p(ws), ws.numel(), _stream()))
        return dict(n_neighbors=nn, eig=ev, saliency=sal, keypoints=kp, n_keypoints=n_kp)

    def fit_planes(self, max_distance, ref_vec=None, max_angle=math.pi / 2, max_planes: int = 1, n_trials: int = 1000,
                   min_inliers: int = 3, seed: int = 0, samples=None, idx_base: int = 0, out=None):
        """MSAC plane fitting and extraction over the model's own rows on torch's current stream (pcreg_dev_model_fit_planes_f32; the
        contract is pcreg_model_fit_planes_f32's): -> a dict of device tensors -- labels [M] int32 (plane p's rows carry p + 1),
        planes [P, 4] float64, centres [P, 3], counts [P] int32, rmse [P], n_planes [1] int32 and the diagnostics best_trial,
        best_cost (int64), best_count [P].  samples is an int32 device tensor [max_planes, n_trials, 3] of rows counted from idx_base,
        or None for the sampler.  Nothing synchronises: the caller reads n_planes when it needs it.  The workspace is cached on the
        model and grown on demand; calls that may overlap on two streams pass buffers of their own, out=(labels, planes, centres,
        counts, rmse, n_planes, best_trial, best_cost, best_count, ws) with ws of pcreg_dev_model_fit_planes_workspace(M, n_trials)
        bytes."""
        from .api import planes_args
        t, rv, ang, P, B, mi, sd = planes_args(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed)
        dev, M = self.tensor.device, self.M
        if samples is not None and (samples.dtype != torch.int32 or tuple(samples.shape) != (P, B, 3) or not samples.is_contiguous()
                                    or samples.device != dev):
            raise ValueError(f"samples must be a contiguous int32 tensor {(P, B, 3)} on the model's device")
        need = max(int(lib().pcreg_dev_model_fit_planes_workspace(M, B)), 256)
        if out is not None:
            lab, pl, ce, cnt, rm, n_pl, bt, bc, bn, ws = out
        else:
            lab = torch.empty(M, dtype=torch.int32, device=dev)
            pl = torch.empty((P, 4), dtype=torch.float64, device=dev)
            ce = torch.empty((P, 3), dtype=torch.float64, device=dev)
            cnt = torch.empty(P, dtype=torch.int32, device=dev)
            rm = torch.empty(P, dtype=torch.float64, device=dev)
            n_pl = torch.empty(1, dtype=torch.int32, device=dev)
            bt = torch.empty(P, dtype=torch.int32, device=dev)
            bc = torch.empty(P, dtype=torch.int64, device=dev)
            bn = torch.empty(P, dtype=torch.int32, device=dev)
            ws = getattr(self, "_planes_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._planes_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda x: _p(x) if x is not None and x.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_fit_planes_f32(self.handle, t, rv.ctypes.data if rv is not None else None, ang, P, B, mi, sd, opt(samples),
                                                       int(idx_base), opt(lab), opt(pl), opt(ce), opt(cnt), opt(rm), opt(n_pl), opt(bt), opt(bc),
                                                       opt(bn), _p(ws), ws.numel(), _stream()))
        return dict(labels=lab, planes=pl, centres=ce, counts=cnt, rmse=rm, n_planes=n_pl, best_trial=bt, best_cost=bc, best_count=bn)

    def fit_spheres(self, max_distance, min_radius: float = 0.0, max_radius: float = math.inf, max_spheres: int = 1,
                    n_trials: int = 1000, min_inliers: int = 4, seed: int = 0, samples=None, idx_base: int = 0, out=None):
        """MSAC sphere fitting and extraction over the model's own rows on torch's current stream (pcreg_dev_model_fit_spheres_f32;
        the contract is pcreg_model_fit_spheres_f32's): -> a dict of device tensors -- labels [M] int32 (sphere p's rows carry
        p + 1), spheres [P, 4] float64 (cx, cy, cz, R), counts [P] int32, rmse [P], refit_used [P] int32, n_spheres [1] int32 and
        the diagnostics best_trial, best_cost (int64), best_count [P].  samples is an int32 device tensor [max_spheres, n_trials, 4]
        of rows counted from idx_base, or None for the sampler.  Nothing synchronises: the caller reads n_spheres when it needs it.
        The workspace is cached on the model and grown on demand; calls that may overlap on two streams pass buffers of their own,
        out=(labels, spheres, counts, rmse, refit_used, n_spheres, best_trial, best_cost, best_count, ws) with ws of
        pcreg_dev_model_fit_spheres_workspace(M, n_trials) bytes."""
        from .api import fit_spheres_args
        t, r0, r1, P, B, mi, sd = fit_spheres_args(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed)
        dev, M = self.tensor.device, self.M
        if samples is not None and (samples.dtype != torch.int32 or tuple(samples.shape) != (P, B, 4) or not samples.is_contiguous()
                                    or samples.device != dev):
            raise ValueError(f"samples must be a contiguous int32 tensor {(P, B, 4)} on the model's device")
        need = max(int(lib().pcreg_dev_model_fit_spheres_workspace(M, B)), 256)
        if out is not None:
            lab, sp, cnt, rm, used, n_sp, bt, bc, bn, ws = out
        else:
            lab = torch.empty(M, dtype=torch.int32, device=dev)
            sp = torch.empty((P, 4), dtype=torch.float64, device=dev)
            cnt = torch.empty(P, dtype=torch.int32, device=dev)
            rm = torch.empty(P, dtype=torch.float64, device=dev)
            used = torch.empty(P, dtype=torch.int32, device=dev)
            n_sp = torch.empty(1, dtype=torch.int32, device=dev)
            bt = torch.empty(P, dtype=torch.int32, device=dev)
            bc = torch.empty(P, dtype=torch.int64, device=dev)
            bn = torch.empty(P, dtype=torch.int32, device=dev)
            ws = getattr(self, "_fit_spheres_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fit_spheres_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda x: _p(x) if x is not None and x.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_fit_spheres_f32(self.handle, t, r0, r1, P, B, mi, sd, opt(samples), int(idx_base), opt(lab), opt(sp),
                                                        opt(cnt), opt(rm), opt(used), opt(n_sp), opt(bt), opt(bc), opt(bn), _p(ws), ws.numel(),
                                                        _stream()))
        return dict(labels=lab, spheres=sp, counts=cnt, rmse=rm, refit_used=used, n_spheres=n_sp, best_trial=bt, best_cost=bc, best_count=bn)

    def fit_cylinders(self, max_distance, normals: torch.Tensor, min_radius: float = 0.0, max_radius: float = math.inf, ref_vec=None,
                      max_angle=math.pi / 2, max_cylinders: int = 1, n_trials: int = 1000, min_inliers: int = 4, seed: int = 0,
                      samples=None, idx_base: int = 0, out=None):
        """MSAC cylinder fitting and extraction over the model's own rows on torch's current stream
        (pcreg_dev_model_fit_cylinders_f32; the contract is pcreg_model_fit_cylinders_f32's): normals the [3, M] float32 tensor
        PreparedModel.normals returns (by ORIGINAL row; their sign does not matter) -> a dict of device tensors -- labels [M] int32
        (cylinder p's rows carry p + 1), cylinders [P, 7] float64 (cx, cy, cz, wx, wy, wz, R), extents [P, 2] float64 (h_lo, h_hi
        along the axis from the centre), counts [P] int32, rmse [P], refit_used [P] int32, n_cylinders [1] int32 and the diagnostics
        best_trial, best_cost (int64), best_count [P].  ref_vec (three host numbers) and max_angle (radians) bound the axis.
        samples is an int32 device tensor [max_cylinders, n_trials, 2] of rows counted from idx_base, or None for the sampler.
        Nothing synchronises: the caller reads n_cylinders when it needs it.  The workspace is cached on the model and grown on
        demand; calls that may overlap on two streams pass buffers of their own, out=(labels, cylinders, extents, counts, rmse,
        refit_used, n_cylinders, best_trial, best_cost, best_count, ws) with ws of pcreg_dev_model_fit_cylinders_workspace(M,
        n_trials) bytes."""
        from .api import fit_cylinders_args
        t, r0, r1, rv, ang, P, B, mi, sd = fit_cylinders_args(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders,
                                                              n_trials, min_inliers, seed)
        dev, M = self.tensor.device, self.M
        if (normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3 or normals.shape[1] != M or (M and normals.stride(1) != 1)
                or normals.device != dev):
            raise TypeError("normals are a [3, M] float32 tensor with contiguous rows on the model's device (the row stride is the leading dimension)")
        if samples is not None and (samples.dtype != torch.int32 or tuple(samples.shape) != (P, B, 2) or not samples.is_contiguous()
                                    or samples.device != dev):
            raise ValueError(f"samples must be a contiguous int32 tensor {(P, B, 2)} on the model's device")
        need = max(int(lib().pcreg_dev_model_fit_cylinders_workspace(M, B)), 256)
        if out is not None:
            lab, cy, ex, cnt, rm, used, n_cy, bt, bc, bn, ws = out
        else:
            lab = torch.empty(M, dtype=torch.int32, device=dev)
            cy = torch.empty((P, 7), dtype=torch.float64, device=dev)
            ex = torch.empty((P, 2), dtype=torch.float64, device=dev)
            cnt = torch.empty(P, dtype=torch.int32, device=dev)
            rm = torch.empty(P, dtype=torch.float64, device=dev)
            used = torch.empty(P, dtype=torch.int32, device=dev)
            n_cy = torch.empty(1, dtype=torch.int32, device=dev)
            bt = torch.empty(P, dtype=torch.int32, device=dev)
            bc = torch.empty(P, dtype=torch.int64, device=dev)
            bn = torch.empty(P, dtype=torch.int32, device=dev)
            ws = getattr(self, "_fit_cylinders_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fit_cylinders_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda x: _p(x) if x is not None and x.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_fit_cylinders_f32(self.handle, t, r0, r1, rv.ctypes.data if rv is not None else None, ang, opt(normals),
                                                          max(int(normals.stride(0)), M), P, B, mi, sd, opt(samples), int(idx_base), opt(lab),
                                                          opt(cy), opt(ex), opt(cnt), opt(rm), opt(used), opt(n_cy), opt(bt), opt(bc), opt(bn),
                                                          _p(ws), ws.numel(), _stream()))
        return dict(labels=lab, cylinders=cy, extents=ex, counts=cnt, rmse=rm, refit_used=used, n_cylinders=n_cy, best_trial=bt, best_cost=bc,
                    best_count=bn)

    def denoise(self, k: int = 4, threshold: float = 1.0, out=None):
        """pcdenoise(model, 'NumNeighbors', k, 'Threshold', threshold) over the model's own rows, on torch's current stream
        (pcreg_dev_model_denoise_f32; the contract is pcreg_model_denoise_f32's): -> a dict of device tensors -- mean_dist [M]
        float64 by ORIGINAL row; inliers, an [M] int32 tensor whose first n_inliers [1] int32 entries are the 0-based rows with
        mean_dist <= thr, ascending (the rest is not written); stats [4] float64 = thr, mean, std, n_finite, also under the
        names thr, mean, std and n_finite as views of it.  Nothing synchronises: the caller reads n_inliers when it needs it.
        The workspace is cached on the model and grown on demand; calls that may overlap on two streams pass buffers of their
        own, out=(mean_dist, inliers, n_inliers, stats, ws) with ws of pcreg_dev_model_denoise_workspace(M, k) bytes."""
        k, threshold = int(k), float(threshold)
        if not 1 <= k <= _l.KNN_MAX_K - 1:
            raise ValueError(f"k (NumNeighbors) must lie in [1, {_l.KNN_MAX_K - 1}], got {k}")
        if not (math.isfinite(threshold) and threshold >= 0.0):
            raise ValueError(f"threshold must be a finite number >= 0, got {threshold}")
        dev, M = self.tensor.device, self.M
        need = max(int(lib().pcreg_dev_model_denoise_workspace(M, k)), 256)
        if out is not None:
            md, inl, n_inl, stats, ws = out
        else:
            md = torch.empty(M, dtype=torch.float64, device=dev)
            inl = torch.empty(M, dtype=torch.int32, device=dev)
            n_inl = torch.empty(1, dtype=torch.int32, device=dev)
            stats = torch.empty(4, dtype=torch.float64, device=dev)
            ws = getattr(self, "_denoise_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._denoise_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda t: _p(t) if t is not None and t.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_denoise_f32(self.handle, k, threshold, opt(md), opt(inl), opt(n_inl), opt(stats), _p(ws), ws.numel(),
                                                    _stream()))
        res = dict(mean_dist=md, inliers=inl, n_inliers=n_inl, stats=stats)
        if stats is not None:
            res.update(thr=stats[0], mean=stats[1], std=stats[2], n_finite=stats[3])
        return res

    def farthest_points(self, K: int, start: int = -1, stop_d2: float = 0.0, out=None):
        """Farthest point sampling of the model's own rows, on torch's current stream (pcreg_dev_model_fps_f32; the contract is
        pcreg_model_fps_f32's): -> a dict of device tensors -- idx [K] int32 and dist [K] float32, whose first n_out [1] int32
        entries are the 0-based original rows in selection order and their squared distances to the earlier samples (the rest is
        not written); cover_d2 [1] float32; min_dist [M] float32 and label [M] int32 by ORIGINAL row; info [1] int32, 1 when the
        start row has a non-finite coordinate (then n_out = 0 and nothing else is written).  Nothing synchronises: the caller reads
        n_out and info when it needs them.  The workspace is cached on the model and grown on demand; calls that may overlap on two
        streams pass buffers of their own, out=(idx, dist, n_out, cover_d2, min_dist, label, info, ws) with ws of
        pcreg_dev_model_fps_workspace(M, K) bytes."""
        K, start, stop_d2 = int(K), int(start), float(stop_d2)
        dev, M = self.tensor.device, self.M
        if K < 0 or (M > 0 and not -1 <= start < M) or not stop_d2 >= 0.0:
            raise ValueError(f"K >= 0, start in -1 .. M - 1 and stop_d2 >= 0 are required, got {K}, {start}, {stop_d2}")
        need = int(lib().pcreg_dev_model_fps_workspace(M, K))
        if need == 0:
            raise ValueError(f"farthest point sampling serves at most 2097152 rows, got {M}")
        if out is not None:
            idx, dist, n_out, cover, md, lab, info, ws = out
        else:
            idx = torch.empty(K, dtype=torch.int32, device=dev)
            dist = torch.empty(K, dtype=torch.float32, device=dev)
            n_out = torch.empty(1, dtype=torch.int32, device=dev)
            cover = torch.empty(1, dtype=torch.float32, device=dev)
            md = torch.empty(M, dtype=torch.float32, device=dev)
            lab = torch.empty(M, dtype=torch.int32, device=dev)
            info = torch.empty(1, dtype=torch.int32, device=dev)
            ws = getattr(self, "_fps_ws_t", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._fps_ws_t = torch.empty(need, dtype=torch.uint8, device=dev)
        opt = lambda t: _p(t) if t is not None and t.numel() else None      # (an empty tensor has no address to pass)
        with torch.cuda.device(dev):
            check(lib().pcreg_dev_model_fps_f32(self.handle, K, start, stop_d2, opt(idx), opt(dist), _p(n_out), opt(cover), opt(md), opt(lab),
                                                opt(info), _p(ws), ws.numel(), _stream()))
        return dict(idx=idx, dist=dist, n_out=n_out, cover_d2=cover, min_dist=md, label=lab, info=info)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().pcreg_dev_model_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_dropped: list = []            # handles replaced by as_prepared(): freed later, not in the middle of a hot loop
_reprepared = 0


def downsample_grid(points_soa: torch.Tensor, step: float, stream=None, out=None):
    """pcdownsample(pc, 'gridAverage', step) on a resident cloud (pcreg_dev_downsample_grid_f32; the contract is
    pcreg_downsample_grid_f32's): points_soa a [3, n] float32 tensor with contiguous rows -> (out [3, n] float32 of which the
    first n_out columns are written, count [n] int32 likewise, label [n] int32: the 1-based output column of every input row, 0
    for a row with a non-finite coordinate; n_out, info: one int32 tensor each on the device).  info is 1 when the cloud spans
    2^21 or more cells along an axis; then n_out is 0 and nothing else is written.  Runs on `stream` (a torch.cuda.Stream) or
    torch's current stream; nothing synchronises -- the one read is the caller's:

        out, count, label, n_out, info = downsample_grid(soa(cloud), 0.5)
        u = int(n_out.item())                                   # the only trip to the host
        coarse = PreparedModel(out[:, :u])                      # a view: the row stride stays n

    Buffers are allocated per call; calls that reuse theirs pass out=(out, count, label, n_out, info, ws) with ws of
    pcreg_dev_downsample_grid_workspace(n) bytes."""
    if points_soa.dtype != torch.float32 or points_soa.dim() != 2 or points_soa.shape[0] != 3 or (points_soa.shape[1] and points_soa.stride(1) != 1):
        raise TypeError("a cloud is a [3, n] float32 tensor with contiguous rows (column-major n x 3)")
    step = float(step)
    if not (step > 0.0 and step != float("inf")):
        raise ValueError(f"step must be a finite number > 0, got {step}")
    n, dev = int(points_soa.shape[1]), points_soa.device
    need = max(int(lib().pcreg_dev_downsample_grid_workspace(n)), 256)
    if out is not None:
        o, count, label, n_out, info, ws = out
    else:
        o = torch.empty((3, n), dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    with torch.cuda.device(dev):
        check(lib().pcreg_dev_downsample_grid_f32(_p(points_soa) if n else None, n, max(int(points_soa.stride(0)), n) if n else 1, step,
                                                  _p(o) if n else None, max(int(o.stride(0)), n) if n else 1, _p(count) if n else None,
                                                  _p(label) if n else None, _p(n_out), _p(info), _p(ws), C.c_size_t(ws.numel()), st))
    return o, count, label, n_out, info


class NdtModel:
    """A cloud summarised ONCE as one Gaussian per occupied voxel (pcreg_dev_ndt_create; the contract is pcreg_ndt's,
    include/pcreg.h), against which candidate transforms are refined by NDT steps that need no nearest-row search.
    points_soa: a [3, n] float32 tensor with contiguous rows; step: the voxel size; min_points: the rows a voxel needs to hold
    a Gaussian.  The build runs on torch's current stream and synchronises it; the handle keeps its own table, not the cloud."""

    def __init__(self, points_soa: torch.Tensor, step: float, min_points: int = 6):
        if points_soa.dtype != torch.float32 or points_soa.dim() != 2 or points_soa.shape[0] != 3 or (points_soa.shape[1] and points_soa.stride(1) != 1):
            raise TypeError("a cloud is a [3, n] float32 tensor with contiguous rows (column-major n x 3)")
        step, min_points = float(step), int(min_points)
        if not (step > 0.0 and step != float("inf")):
            raise ValueError(f"step must be a finite number > 0, got {step}")
        if min_points < 3:
            raise ValueError(f"min_points must be at least 3, got {min_points}")
        n = int(points_soa.shape[1])
        self.device, self.step, self.min_points = points_soa.device, step, min_points
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().pcreg_dev_ndt_create(_p(points_soa) if n else None, n, max(int(points_soa.stride(0)), n) if n else 1, step, min_points,
                                             _stream(), C.byref(self.handle)))
        nv, ng = C.c_int(), C.c_int()
        check(lib().pcreg_dev_ndt_size(self.handle, C.byref(nv), C.byref(ng)))
        self.n_voxels, self.n_gaussians = nv.value, ng.value

    def gaussians(self):
        """-> dict of numpy arrays: cells [G, 3] int32, counts [G] int32, means [G, 3] float64, C [G, 6] float64 (xx xy xz yy yz
        zz of the floored inverse covariance), lo [3] and origin [3] float32; the Gaussians ascend by cell.  Synchronises."""
        import numpy as np
        G = self.n_gaussians
        cells, counts = np.zeros((G, 3), np.int32), np.zeros(G, np.int32)
        means, Cm = np.zeros((G, 3), np.float64), np.zeros((G, 6), np.float64)
        lo, origin = np.zeros(3, np.float32), np.zeros(3, np.float32)
        with torch.cuda.device(self.device):
            check(lib().pcreg_dev_ndt_get(self.handle, cells.ctypes.data, counts.ctypes.data, means.ctypes.data, Cm.ctypes.data, lo.ctypes.data,
                                          origin.ctypes.data))
        return dict(cells=cells, counts=counts, means=means, C=Cm, lo=lo, origin=origin)

    def refit(self, q_soa: torch.Tensor, T_dev: torch.Tensor, neighbors: int = 1, outlier_ratio: float = 0.55, steps: int = 1, out=None):
        """B transforms refined by the NDT step, `steps` times over, on torch's current stream (pcreg_dev_ndt_refit_f32 once per
        step, a step's T_out the next one's input, no host synchronisation): q_soa a [3, Q] float32 tensor with contiguous rows,
        T_dev a contiguous float64 tensor of B x 16 numbers; neighbors 1 (a point's own voxel) or 7 (and its face neighbours)
        -> (T_out [B, 16], T_step [B, 16], n_pairs [B] int32, sum_e [B] float64, empty [B] int32), the counts and sums for the
        transform that went INTO the last step.  T_dev is not written.  The workspace is cached on the handle; calls that may
        overlap on two streams pass buffers of their own, out=(T_out, T_step, n_pairs, sum_e, empty, ws, T_tmp) with ws of
        pcreg_dev_ndt_refit_workspace(Q, B) bytes and T_tmp [B, 16] float64 (None with steps = 1)."""
        st = _RefitSteps(q_soa, T_dev, steps, empty_any_stride=True)
        neighbors, outlier_ratio = int(neighbors), float(outlier_ratio)
        if neighbors not in (1, 7):
            raise ValueError(f"neighbors must be 1 or 7, got {neighbors}")
        if not 0.0 <= outlier_ratio < 1.0:
            raise ValueError(f"outlier_ratio must lie in [0, 1), got {outlier_ratio}")

        def call(src, dst, T_step, n_pairs, sum_e, empty, ws):
            check(lib().pcreg_dev_ndt_refit_f32(self.handle, *st.q_args, _p(src), st.B, neighbors, outlier_ratio, _p(dst), _p(T_step), _p(n_pairs),
                                                _p(sum_e), _p(empty), _p(ws), C.c_size_t(ws.numel()), _stream()))
        return st.run(self, "_refit_ws_t", lib().pcreg_dev_ndt_refit_workspace(st.Q, st.B), (torch.int32, torch.float64, torch.int32), out, call)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().pcreg_dev_ndt_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_dropped() -> None:
    """Free the prepared models that as_prepared() replaced (pcreg_dev_model_destroy synchronises the device: not something to
    do between two launches of a hot loop, which is where a replaced cache entry used to die)."""
    while _dropped:
        _dropped.pop().close()


def _model_key(t: torch.Tensor):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version, t.device.index)


def as_prepared(model, cache: PreparedModel | None = None) -> PreparedModel:
    """model: a PreparedModel (used as is) or a [3, M] tensor -- prepared now, unless `cache` was prepared from the same memory
    (data pointer, shape, strides) and torch has seen no write to it since (`_version`).  A fresh VIEW of the same storage
    (`model[:, :M]`, `soa(x)` returning its input) therefore hits the cache.  Writes through raw pointers (this library's own
    ctypes calls, another stream) are invisible to `_version`: after such a write build a new PreparedModel yourself.
    A replaced entry is parked (release_dropped()) instead of being freed here; repeated re-preparation is reported once."""
    global _reprepared
    if isinstance(model, PreparedModel):
        return model
    if cache is not None and cache.handle.value and cache.key == _model_key(model):
        return cache
    if cache is not None:
        _dropped.append(cache)
        _reprepared += 1
        if _reprepared == 8:
            import warnings
            warnings.warn("pcreg_amd: a model tensor was re-prepared 8 times (box, operand tiles and seeding grid rebuilt per call); "
                          "pass a PreparedModel, or keep the model tensor unmodified between calls", RuntimeWarning, stacklevel=3)
        if len(_dropped) > 4:
            _dropped.pop(0).close()
    return PreparedModel(model)


class HipOps:
    """The `ops` backend of ShardedMatcher on an MI355X (preallocated, no host syncs).  Five launches per match on one
    rank: four for the search against the prepared model, one for filters + Unique + compaction."""

    def __init__(self, Q: int, M_local: int, device: torch.device):
        L = lib()
        self.device, self.Q, self.M_local = device, Q, M_local
        i32, f32, f64 = torch.int32, torch.float32, torch.float64
        kw = dict(device=device)
        self.ws = torch.empty(max(L.pcreg_dev_model_search_workspace(Q, M_local), 256), dtype=torch.uint8, **kw)
        self.top2_local = torch.empty((2, Q, 2), dtype=i32, **kw)        # one buffer: a single all_gather carries both
        self.idx_local = self.top2_local[0]
        self.dist_local = self.top2_local[1].view(f32)
        self.idx = torch.empty((Q, 2), dtype=i32, **kw)
        self.dist = torch.empty((Q, 2), dtype=f32, **kw)
        self.n_pairs = torch.zeros(1, dtype=i32, **kw)
        self.pairs = torch.empty((Q, 2), dtype=i32, **kw)
        self.pts1 = torch.empty((3, Q), dtype=f64, **kw)
        self.pts2 = torch.empty((3, Q), dtype=f64, **kw)
        self.table = torch.zeros((4, Q), dtype=i32, **kw)               # multi-GPU table, column = query (sharded.py step 3)
        self._prepared = None

    def prepared(self, model) -> PreparedModel:
        self._prepared = as_prepared(model, self._prepared)
        if self._prepared.M > self.M_local:
            raise ValueError(f"model of {self._prepared.M} rows, the pipeline was sized for {self.M_local}")
        return self._prepared

    def local_top2(self, q, model, m_lo):
        pm = self.prepared(model)
        check(lib().pcreg_dev_model_search_f32(pm.handle, _p(q), self.Q, q.stride(0), C.c_int32(m_lo), _p(self.idx_local), _p(self.dist_local),
                                               _p(self.ws), C.c_size_t(self.ws.numel()), _stream()))
        return self.idx_local, self.dist_local

    def merge_top2(self, idx_all, dist_all):
        check(lib().pcreg_dev_merge_top2_strided_f32(_p(idx_all), _p(dist_all), idx_all.shape[0], self.Q,
                                                     C.c_size_t(idx_all.stride(0)), _p(self.idx), _p(self.dist), _stream()))
        return self.idx, self.dist

    def match_single(self, q, model, idx, dist, thr, ratio, unique):
        pm = self.prepared(model)
        check(lib().pcreg_dev_model_match_f32(pm.handle, _p(q), self.Q, q.stride(0), _p(idx), _p(dist), C.c_float(thr), C.c_float(ratio),
                                              int(bool(unique)), _p(self.ws), C.c_size_t(self.ws.numel()), _p(self.pairs), _p(self.pts1),
                                              _p(self.pts2), _p(self.n_pairs), _stream()))
        return self.pairs, self.pts1, self.pts2, self.n_pairs

    def match_table(self, q, model, m_lo, M_total, idx, dist, thr, ratio, unique):
        pm = self.prepared(model)
        check(lib().pcreg_dev_model_match_table_f32(pm.handle, C.c_int32(m_lo), M_total, _p(q), self.Q, q.stride(0), _p(idx), _p(dist),
                                                    C.c_float(thr), C.c_float(ratio), int(bool(unique)), _p(self.ws),
                                                    C.c_size_t(self.ws.numel()), _p(self.table), _stream()))
        return self.table

    def match_from_table(self, q, M_total, idx, dist, thr, ratio, table):
        check(lib().pcreg_dev_match_from_table_f32(_p(q), self.Q, q.stride(0), M_total, _p(idx), _p(dist), C.c_float(thr), C.c_float(ratio),
                                                   _p(table), _p(self.ws), C.c_size_t(self.ws.numel()), _p(self.pairs), _p(self.pts1),
                                                   _p(self.pts2), _p(self.n_pairs), _stream()))
        return self.pairs, self.pts1, self.pts2, self.n_pairs


class RegistrationPipeline:
    """match (top-2 search -> threshold -> ratio -> Unique) then RANSAC, all resident in HBM."""

    def __init__(self, Q: int, M_local: int, m_lo: int = 0, M_total: int | None = None, group=None,
                 device: torch.device | None = None, replica: bool = False):
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        self.Q, self.M_local, self.m_lo = Q, M_local, m_lo
        self.M_total = M_total if M_total is not None else M_local
        self.ops = HipOps(Q, M_local, self.dev)
        self.matcher = ShardedMatcher(self.ops, Q, M_local, m_lo, self.M_total, group, replica=replica)
        self.world = self.matcher.world
        self.inliers = torch.empty(Q, dtype=torch.int32, device=self.dev)
        self.result = torch.zeros(C.sizeof(DevRansacResult), dtype=torch.uint8, device=self.dev)
        self.ws_ransac = None
        self.pairs = self.pts1 = self.pts2 = None
        self.n_pairs = self.ops.n_pairs
        self._local = None

    def search_local(self, q_soa, model_soa):
        """Top-2 of every query over THIS rank's model shard (the dominant kernel).  model_soa: the [3, M] tensor (prepared
        on first use and again whenever another tensor, or a modified one, is passed) or a PreparedModel."""
        self._local = self.ops.local_top2(q_soa, model_soa, self.m_lo)

    def match_after_search(self, q_soa, model_soa, thr_abs: float, max_ratio: float, unique: bool = True):
        self.matcher.merge_ranks(*self._local)
        self.pairs, self.pts1, self.pts2, self.n_pairs = self.matcher.finish(q_soa, model_soa, thr_abs, max_ratio, unique)
        return self.pairs, self.pts1, self.pts2, self.n_pairs

    def match(self, q_soa, model_soa, thr_abs: float, max_ratio: float, unique: bool = True):
        self.search_local(q_soa, model_soa)
        return self.match_after_search(q_soa, model_soa, thr_abs, max_ratio, unique)

    def ransac(self, coef: dict, seed: int = 0, n_dev=None, pts1=None, pts2=None, sample_idx=None):
        """Device-resident ransac on the matched pairs (or on explicit [3,cap] float64 tensors)."""
        L = lib()
        o = RansacOpts(int(coef["minPtNum"]), int(coef["iterNum"]), float(coef["thDist"]), float(coef["thInlrRatio"]),
                       int(bool(coef["REFINE"])), 0, int(seed))
        pts1 = self.pts1 if pts1 is None else pts1
        pts2 = self.pts2 if pts2 is None else pts2
        n_dev = self.n_pairs if n_dev is None else n_dev
        cap = pts1.shape[1]
        need = L.pcreg_dev_ransac_workspace(cap, o.iterNum)
        if self.ws_ransac is None or self.ws_ransac.numel() < need:
            self.ws_ransac = torch.empty(need, dtype=torch.uint8, device=self.dev)
        if self.inliers.numel() < cap:
            self.inliers = torch.empty(cap, dtype=torch.int32, device=self.dev)
        check(L.pcreg_dev_ransac(_p(pts1), _p(pts2), _p(n_dev), cap, cap, C.byref(o),
                                 _p(sample_idx) if sample_idx is not None else None, _p(self.result), _p(self.inliers),
                                 _p(self.ws_ransac), C.c_size_t(self.ws_ransac.numel()), _stream()))

    def ransac_sharded(self, coef: dict, seed: int = 0):
        """The same registration with its hypotheses split over the ranks of the group (each rank scores
        iterNum / world of them, one all_gather of the 112-byte partial results agrees the winner): identical result to
        ransac(), 1/world of its time.  Falls back to ransac() on one rank."""
        if not self.matcher.collective:
            return self.ransac(coef, seed)
        L = lib()
        o = RansacOpts(int(coef["minPtNum"]), int(coef["iterNum"]), float(coef["thDist"]), float(coef["thInlrRatio"]),
                       int(bool(coef["REFINE"])), 0, int(seed))
        cap = self.pts1.shape[1]
        begin, count = hypothesis_share(o.iterNum, self.matcher.rank, self.world)
        need = L.pcreg_dev_ransac_workspace(cap, max(count, 1))
        if self.ws_ransac is None or self.ws_ransac.numel() < need:
            self.ws_ransac = torch.empty(need, dtype=torch.uint8, device=self.dev)
        if self.inliers.numel() < cap:
            self.inliers = torch.empty(cap, dtype=torch.int32, device=self.dev)
        part = torch.zeros(14, dtype=torch.int64, device=self.dev)      # pcreg_dev_ransac_part: key | (ns, has) | T[12]
        check(L.pcreg_dev_ransac_partial(_p(self.pts1), _p(self.pts2), _p(self.n_pairs), cap, cap, C.byref(o), None,
                                         begin, count, _p(part), _p(self.ws_ransac), C.c_size_t(self.ws_ransac.numel()), _stream()))
        allp = gather_ransac_parts(part, self.matcher.group)             # the one collective: 112 bytes per rank
        check(L.pcreg_dev_ransac_finish_parts(_p(self.pts1), _p(self.pts2), _p(self.n_pairs), cap, cap, C.byref(o), _p(allp),
                                              allp.shape[0], _p(self.result), _p(self.inliers), _stream()))

    def fetch_result(self) -> dict:
        """D2H copy of the last ransac result (synchronises)."""
        import numpy as np
        r = DevRansacResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        T = np.array(r.T[:]).reshape(4, 4, order="F")
        return dict(T=T, n_inliers=r.n_inliers, numSuccess=r.num_success, maxInliers=r.max_inliers,
                    failed=bool(r.failed), n=r.n, winner=r.winner, inlierIdx=self.inliers[:r.n_inliers].cpu().numpy())


class U16Rows:
    """Descriptor rows as the kernel leaves them: uint16 counts [S, 980] in keypoint order + the ascending list of the
    surviving keypoints (pcreg_dev_spatial_histogram_descriptors_rows_u16)."""

    def __init__(self, rows: torch.Tensor, index: torch.Tensor):
        self.rows, self.index = rows, index

    def compact(self, V: int) -> torch.Tensor:
        """[V, 980] uint16: the survivors' rows in order (a copy; for inspection and tests)."""
        return self.rows.view(torch.int16)[self.index[:V].long()].view(torch.uint16)      # (torch cannot index uint16 tensors)


class DescriptorPipeline:
    """One sphere position of completeExperimentFast.m:131-213, resident in HBM:
    getSpacialHistogramDescriptors (surface + model) -> getMatches -> matched keypoints -> ransac.

    Point sets are [3, N] float64 tensors.  Descriptors stay on the device as row-major [V][980];
    the only host traffic is the keypoint counts (two int32 reads that size the match grid)."""

    ND = 980

    def __init__(self, device: torch.device | None = None):
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        self._ws = {}
        self.result = torch.zeros(C.sizeof(DevRansacResult), dtype=torch.uint8, device=self.dev)
        self.n_pairs = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def _workspace(self, key: str, nbytes: int) -> torch.Tensor:
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = self._ws[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.dev)
        return t

    def describe(self, pts: torch.Tensor, sample_pts: torch.Tensor, options: dict, compact: bool = False, single_mode: int = 0):
        """describe_async + the read of the survivor count (one host synchronisation)."""
        feat, desc, counters = self.describe_async(pts, sample_pts, options, compact, single_mode)
        V, overflow = (int(v) for v in counters.cpu())
        if overflow:
            raise ValueError(f"a support holds {overflow} points: more than an LDS-resident support may have (lower max_pts)")
        return feat, desc, V

    def describe_async(self, pts: torch.Tensor, sample_pts: torch.Tensor, options: dict, compact: bool = False, single_mode: int = 0,
                       ws_key: str = "desc"):
        """-> (feat [S,3], desc, counters): enqueued, nothing read back.  counters (device int32 [2]) = the number V of surviving
        keypoints and the overflow flag; rows < V of feat are the survivors in sample order.  ws_key: callers that keep several
        descriptor stages in flight on different streams give each its own workspace.
        compact=False: desc [S,980] float64, rows < V compact (MATLAB's shape).
        compact=True: desc is a U16Rows -- the counts as uint16 rows in KEYPOINT order, written once by the kernel, plus the
        list of the V survivors (a quarter of the bytes and no staging copy; `match` takes it as it is).
        single_mode: 0 double data; 1 / 2 `single` arithmetic for the support (include/pcreg.h), compact form only."""
        from .api import _desc_opts
        L = lib()
        o = _desc_opts(options)
        P, S = pts.shape[1], sample_pts.shape[1]
        feat = torch.empty((S, 3), dtype=torch.float64, device=self.dev)
        counters = torch.zeros(2, dtype=torch.int32, device=self.dev)
        ws = self._workspace(ws_key, L.pcreg_dev_spatial_histogram_descriptors_workspace(P, S))
        if compact:
            rows = torch.empty((S, self.ND), dtype=torch.uint16, device=self.dev)
            index = torch.empty(S, dtype=torch.int32, device=self.dev)
            check(L.pcreg_dev_spatial_histogram_descriptors_rows_u16(_p(pts), P, pts.stride(0), _p(sample_pts), S, sample_pts.stride(0), C.byref(o),
                                                                     int(single_mode), _p(feat), _p(rows), _p(index), _p(counters), _p(ws),
                                                                     C.c_size_t(ws.numel()), _stream()))
            desc = U16Rows(rows, index)
        else:
            if single_mode:
                raise ValueError("single_mode is implemented for the compact (uint16 rows) form and for the host tier")
            desc = torch.empty((S, self.ND), dtype=torch.float64, device=self.dev)
            check(L.pcreg_dev_spatial_histogram_descriptors(_p(pts), P, pts.stride(0), _p(sample_pts), S, sample_pts.stride(0), C.byref(o), _p(feat),
                                                            _p(desc), _p(counters), _p(ws), C.c_size_t(ws.numel()), _stream()))
        return feat, desc, counters

    def match(self, descS, VS: int, descM, VM: int, par: dict, pairs_out: torch.Tensor | None = None,
              n_pairs_out: torch.Tensor | None = None, ws_cap: tuple | None = None):
        """-> (pairs [VS,2] int32 1-based, n_pairs device int32).  pairs_out / n_pairs_out: write into the caller's
        buffers (the batched sweep); ws_cap = (VS, VM) sizes the workspace once for a series of calls."""
        from .api import _match_opts
        L = lib()
        o = _match_opts(par)
        pairs = pairs_out if pairs_out is not None else torch.empty((max(VS, 1), 2), dtype=torch.int32, device=self.dev)
        n_pairs = n_pairs_out if n_pairs_out is not None else self.n_pairs
        cap = ws_cap or (VS, VM)
        if isinstance(descS, U16Rows) or isinstance(descM, U16Rows):        # uint16 rows + survivor lists on both sides
            if not (isinstance(descS, U16Rows) and isinstance(descM, U16Rows)):
                raise TypeError("uint16 rows on one side only")
            D = descS.rows.shape[1]
            ws = self._workspace("match", L.pcreg_dev_get_matches_workspace(cap[0], cap[1], D))
            check(L.pcreg_dev_get_matches_rows_u16(_p(descS.rows), _p(descS.index), VS, _p(descM.rows), _p(descM.index), VM, D, C.byref(o),
                                                   _p(pairs), None, _p(n_pairs), _p(ws), C.c_size_t(ws.numel()), _stream()))
        else:
            D = descS.shape[1]
            ws = self._workspace("match", L.pcreg_dev_get_matches_workspace(cap[0], cap[1], D))
            check(L.pcreg_dev_get_matches(_p(descS), VS, D, _p(descM), VM, D, D, _l.LAYOUT_ROW_MAJOR,
                                          C.byref(o), _p(pairs), None, _p(n_pairs), _p(ws), C.c_size_t(ws.numel()),
                                          _stream()))
        return pairs, n_pairs

    def ransac(self, pairs: torch.Tensor, featS: torch.Tensor, featM: torch.Tensor, coef: dict, seed: int = 0):
        """ransac on featS(pairs(:,1),:) / featM(pairs(:,2),:); result via fetch_result()."""
        L = lib()
        cap = pairs.shape[0]
        self.pts1 = torch.empty((3, cap), dtype=torch.float64, device=self.dev)
        self.pts2 = torch.empty((3, cap), dtype=torch.float64, device=self.dev)
        check(L.pcreg_dev_gather_matched_rows(_p(pairs), _p(self.n_pairs), cap, _p(featS), _p(featM), _p(self.pts1),
                                              _p(self.pts2), _stream()))
        o = RansacOpts(int(coef["minPtNum"]), int(coef["iterNum"]), float(coef["thDist"]), float(coef["thInlrRatio"]),
                       int(bool(coef["REFINE"])), 0, int(seed))
        ws = self._workspace("ransac", L.pcreg_dev_ransac_workspace(cap, o.iterNum))
        self.inliers = torch.empty(cap, dtype=torch.int32, device=self.dev)
        check(L.pcreg_dev_ransac(_p(self.pts1), _p(self.pts2), _p(self.n_pairs), cap, cap, C.byref(o), None,
                                 _p(self.result), _p(self.inliers), _p(ws), C.c_size_t(ws.numel()), _stream()))

    fetch_result = RegistrationPipeline.fetch_result


def fgr_batched_dev(p1: torch.Tensor, p2: torch.Tensor, offsets: torch.Tensor, n_cap: int, opts: dict, T0: torch.Tensor = None,
                    tuple_idx: torch.Tensor = None, kept: bool = False, ws: torch.Tensor = None, out=None):
    """Fast global registration on device buffers (pcreg_dev_fgr_batched), enqueued on torch's current stream, nothing
    read back.  p1 / p2: [3, ld] float64 (column-major n x 3 with leading dimension ld), offsets: [B + 1] int32 on the device,
    n_cap: the largest registration (trusted for the launch only), opts: api.fgr_batched's dict; T0 [B, 16] float64, tuple_idx
    [B, n_tuples, 3] int32 and ws (uint8, at least fgr_workspace_bytes) are optional.  -> (results [B, sizeof(pcreg_fgr_result)]
    uint8, inlier_idx [ld] int32, kept [ld] uint8 or None): parse a row of results with fgr_results().  Calls that reuse their
    buffers pass out=(results, inlier_idx, kept) (kept None when not wanted)."""
    from ._lib import FgrResult
    from .api import _fgr_opts
    o = _fgr_opts(opts)
    for t in (p1, p2):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != 3 or not t.is_contiguous():
            raise TypeError("pts1 / pts2 are contiguous [3, ld] float64 tensors")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise TypeError("offsets are B + 1 int32 numbers on the device")
    dev, ld, B = p1.device, int(p1.shape[1]), offsets.numel() - 1
    if tuple_idx is not None and (tuple_idx.dtype != torch.int32 or tuple(tuple_idx.shape) != (B, o.n_tuples, 3) or not tuple_idx.is_contiguous()):
        raise TypeError("tuple_idx is a contiguous [B, n_tuples, 3] int32 tensor")
    if T0 is not None and (T0.dtype != torch.float64 or T0.numel() != 16 * B or not T0.is_contiguous()):
        raise TypeError("T0 is a contiguous float64 tensor of B x 16 numbers")
    L = lib()
    need = L.pcreg_dev_fgr_batched_workspace(int(n_cap), B, o.iterations)
    if need == 0:
        raise ValueError("fast global registration: n_cap, B or iterations out of range")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"fast global registration: the workspace is a contiguous uint8 tensor of at least {need} bytes")
    if out is not None:
        results, inliers, kept_t = out
    else:
        results = torch.zeros((B, C.sizeof(FgrResult)), dtype=torch.uint8, device=dev)
        inliers = torch.zeros(max(ld, 1), dtype=torch.int32, device=dev)
        kept_t = torch.zeros(max(ld, 1), dtype=torch.uint8, device=dev) if kept else None
    check(L.pcreg_dev_fgr_batched(_p(p1), _p(p2), ld, _p(offsets), B, int(n_cap), C.addressof(o), None if T0 is None else _p(T0),
                                  None if tuple_idx is None else _p(tuple_idx), _p(results), _p(inliers), None if kept_t is None else _p(kept_t),
                                  _p(ws), ws.numel(), _stream()))
    return results, inliers, kept_t


def fgr_results(raw) -> list:
    """the rows of fgr_batched_dev's results on the host (a numpy uint8 [B, sizeof(pcreg_fgr_result)] array) -> FgrResult structs"""
    from ._lib import FgrResult
    return [FgrResult.from_buffer_copy(bytes(r)) for r in raw]
