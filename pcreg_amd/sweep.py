"""The sphere-sweep driver of completeExperimentFast.m:46-225 and its final stage (:291, :356-394)
as a device-resident pipeline.

Everything that touches descriptors or points runs through the device tier of include/pcreg.h on resident
buffers: the model's keypoints and descriptors are uploaded once, each sphere is an index list + a row gather
on the device, `getMatches` and `ransac` consume those buffers in place.  `SphereSweep.run` is the batched form
(the reference's two parfor loops as one enqueue chain, TWO host synchronisations for the whole sweep);
`run_serial` walks the spheres one at a time like the script's inner loops and is kept as its cross-check.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as _l
from ._lib import RansacOpts, check, lib
from .api import _fgr_opts, _match_opts, _transforms16, cluster_points, dbscan_points, invertTF, score_summary
from .device import DescriptorPipeline, PreparedModel, _p, _stream


def pcUniformSamples(pts, d: float, limits=None) -> np.ndarray:
    """completeExperimentFast.m:406-414: meshgrid over the cloud's limits, y fastest, then x, then z.  `limits` = (min, max) per
    axis if the caller already has them."""
    if limits is None:
        pts = np.asarray(pts, dtype=np.float64)
        limits = (pts.min(axis=0), pts.max(axis=0))
    lo, hi = limits
    ax = [lo[k] + d * np.arange(int(np.floor((hi[k] - lo[k]) / d + 1e-12)) + 1) for k in range(3)]
    X, Y, Z = np.meshgrid(ax[0], ax[1], ax[2])
    return np.column_stack([X.ravel(order="F"), Y.ravel(order="F"), Z.ravel(order="F")])


class SphereSweep:
    """featModel [VM,3] / descModel [VM,980] / featSurface [VS,3] / descSurface [VS,980]: numpy arrays or
    row-major CUDA tensors (e.g. straight from DescriptorPipeline.describe)."""

    def __init__(self, featModel, descModel, featSurface, descSurface, device: torch.device | None = None):
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(self.dev).contiguous()
        self.featM, self.descM, self.featS, self.descS = t(featModel), t(descModel), t(featSurface), t(descSurface)
        self.VM, self.D = self.descM.shape
        self.VS = self.descS.shape[0]
        self.pipe = DescriptorPipeline(self.dev)
        L = lib()
        self._idx = torch.empty(max(self.VM, 1), dtype=torch.int32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._ws_sel = torch.empty(max(L.pcreg_dev_sphere_select_workspace(self.VM), 256), dtype=torch.uint8, device=self.dev)
        self._featM_host = None
        self._limits = None

    def set_surface(self, featSurface, descSurface) -> None:
        """The next surface against the SAME model (completeExperimentFast.m runs once per surface crop): everything run() keeps
        for the model -- its spheres, the powered rows of its descriptor set, the workspaces -- stays."""
        t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(self.dev).contiguous()
        fS, dS = t(featSurface), t(descSurface)
        if dS.shape[1] != self.D or fS.shape[0] != dS.shape[0]:
            raise ValueError("surface descriptors must have the model's length and one row per surface keypoint")
        self.featS, self.descS = fS, dS
        self.VS = dS.shape[0]

    def release(self) -> None:
        """Drop the cached workspaces (the segmented chain's ~1.4 GB, the batched ransac's, the per-stream pipelines of
        run_streams()); the next run allocates them again.  The descriptor sets stay resident."""
        self._seg_ws = None
        self._rs_ws = None
        self._agg = None
        self._agg_ws = None
        if hasattr(self, "_lanes"):
            del self._lanes
        self.pipe = DescriptorPipeline(self.dev)
        torch.cuda.empty_cache()

    # -- :49-50
    def sphere_centres(self, d_spheres: float = 5.0) -> np.ndarray:
        """The model is fixed for the life of this object (one model, many surfaces: completeExperimentFast.m's shape): the limits
        of its keypoints are taken once (numpy's column-wise min / max of 60 000 x 3 rows: ~2 ms of host time that a 19-ms sweep
        would otherwise spend with the GPU idle); the mesh itself is rebuilt per call."""
        if self._limits is None:
            if self._featM_host is None:
                self._featM_host = self.featM.cpu().numpy()
            self._limits = (self._featM_host.min(axis=0), self._featM_host.max(axis=0))
        return pcUniformSamples(None, d_spheres, self._limits)

    # -- :52-64
    def valid_spheres(self, centres: np.ndarray, R_desc: float, min_pts: int = 1400, max_pts: float = float("inf")):
        c = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64)).to(self.dev)
        counts = torch.zeros(max(len(centres), 1), dtype=torch.int32, device=self.dev)
        check(lib().pcreg_dev_sphere_counts(_p(self.featM), self.VM, _p(c), len(centres), C.c_double(R_desc), _p(counts), _stream()))
        n = counts[:len(centres)].cpu().numpy().astype(np.int64)
        return (n >= min_pts) & (n <= max_pts), n

    def _select(self, centre, R: float) -> int:
        cc = (C.c_double * 3)(*[float(v) for v in centre])
        check(lib().pcreg_dev_sphere_select(_p(self.featM), self.VM, cc, C.c_double(R), _p(self._idx), _p(self._n), _p(self._ws_sel),
                                            C.c_size_t(self._ws_sel.numel()), _stream()))
        return int(self._n.item())

    # -- :109-149, one sphere
    def match_sphere(self, centre, R_desc: float, par: dict) -> dict:
        L = lib()
        n = self._select(centre, R_desc)                                   # getDescriptorMask, :118
        rows = self._idx[:n].clone()
        descCur = torch.empty((max(n, 1), self.D), dtype=torch.float64, device=self.dev)
        featCur = torch.empty((max(n, 1), 3), dtype=torch.float64, device=self.dev)
        if n > 0:
            check(L.pcreg_dev_gather_rows_f64(_p(self.descM), self.D, _p(rows), _p(self._n), n, _p(descCur), _stream()))   # :121-125
            check(L.pcreg_dev_gather_rows_f64(_p(self.featM), 3, _p(rows), _p(self._n), n, _p(featCur), _stream()))
        pairs, n_pairs = self.pipe.match(self.descS, self.VS, descCur, n, par) if n > 0 else (torch.zeros((1, 2), dtype=torch.int32, device=self.dev), None)
        P = int(n_pairs.item()) if n_pairs is not None else 0
        return dict(rows=rows, featCur=featCur, num_desc=n, pairs=pairs, num_putative=P)

    # -- :200-224, one promising sphere
    def ransac_sphere(self, m: dict, options: dict, seed: int = 0) -> dict:
        self.pipe.n_pairs.fill_(m["num_putative"])
        self.pipe.ransac(m["pairs"], self.featS, m["featCur"], options, seed=seed)
        return self.pipe.fetch_result()

    def run_serial(self, par: dict, options: dict, R_desc: float, d_spheres: float = 5.0, min_pts: int = 1400,
                   putative_thresh: int = 170, seed: int = 0) -> dict:
        """The script's loops one sphere at a time (two host reads per sphere): kept as the plain reading of
        completeExperimentFast.m:46-224 and as the cross-check of run()."""
        centres = self.sphere_centres(d_spheres)
        valid, _ = self.valid_spheres(centres, R_desc, min_pts)
        centres = centres[valid]
        S = len(centres)
        per = [self.match_sphere(centres[i], R_desc, par) for i in range(S)]
        num_putative = np.array([m["num_putative"] for m in per], dtype=np.int64)
        num_desc = np.array([m["num_desc"] for m in per], dtype=np.int64)
        trial = np.nonzero(num_putative > putative_thresh)[0]                # :175
        sp, ss, si, sr, tf = [], [], [], [], []
        for t, i in enumerate(trial):
            r = self.ransac_sphere(per[i], options, seed=seed + t)
            sp.append(per[i]["num_putative"]); ss.append(r["numSuccess"]); si.append(r["maxInliers"])
            sr.append(100.0 * r["maxInliers"] / per[i]["num_putative"] if not r["failed"] else 0.0)
            tf.append(None if r["failed"] else r["T"])
        return dict(centres=centres, num_desc=num_desc, num_putative=num_putative,
                    matches=[m["pairs"][:m["num_putative"]].cpu().numpy().astype(np.uint32) for m in per],
                    model_rows=[m["rows"].cpu().numpy().astype(np.int64) for m in per], trial=trial,
                    statsPutative=np.array(sp, dtype=np.int64), statsSuccess=np.array(ss, dtype=np.int64),
                    statsInliers=np.array(si, dtype=np.int64), statsRatio=np.array(sr, dtype=np.float64), transforms=tf)

    def run(self, par: dict, options: dict, R_desc: float, d_spheres: float = 5.0, min_pts: int = 1400,
            putative_thresh: int = 170, seed: int = 0) -> dict:
        """completeExperimentFast.m:46-224 with every per-sphere loop as ONE launch chain over all spheres, TWO host
        synchronisations for the first sweep with a set of sphere parameters and ONE for every later one (the spheres -- centres,
        row lists, gathered keypoints -- depend on the model only and are kept).

        (sync 1) the descriptor counts of all candidate centres fix the valid spheres and every buffer size (:52-64).
        Then, with nothing read back in between: getDescriptorMask of every valid sphere as one launch writing the row
        lists and featCur back to back (:109-125, pcreg_dev_sphere_select_batched); getMatches of the surface against every
        sphere's rows as ONE segmented chain of ~18 launches (:131-149, pcreg_dev_get_matches_segmented: the powered
        columns are computed once, the appended constant and the row norms per sphere); the putative threshold as a device
        list of trial spheres (:175, pcreg_dev_sweep_plan); the matched keypoints of all trials packed back to back
        (:205-206, pcreg_dev_sweep_gather); ONE batched ransac launch over the trial capacity (:201-216,
        pcreg_dev_ransac_batched, seed + trial ordinal).  (sync 2) counts, pairs, rows and result structs come back
        together.  Same outputs as run_streams() / run_serial(); SSD (never used by the reference's drivers) takes
        run_streams()."""
        from ._lib import DevRansacResult
        if str(par.get("Metric", "SSD")).upper() != "SAD":
            return self.run_streams(par, options, R_desc, d_spheres, min_pts, putative_thresh, seed)
        L = lib()
        dev = self.dev
        i32, f64 = torch.int32, torch.float64
        VS, sp = self.VS, _stream()
        # The spheres are a property of the MODEL (its keypoints, R_desc, the spacing, min_pts): their centres, row lists and gathered
        # keypoints are made at the first sweep with these parameters and kept -- one model, many surfaces.  That first sweep has the
        # script's two host synchronisations (the counts fix every size); the later ones have ONE, at the end.
        skey = (float(R_desc), float(d_spheres), int(min_pts))
        sph = self.__dict__.setdefault("_spheres", {}).get(skey)
        if sph is None:
            centres = self.sphere_centres(d_spheres)
            valid, counts = self.valid_spheres(centres, R_desc, min_pts)                     # ---- sync 1 (first sweep only)
            centres = centres[valid]
            num_desc = counts[valid].astype(np.int64)
            S = len(centres)
            sph = dict(centres=centres, num_desc=num_desc, S=S)
            if S:
                row_off = np.zeros(S + 1, dtype=np.int64); row_off[1:] = np.cumsum(num_desc)
                tot, n_max = int(row_off[-1]), int(num_desc.max())
                if tot >= 2**31:
                    raise ValueError("sphere sweep: more than 2^31 rows over all spheres")
                seg_off = torch.from_numpy(row_off.astype(np.int32)).to(dev)
                cen = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64)).to(dev)
                roff_dev = torch.from_numpy(row_off[:S].copy()).to(dev)
                rows_all = torch.empty(tot, dtype=i32, device=dev)
                feat_all = torch.empty((tot, 3), dtype=f64, device=dev)
                n_sel = torch.zeros(S, dtype=i32, device=dev)
                check(L.pcreg_dev_sphere_select_batched(_p(self.featM), self.VM, _p(cen), S, C.c_double(R_desc), _p(seg_off), _p(rows_all), _p(feat_all),
                                                        _p(n_sel), sp))                                                     # :109-125
                assert np.array_equal(n_sel.cpu().numpy(), num_desc), "sphere_select disagrees with sphere_counts"
                rows_host = rows_all.cpu().numpy().astype(np.int64)
                # model rows that lie in NO sphere never meet the surface: the matcher gets the model set restricted to the union of the
                # spheres' rows (the lists renumbered into it; a pair's model index counts inside its sphere, so nothing else changes)
                union = np.unique(rows_host)
                if len(union) < 0.95 * self.VM:
                    desc_u = self.descM[torch.from_numpy(union).to(dev)].contiguous()
                    rows_u = torch.from_numpy(np.searchsorted(union, rows_host).astype(np.int32)).to(dev)
                else:
                    desc_u, rows_u = self.descM, rows_all
                sph.update(row_off=row_off, tot=tot, n_max=n_max, seg_off=seg_off, roff_dev=roff_dev, rows_all=rows_all, feat_all=feat_all,
                           model_rows=[rows_host[row_off[i]:row_off[i + 1]] for i in range(S)], desc_u=desc_u, rows_u=rows_u, n_union=int(len(union)))
            # an entry holds the restricted model set (hundreds of MB at the reference's shape): keep the two most recent parameter sets
            while len(self._spheres) >= 2:
                self._spheres.pop(next(iter(self._spheres)))
            self._spheres[skey] = sph
        centres, num_desc, S = sph["centres"], sph["num_desc"], sph["S"]
        if S == 0:
            self._agg = None
            return dict(centres=centres, num_desc=num_desc, num_putative=np.zeros(0, np.int64), matches=[], model_rows=[], trial=np.zeros(0, np.int64),
                        statsPutative=np.zeros(0, np.int64), statsSuccess=np.zeros(0, np.int64), statsInliers=np.zeros(0, np.int64),
                        statsRatio=np.zeros(0), transforms=[])
        row_off, tot, n_max, seg_off, roff_dev, rows_all, feat_all = (sph[k] for k in ("row_off", "tot", "n_max", "seg_off", "roff_dev", "rows_all", "feat_all"))
        pairs_all = torch.zeros((S, max(VS, 1), 2), dtype=i32, device=dev)
        n_pairs = torch.zeros(S, dtype=i32, device=dev)
        o = _match_opts(par)
        wsb = L.pcreg_dev_get_matches_segmented_workspace(VS, sph["desc_u"].shape[0], self.D, S, tot, n_max)
        if getattr(self, "_seg_ws", None) is None or self._seg_ws.numel() < wsb:
            self._seg_ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        # the model is fixed for the life of this object (one model, many surfaces): its powered rows and row scalars -- what the
        # segmented matcher makes of the model set alone -- are prepared once per set of options, not once per sweep
        desc_u, rows_u = sph["desc_u"], sph["rows_u"]
        VMu = desc_u.shape[0]
        key = (skey, int(o.change_metric), float(o.metric_factor) if o.change_metric else 0.0)
        if getattr(self, "_seg_prep_key", None) != key:
            nb = L.pcreg_dev_segmented_model_bytes(VMu, self.D)
            if getattr(self, "_seg_prep", None) is None or self._seg_prep.numel() < nb:
                self._seg_prep = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
            check(L.pcreg_dev_segmented_model_prepare(_p(desc_u), VMu, self.D, C.byref(o), _p(self._seg_prep), C.c_size_t(self._seg_prep.numel()), sp))
            self._seg_prep_key = key
        check(L.pcreg_dev_get_matches_segmented_prepared(_p(self.descS), VS, _p(desc_u), VMu, self.D, _p(self._seg_prep), key[1], C.c_double(o.metric_factor),
                                                         _p(rows_u), _p(seg_off), S, tot, n_max, C.byref(o), _p(pairs_all), None, _p(n_pairs), _p(self._seg_ws),
                                                         C.c_size_t(self._seg_ws.numel()), sp))                                  # :131-149
        return self._finish_sweep(centres, num_desc, row_off, rows_all, feat_all, None, pairs_all, n_pairs, options, putative_thresh, seed, roff_dev,
                                  model_rows=sph["model_rows"])

    def _pinned(self, key: str, n: int, dtype) -> "torch.Tensor":
        """A page-locked host buffer of at least n elements, kept across sweeps (the first n elements are returned)."""
        cache = self.__dict__.setdefault("_pin", {})
        t = cache.get(key)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
            cache[key] = t
        return t[:n]

    def _finish_sweep(self, centres, num_desc, row_off, rows_all, feat_all, n_sel, pairs_all, n_pairs, options, putative_thresh, seed, roff_dev=None,
                      model_rows=None) -> dict:
        """:166-224 on the current stream + the sweep's second (last) host synchronisation."""
        from ._lib import DevRansacResult
        L = lib()
        dev = self.dev
        S = len(centres)
        i32, f64 = torch.int32, torch.float64
        sp = _stream()
        trial_idx = torch.empty(S, dtype=i32, device=dev); offsets = torch.empty(S + 1, dtype=i32, device=dev)
        n_trials = torch.zeros(1, dtype=i32, device=dev)
        check(L.pcreg_dev_sweep_plan(_p(n_pairs), S, int(putative_thresh), _p(trial_idx), _p(offsets), _p(n_trials), sp))
        ld = S * max(self.VS, 1)                                    # capacity of the packed correspondences (Unique: <= VS pairs per sphere)
        p1 = torch.zeros((3, ld), dtype=f64, device=dev); p2 = torch.zeros((3, ld), dtype=f64, device=dev)
        if roff_dev is None:
            roff_dev = torch.from_numpy(row_off[:S].copy()).to(dev)
        check(L.pcreg_dev_sweep_gather(_p(pairs_all), self.VS, _p(n_pairs), _p(trial_idx), _p(offsets), _p(n_trials), S, _p(self.featS),
                                       _p(feat_all), _p(roff_dev), _p(p1), _p(p2), ld, sp))
        o = RansacOpts(int(options["minPtNum"]), int(options["iterNum"]), float(options["thDist"]), float(options["thInlrRatio"]),
                       int(bool(options["REFINE"])), 0, int(seed))
        rs = C.sizeof(DevRansacResult)
        results = torch.zeros((S, rs), dtype=torch.uint8, device=dev)
        inliers = torch.empty(ld, dtype=i32, device=dev)
        wsb = L.pcreg_dev_ransac_batched_workspace(self.VS, o.iterNum, S)
        if getattr(self, "_rs_ws", None) is None or self._rs_ws.numel() < wsb:
            self._rs_ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        check(L.pcreg_dev_ransac_batched(_p(p1), _p(p2), ld, _p(offsets), S, self.VS, C.byref(o), _p(results), _p(inliers), _p(self._rs_ws),
                                         C.c_size_t(self._rs_ws.numel()), sp))
        # ---- sync 2: everything comes back together -- the small results in ONE pinned transfer (seven separate .cpu() calls were
        # seven synchronisations, ~0.4 ms of the sweep), then the pair and row lists, which need the pair counts for their size
        check_sel = n_sel is not None
        if not check_sel:                                            # run(): the row lists were checked and fetched when the spheres were made
            n_sel = torch.zeros(S, dtype=i32, device=dev)            # (keeps the layout of the packed transfer below)
        small = torch.cat([n_pairs, n_trials, trial_idx, n_sel, results.view(torch.int32).view(-1)])
        hs = self._pinned("small", small.numel(), torch.int32)
        hs.copy_(small, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h = hs.numpy()
        npr = h[:S].astype(np.int64)
        nt = int(h[S])
        trial = h[S + 1:S + 1 + nt].astype(np.int64)
        nsel = h[2 * S + 1:3 * S + 1].copy()
        raw = h[3 * S + 1:].view(np.uint8).reshape(S, rs)[:max(nt, 1)].copy()
        m_pairs = max(int(npr.max()) if S else 0, 1)                # only the columns that hold pairs cross the bus
        hp = self._pinned("pairs", S * m_pairs * 2, torch.int32).view(S, m_pairs, 2)
        hp.copy_(pairs_all[:, :m_pairs], non_blocking=True)
        if model_rows is None:
            hr = self._pinned("rows", max(rows_all.numel(), 1), torch.int32)[:rows_all.numel()]
            hr.copy_(rows_all, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        pairs_host = hp.numpy().astype(np.uint32)                   # one conversion (a copy: the pinned buffer is reused); the per-sphere lists are views of it
        if model_rows is None:
            rows_host = hr.numpy().astype(np.int64)
            model_rows = [rows_host[row_off[i]:row_off[i + 1]] for i in range(S)]
        assert not check_sel or np.array_equal(nsel, num_desc), "sphere_select disagrees with sphere_counts"
        sp_, ss, si, sr, tf = [], [], [], [], []
        for t in range(nt):
            r = DevRansacResult.from_buffer_copy(raw[t].tobytes())
            P = int(npr[trial[t]])
            sp_.append(P); ss.append(r.num_success); si.append(r.max_inliers)
            sr.append(100.0 * r.max_inliers / P if not r.failed else 0.0)
            tf.append(None if r.failed else np.array(r.T[:]).reshape(4, 4, order="F"))
        out = dict(centres=centres, num_desc=num_desc, num_putative=npr,
                   matches=[pairs_host[i, :npr[i]] for i in range(S)],
                   model_rows=model_rows, trial=trial,
                   statsPutative=np.array(sp_, dtype=np.int64), statsSuccess=np.array(ss, dtype=np.int64),
                   statsInliers=np.array(si, dtype=np.int64), statsRatio=np.array(sr, dtype=np.float64), transforms=tf)
        # what aggregate() stacks from: this sweep's resident pairs, their counts, the spheres' keypoints and row offsets, the surface
        # they were matched against -- private references, dropped by release() and replaced by the next sweep
        self._agg = dict(result=out, pairs_all=pairs_all, n_pairs=n_pairs, feat_all=feat_all, roff_dev=roff_dev, featS=self.featS, VS=self.VS)
        return out

    def aggregate(self, result: dict, members, options: dict, seed: int = 0) -> dict:
        """completeExperiment.m:424-458 on the buffers the last run() / run_streams() left on the device: stack the putative matches
        of the spheres `members` (indices into result["centres"], e.g. largest_cluster(result)[1]) in that order, pairs in each
        sphere's own order (:424-437, pcreg_dev_sweep_gather with the members as its list); make them unique twice (:439-443,
        pcreg_dev_aggregate_matches); ONE ransac on what is left with `options` and `seed` (:446-455, the built-in sampler);
        T_final = estimateTransform over its inliers (:458, pcreg_dev_estimate_transform_indexed).  ONE host synchronisation: the
        final read.  `result` must be the dict that sweep returned.  -> dict(n_total, n_unique1, n_unique2, T, inlierIdx (1-based
        rows of the aggregated pairs), numSuccess, maxInliers, maxInlierRatio (percent), T_final, host_syncs); T and T_final are None
        where ransac fails (the script stops there)."""
        from ._lib import DevRansacResult
        st = getattr(self, "_agg", None)
        if st is None or result is not st["result"]:
            raise ValueError("aggregate: `result` is not the result of this object's last run() / run_streams() (or release() dropped its buffers)")
        L = lib()
        dev, sp = self.dev, _stream()
        i32, f64 = torch.int32, torch.float64
        members = np.asarray(members, dtype=np.int64).reshape(-1)
        S = len(result["centres"])
        if len(members) and (members.min() < 0 or members.max() >= S):
            raise ValueError("aggregate: a member is not a sphere of this sweep")
        K = len(members)
        offs = np.zeros(K + 1, dtype=np.int64); offs[1:] = np.cumsum(np.asarray(result["num_putative"], dtype=np.int64)[members])
        total = int(offs[-1])
        if total >= 2**31 - 4096:
            raise ValueError("aggregate: more than 2^31 stacked matches")
        if total == 0:
            return dict(n_total=0, n_unique1=0, n_unique2=0, T=None, inlierIdx=np.zeros(0, np.int64), numSuccess=0, maxInliers=0,
                        maxInlierRatio=0.0, T_final=None, host_syncs=0)
        VS = st["VS"]
        # the member list, its offsets, the list's length and the stacked total: one upload
        ints = torch.from_numpy(np.concatenate([members, offs, [K, total]]).astype(np.int32)).to(dev)
        m_dev, o_dev, k_dev, n_dev = ints[:K], ints[K:2 * K + 1], ints[2 * K + 1:2 * K + 2], ints[2 * K + 2:]
        p1 = torch.empty((3, total), dtype=f64, device=dev); p2 = torch.empty((3, total), dtype=f64, device=dev)
        check(L.pcreg_dev_sweep_gather(_p(st["pairs_all"]), max(VS, 1), _p(st["n_pairs"]), _p(m_dev), _p(o_dev), _p(k_dev), K, _p(st["featS"]),
                                       _p(st["feat_all"]), _p(st["roff_dev"]), _p(p1), _p(p2), total, sp))           # :424-437
        u1 = torch.empty((3, total), dtype=f64, device=dev); u2 = torch.empty((3, total), dtype=f64, device=dev)
        n_out = torch.zeros(1, dtype=i32, device=dev)
        wsb = L.pcreg_dev_aggregate_matches_workspace(total)
        rcap = min(total, max(VS, 1))                              # a surface keypoint survives the first unique once: <= VS pairs reach ransac
        o = RansacOpts(int(options["minPtNum"]), int(options["iterNum"]), float(options["thDist"]), float(options["thInlrRatio"]),
                       int(bool(options["REFINE"])), 0, int(seed))
        wsr = L.pcreg_dev_ransac_workspace(rcap, o.iterNum)
        if getattr(self, "_agg_ws", None) is None or self._agg_ws[0].numel() < wsb or self._agg_ws[1].numel() < wsr:
            self._agg_ws = (torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev), torch.empty(max(wsr, 256), dtype=torch.uint8, device=dev))
        ws_a, ws_r = self._agg_ws
        check(L.pcreg_dev_aggregate_matches(_p(p1), _p(p2), _p(n_dev), total, total, _p(u1), _p(u2), total, 1, None, _p(n_out), _p(ws_a),
                                            C.c_size_t(ws_a.numel()), sp))                                           # :439-443
        n1_off = 2 * ((4 * total + 255) // 256 * 256)              # the first unique's count, where include/pcreg.h says the chain leaves it
        n1 = ws_a[n1_off:n1_off + 4].view(i32)
        rs = C.sizeof(DevRansacResult)
        res = torch.zeros(rs // 4, dtype=i32, device=dev)
        inl = torch.zeros(rcap, dtype=i32, device=dev)
        check(L.pcreg_dev_ransac(_p(u1), _p(u2), _p(n_out), rcap, total, C.byref(o), None, _p(res), _p(inl), _p(ws_r), C.c_size_t(ws_r.numel()),
                                 sp))                                                                                # :446-455
        T16 = torch.zeros(16, dtype=f64, device=dev)
        info = torch.zeros(2, dtype=i32, device=dev)
        check(L.pcreg_dev_estimate_transform_indexed(_p(u1), _p(u2), total, _p(inl), 1, _p(res[32:33]), rcap, _p(T16), _p(info), sp))   # :458
        h = torch.cat([n1, n_out, res, info, T16.view(i32), inl]).cpu().numpy()                                       # ---- the one sync
        nu1, nu2 = int(h[0]), int(h[1])
        r = DevRansacResult.from_buffer_copy(h[2:2 + rs // 4].tobytes())
        empty_final = int(h[3 + rs // 4])
        Tf = h[4 + rs // 4:36 + rs // 4].copy().view(np.float64).reshape(4, 4, order="F")
        inliers = h[36 + rs // 4:36 + rs // 4 + r.n_inliers].astype(np.int64)
        failed = bool(r.failed)
        return dict(n_total=total, n_unique1=nu1, n_unique2=nu2, T=None if failed else np.array(r.T[:]).reshape(4, 4, order="F"),
                    inlierIdx=np.zeros(0, np.int64) if failed else inliers, numSuccess=r.num_success, maxInliers=r.max_inliers,
                    maxInlierRatio=0.0 if failed or nu2 == 0 else 100.0 * r.max_inliers / nu2,
                    T_final=None if failed or empty_final else Tf, host_syncs=1)

    def fgr_trials(self, result: dict, opts: dict) -> dict:
        """Fast global registration (pcreg_dev_fgr_batched) of every trial of the last sweep in ransac's place: the
        trial list of `result` gathered again from the buffers the sweep left on the device (pcreg_dev_sweep_gather, the same
        packing as the sweep's own), ONE device call over the trials, ONE host synchronisation: the final read.  opts:
        api.fgr_batched's dict (delta2 is compared with squared distances, as thDist is).  `result` must be the dict that sweep
        returned.  -> dict(trial, statsPutative, statsInliers (kept pairs within delta2 of the final T), statsRatio (percent),
        transforms (None where failed), inlierIdx (1-based rows of each trial's pairs), n_kept, cost, host_syncs)."""
        from .device import fgr_batched_dev, fgr_results
        st = getattr(self, "_agg", None)
        if st is None or result is not st["result"]:
            raise ValueError("fgr_trials: `result` is not the result of this object's last run() / run_streams() (or release() dropped its buffers)")
        L = lib()
        dev, sp = self.dev, _stream()
        trial = np.asarray(result["trial"], dtype=np.int64)
        nt, VS = len(trial), max(st["VS"], 1)
        empty = dict(trial=trial, statsPutative=np.zeros(0, np.int64), statsInliers=np.zeros(0, np.int64), statsRatio=np.zeros(0), transforms=[],
                     inlierIdx=[], n_kept=np.zeros(0, np.int64), cost=np.zeros(0), host_syncs=0)
        if nt == 0:
            return empty
        sizes = np.asarray(result["num_putative"], dtype=np.int64)[trial]
        offs = np.zeros(nt + 1, dtype=np.int64); offs[1:] = np.cumsum(sizes)
        total = int(offs[-1])
        # the trial list, its offsets and its length: one upload (aggregate() hands its members to the gather the same way)
        ints = torch.from_numpy(np.concatenate([trial, offs, [nt]]).astype(np.int32)).to(dev)
        t_dev, o_dev, k_dev = ints[:nt], ints[nt:2 * nt + 1], ints[2 * nt + 1:]
        ld = max(total, 1)
        p1 = torch.zeros((3, ld), dtype=torch.float64, device=dev); p2 = torch.zeros((3, ld), dtype=torch.float64, device=dev)
        check(L.pcreg_dev_sweep_gather(_p(st["pairs_all"]), VS, _p(st["n_pairs"]), _p(t_dev), _p(o_dev), _p(k_dev), nt, _p(st["featS"]),
                                       _p(st["feat_all"]), _p(st["roff_dev"]), _p(p1), _p(p2), ld, sp))
        n_cap = int(sizes.max())
        need = L.pcreg_dev_fgr_batched_workspace(n_cap, nt, _fgr_opts(opts).iterations)
        if getattr(self, "_fgr_ws", None) is None or self._fgr_ws.numel() < need:
            self._fgr_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        res, inl, _k = fgr_batched_dev(p1, p2, o_dev, n_cap, opts, ws=self._fgr_ws)
        h = torch.cat([res.view(torch.int32).view(-1), inl]).cpu().numpy()                                            # ---- the one sync
        nres = res.numel() // 4
        rs = fgr_results(h[:nres].view(np.uint8).reshape(nt, -1))
        inliers = h[nres:]
        return dict(trial=trial, statsPutative=sizes.copy(), statsInliers=np.array([r.n_inliers for r in rs], dtype=np.int64),
                    statsRatio=np.array([100.0 * r.n_inliers / max(int(n), 1) for r, n in zip(rs, sizes)]),
                    transforms=[None if r.failed else np.array(r.T[:]).reshape(4, 4, order="F") for r in rs],
                    inlierIdx=[inliers[offs[t]:offs[t] + rs[t].n_inliers].astype(np.int64) for t in range(nt)],
                    n_kept=np.array([r.n_kept for r in rs], dtype=np.int64), cost=np.array([r.cost for r in rs]), host_syncs=1)

    def run_streams(self, par: dict, options: dict, R_desc: float, d_spheres: float = 5.0, min_pts: int = 1400,
                    putative_thresh: int = 170, seed: int = 0, n_streams: int = 8) -> dict:
        """Round 2's batched form, kept as the cross-check of run() and for SSD: one getMatches CHAIN per sphere,
        round-robin on `n_streams` HIP streams, then the same plan / gather / batched ransac.

        The reference runs the per-sphere getMatches under parfor (:131-149) and the per-trial ransac under a second
        parfor (:201-216).  Here: (sync 1) the descriptor counts of all candidate centres, which fix the valid spheres
        and every buffer size (:52-64); then, with nothing read back in between, for every valid sphere -- round-robin on
        `n_streams` HIP streams so that the latency-sized kernels of different spheres overlap -- getDescriptorMask as an
        index list, the row gathers and getMatches (:109-149); then on the main stream the putative threshold as a device
        list of trial spheres (:175, pcreg_dev_sweep_plan), the matched keypoints of all trials packed back to back
        (:205-206, pcreg_dev_sweep_gather) and ONE batched ransac launch over the trial capacity
        (pcreg_dev_ransac_batched, seed + trial ordinal); (sync 2) counts, pairs, rows and the result structs come back
        together.  Same outputs as run_serial()."""
        from ._lib import DevRansacResult
        L = lib()
        dev = self.dev
        centres = self.sphere_centres(d_spheres)
        valid, counts = self.valid_spheres(centres, R_desc, min_pts)                     # ---- sync 1
        centres = centres[valid]
        num_desc = counts[valid].astype(np.int64)
        S = len(centres)
        empty = dict(centres=centres, num_desc=num_desc, num_putative=np.zeros(0, np.int64), matches=[], model_rows=[], trial=np.zeros(0, np.int64),
                     statsPutative=np.zeros(0, np.int64), statsSuccess=np.zeros(0, np.int64), statsInliers=np.zeros(0, np.int64),
                     statsRatio=np.zeros(0), transforms=[])
        if S == 0:
            self._agg = None
            return empty
        i32, f64 = torch.int32, torch.float64
        row_off = np.zeros(S + 1, dtype=np.int64); row_off[1:] = np.cumsum(num_desc)
        tot = int(row_off[-1]); n_max = int(num_desc.max())
        rows_all = torch.empty(tot, dtype=i32, device=dev)
        feat_all = torch.empty((tot, 3), dtype=f64, device=dev)
        desc_all = torch.empty((tot, self.D), dtype=f64, device=dev)
        n_sel = torch.zeros(S, dtype=i32, device=dev)
        pairs_all = torch.zeros((S, max(self.VS, 1), 2), dtype=i32, device=dev)
        n_pairs = torch.zeros(S, dtype=i32, device=dev)
        ns = max(1, min(n_streams, S))
        if not hasattr(self, "_lanes") or len(self._lanes) < ns:
            self._lanes = [(torch.cuda.Stream(device=dev), DescriptorPipeline(dev),
                            torch.empty(max(L.pcreg_dev_sphere_select_workspace(self.VM), 256), dtype=torch.uint8, device=dev)) for _ in range(ns)]
        cur = torch.cuda.current_stream(dev)
        for st, _, _ in self._lanes[:ns]:
            st.wait_stream(cur)
        for i in range(S):
            st, pipe, ws_sel = self._lanes[i % ns]
            lo, n = int(row_off[i]), int(num_desc[i])
            cc = (C.c_double * 3)(*[float(v) for v in centres[i]])
            with torch.cuda.stream(st):
                sp = C.c_void_p(st.cuda_stream)
                rows = rows_all[lo:lo + n]
                check(L.pcreg_dev_sphere_select(_p(self.featM), self.VM, cc, C.c_double(R_desc), _p(rows), _p(n_sel[i:i + 1]), _p(ws_sel),
                                                C.c_size_t(ws_sel.numel()), sp))                                         # getDescriptorMask, :118
                check(L.pcreg_dev_gather_rows_f64(_p(self.descM), self.D, _p(rows), _p(n_sel[i:i + 1]), n, _p(desc_all[lo:lo + n]), sp))   # :121-125
                check(L.pcreg_dev_gather_rows_f64(_p(self.featM), 3, _p(rows), _p(n_sel[i:i + 1]), n, _p(feat_all[lo:lo + n]), sp))
                pipe.match(self.descS, self.VS, desc_all[lo:lo + n], n, par, pairs_out=pairs_all[i], n_pairs_out=n_pairs[i:i + 1],
                           ws_cap=(self.VS, n_max))                                                                       # getMatches, :141
        for st, _, _ in self._lanes[:ns]:
            cur.wait_stream(st)
        return self._finish_sweep(centres, num_desc, row_off, rows_all, feat_all, n_sel, pairs_all, n_pairs, options, putative_thresh, seed)


def _good_trials(result: dict, thSucc: float, thInliers: float, thRatio: float, thPutative: float):
    """:238-239: (the trials' sphere centres, their transforms, the ordinals of the trials that reach the four thresholds and have a
    transform)"""
    centres = np.asarray(result["centres"], dtype=np.float64).reshape(-1, 3)[np.asarray(result["trial"], dtype=np.int64)]
    tf = result["transforms"]
    mask = ((np.asarray(result["statsSuccess"]) >= thSucc) & (np.asarray(result["statsInliers"]) >= thInliers) &
            (np.asarray(result["statsRatio"]) >= thRatio) & (np.asarray(result["statsPutative"]) >= thPutative) &
            np.array([t is not None for t in tf], dtype=bool))
    return centres, tf, np.nonzero(mask)[0]                                                 # :239


def _cluster_centres(loc, r: float, min_spheres):
    """(cl_off, members) of the promising spheres' centres: cluster_points with the radius squared once in single, or, with
    min_spheres an integer, dbscan_points(loc, r2, min_spheres), whose noise spheres are in no cluster."""
    r32 = np.float32(r)
    if min_spheres is None:
        _, cl_off, members = cluster_points(loc, r32 * r32)                                 # :267
    else:
        _, _, cl_off, members = dbscan_points(loc, r32 * r32, min_spheres)
    return cl_off, members


def promising_clusters(result: dict, thSucc: float = 0, thInliers: float = 28, thRatio: float = 10, thPutative: float = 170,
                       r: float | None = None, d_spheres: float = 5.0, min_spheres: int | None = None) -> list:
    """completeExperimentFast.m:238-248 and :266-288, the link from a sweep's result to FinalStage.run: keep the trials whose
    statsSuccess / statsInliers / statsRatio (percent) / statsPutative reach the four thresholds, cluster their sphere centres
    with radius r (default 1.6 * d_spheres, :266) in ONE cluster_points call, and for every cluster return (locCur, transCur):
    locCur the mean of the cluster's centres in double, transCur the transform of the centre nearest to that mean (the first
    one on a tie, as MATLAB's min).  -> [(locCur [3], transCur [4, 4])] in the clusters' order, [] without a good sphere.  A trial
    whose RANSAC failed has no transform and is never kept.  min_spheres (an integer >= 1, default None: every sphere is in a
    cluster) asks for DBSCAN's density rule: a centre is a core centre only with at least min_spheres centres, itself included,
    within r, and a sphere that is neither core nor within r of a core centre is noise and belongs to no cluster."""
    centres, tf, good = _good_trials(result, thSucc, thInliers, thRatio, thPutative)
    if len(good) == 0:
        return []
    loc = centres[good]                                                                     # :247
    r = 1.6 * float(d_spheres) if r is None else float(r)                                   # :266
    cl_off, members = _cluster_centres(loc, r, min_spheres)
    out = []
    for c in range(len(cl_off) - 1):
        rows = members[cl_off[c]:cl_off[c + 1]]
        cur = loc[rows]
        loc_cur = cur.mean(axis=0)                                                          # :283
        nearest = int(np.argmin(np.sqrt(((cur - loc_cur) ** 2).sum(axis=1))))               # :286-287, the first minimum
        out.append((loc_cur, np.asarray(tf[good[rows[nearest]]], dtype=np.float64)))        # :288
    return out


def largest_cluster(result: dict, thSucc: float = 0, thInliers: float = 28, thRatio: float = 10, thPutative: float = 170,
                    r: float | None = None, d_spheres: float = 5.0, min_spheres: int | None = None):
    """completeExperiment.m:379-389: the LARGEST cluster of promising spheres -- promising_clusters' thresholds and clustering (ONE
    cluster_points call, radius r, default 1.6 * d_spheres); `[~, idx] = max(cluster_size)` takes the first largest, which is the
    one with the smallest first row.  -> (trials, spheres): the members' trial ordinals (indices into result["trial"] / the stats)
    and sphere indices (into result["centres"]), int64, in ascending row order; two empty arrays without a good sphere.  A trial
    whose RANSAC failed is never a member.  `spheres` is what SphereSweep.aggregate takes.  min_spheres: promising_clusters';
    two empty arrays when every good sphere is noise."""
    centres, _, good = _good_trials(result, thSucc, thInliers, thRatio, thPutative)
    if len(good) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    r = 1.6 * float(d_spheres) if r is None else float(r)
    cl_off, members = _cluster_centres(centres[good], r, min_spheres)
    sizes = np.diff(np.asarray(cl_off, dtype=np.int64))
    if len(sizes) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = int(np.argmax(sizes))                                                               # the first maximum, as MATLAB's max
    rows = np.sort(np.asarray(members[cl_off[c]:cl_off[c + 1]], dtype=np.int64))
    trials = good[rows].astype(np.int64)
    return trials, np.asarray(result["trial"], dtype=np.int64)[trials]


def score_trials(result: dict, model: PreparedModel, surface_soa: torch.Tensor, max_dist: float, keep_ratio=None) -> dict:
    """Every trial of a sweep's result scored on the dense clouds (PreparedModel.score_transforms): put the surface ([3, Q]
    float32) on the prepared dense model with invertTF(transforms[t]) -- ransac's transforms map model onto surface -- and count
    the surface points with a model point within max_dist.  A failed trial (None) is the empty transform and scores nothing.
    -> dict(n_close [n] int32, sum_d2 [n] float64, fitness = n_close / Q, rmse = sqrt(sum_d2 / n_close), NaN where nothing is
    close), aligned with result["trial"].  One upload (the [n][16] block) and one read (12 bytes per trial); the radius is
    squared once in single, and the comparison is the point search's: fp32, inclusive.  keep_ratio (None: as above): a number in
    (0, 1] scores each trial on the closest keep_ratio share of its pairs within max_dist (PreparedModel.score_transforms'
    keep_ratio), and the dict gains n_within [n] int32 and d2_cut [n] float32; one read of 20 bytes per trial."""
    tf = [None if T is None else invertTF(np.asarray(T, dtype=np.float64)) for T in result["transforms"]]
    Q, n = int(surface_soa.shape[1]), len(tf)
    if n == 0:
        res = score_summary(np.zeros(0, np.int32), np.zeros(0), Q)
        if keep_ratio is not None:
            res.update(n_within=np.zeros(0, np.int32), d2_cut=np.zeros(0, np.float32))
        return res
    T_dev = torch.from_numpy(_transforms16(tf)).to(surface_soa.device)
    r2 = float(np.float32(max_dist) * np.float32(max_dist))
    if keep_ratio is not None:
        n_close, sum_d2, n_within, d2_cut = model.score_transforms(surface_soa, T_dev, r2, keep_ratio=keep_ratio)
        both = torch.cat([sum_d2.view(torch.int32), n_close, n_within, d2_cut.view(torch.int32)]).cpu().numpy()
        res = score_summary(both[2 * n:3 * n], both[:2 * n].view(np.float64), Q)
        res.update(n_within=both[3 * n:4 * n].copy(), d2_cut=both[4 * n:].view(np.float32).copy())
        return res
    n_close, sum_d2 = model.score_transforms(surface_soa, T_dev, r2)
    both = torch.cat([sum_d2.view(torch.int32), n_close]).cpu().numpy()
    return score_summary(both[2 * n:], both[:2 * n].view(np.float64), Q)


def refine_trials(result: dict, model: PreparedModel, surface_soa: torch.Tensor, max_dist: float, steps: int = 1, normals=None, ndt=None,
                  neighbors: int = 1, outlier_ratio: float = 0.55, surface_normals=None, epsilon: float = 1e-3, cpd=None, keep_ratio=None):
    """Every trial of a sweep's result refitted on the dense clouds (PreparedModel.refit_transforms): completeExperimentFast.m:383-394's
    T_refine with the dense surface ([3, Q] float32) and the prepared dense model in the place of a cluster's re-matched
    keypoints, `steps` times over.  The orientation is score_trials': invertTF(transforms[t]) puts the surface on the model and
    is what gets refitted, and invertTF of the result comes back, so a refined transform maps the model onto the surface as
    ransac's do.  -> (transforms, summary): a list aligned with result["trial"], None for a failed trial and for one whose
    refit is empty; score_trials' dict for the pairs of the last step (the transform that went into it).  One upload and one
    read, whatever `steps`; the radius is squared once in single.  normals (the [3, M] tensor PreparedModel.normals returns): the
    steps are point-to-plane steps (PreparedModel.refit_plane) instead of estimateTransform steps -- the same orientation, the same
    outputs, a trial whose planes give no fit None.  normals and surface_normals (the [3, Q] tensor PreparedModel.normals returns for a
    model made of the surface): the steps are plane-to-plane steps (PreparedModel.refit_gicp with `epsilon`) instead.  ndt (a device.NdtModel of the dense model): the steps are NDT steps
    (NdtModel.refit with `neighbors` and `outlier_ratio`) instead -- no nearest-row search, so model and max_dist are not used and
    may be None; the same orientation; the summary is then dict(n_pairs, sum_e) of the last step, a trial without a fit None.
    cpd (a dict(sigma2=, outlier=), either key optional: PreparedModel.refit_cpd's defaults): the steps are coherent-point-drift
    steps instead -- every surface point softly against every model row, so max_dist is not used and may be None; the same
    orientation; the summary is then dict(sigma2, Np, sum_res2, sum_d2, n_live) of the last step, a trial without a fit None.
    keep_ratio (None: as above; not with ndt or cpd, which pair no nearest rows): a number in (0, 1] makes every estimateTransform,
    point-to-plane or plane-to-plane step keep the closest keep_ratio share of its pairs within max_dist; the
    summary is then about the kept pairs and gains n_within [n] int32 and d2_cut [n] float32 of the last step."""
    if keep_ratio is not None and (ndt is not None or cpd is not None):
        raise ValueError("keep_ratio trims nearest-row pairs: the NDT and coherent-point-drift steps have none")
    tf = [None if T is None else invertTF(np.asarray(T, dtype=np.float64)) for T in result["transforms"]]
    Q, n = int(surface_soa.shape[1]), len(tf)
    if n == 0:
        return [], score_summary(np.zeros(0, np.int32), np.zeros(0), Q)
    T_dev = torch.from_numpy(_transforms16(tf)).to(surface_soa.device)
    if ndt is not None:
        T_out, _step, n_pairs, sum_e, empty = ndt.refit(surface_soa, T_dev, neighbors=neighbors, outlier_ratio=outlier_ratio, steps=steps)
        both = torch.cat([T_out.reshape(-1).view(torch.int32), sum_e.view(torch.int32), n_pairs, empty]).cpu().numpy()
        mats = both[:32 * n].view(np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
        gone = both[35 * n:] != 0
        out = [None if gone[t] else invertTF(np.ascontiguousarray(mats[t])) for t in range(n)]
        return out, dict(n_pairs=both[34 * n:35 * n].copy(), sum_e=both[32 * n:34 * n].view(np.float64).copy())
    if cpd is not None:
        T_out, _step, sig, Np, res2, sum_d2, n_live, empty = model.refit_cpd(surface_soa, T_dev, sigma2=cpd.get("sigma2", 0.0),
                                                                            outlier=cpd.get("outlier", 0.1), steps=steps)
        both = torch.cat([T_out.reshape(-1).view(torch.int32), sig.view(torch.int32), Np.view(torch.int32), res2.view(torch.int32),
                          sum_d2.view(torch.int32), n_live, empty]).cpu().numpy()
        mats = both[:32 * n].view(np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
        gone = both[41 * n:] != 0
        out = [None if gone[t] else invertTF(np.ascontiguousarray(mats[t])) for t in range(n)]
        f64 = lambda k: both[(32 + 2 * k) * n:(34 + 2 * k) * n].view(np.float64).copy()
        return out, dict(sigma2=f64(0), Np=f64(1), sum_res2=f64(2), sum_d2=f64(3), n_live=both[40 * n:41 * n].copy())
    r2 = float(np.float32(max_dist) * np.float32(max_dist))
    trim = []                                                                               # (n_within, d2_cut) of a trimmed call
    if normals is None:
        T_out, _step, n_close, sum_d2, empty, *trim = model.refit_transforms(surface_soa, T_dev, r2, steps=steps, keep_ratio=keep_ratio)
    elif surface_normals is None:
        T_out, _step, n_close, sum_d2, _n_plane, _res2, empty, *trim = model.refit_plane(surface_soa, T_dev, r2, normals, steps=steps,
                                                                                         keep_ratio=keep_ratio)
    else:
        if keep_ratio is None:
            got = model.refit_gicp(surface_soa, T_dev, r2, normals, surface_normals, epsilon=epsilon, steps=steps)
        else:
            got = model.refit_gicp_trimmed(surface_soa, T_dev, r2, keep_ratio, normals, surface_normals, epsilon=epsilon, steps=steps)
        T_out, _step, n_close, sum_d2, _n_pairs, _res2, empty, *trim = got
    both = torch.cat([T_out.reshape(-1).view(torch.int32), sum_d2.view(torch.int32), n_close, empty] +
                     ([trim[0], trim[1].view(torch.int32)] if trim else [])).cpu().numpy()
    mats = both[:32 * n].view(np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
    gone = both[35 * n:36 * n] != 0
    out = [None if gone[t] else invertTF(np.ascontiguousarray(mats[t])) for t in range(n)]
    summary = score_summary(both[34 * n:35 * n], both[32 * n:34 * n].view(np.float64), Q)
    if trim:
        summary.update(n_within=both[36 * n:37 * n].copy(), d2_cut=both[37 * n:].view(np.float32).copy())
    return out, summary


def quickTF_dev(pts_soa: torch.Tensor, TF: np.ndarray) -> torch.Tensor:
    """quickTF.m:5-7 on a resident [3, N] float64 cloud; TF 4x4 (numpy, row-vector convention)."""
    out = torch.empty_like(pts_soa)
    T = (C.c_double * 16)(*np.asarray(TF, dtype=np.float64).ravel(order="F"))
    check(lib().pcreg_dev_quick_tf(_p(pts_soa), pts_soa.shape[1], pts_soa.stride(0), T, _p(out), out.stride(0), _stream()))
    return out


def refine_by_distance_dev(pts1_soa: torch.Tensor, pts2_soa: torch.Tensor, n: int | torch.Tensor, maxDist: float):
    """completeExperimentFast.m:383-391 on resident [3, cap] float64 matched points: (T or None, #inliers)."""
    dev = pts1_soa.device
    cap = pts1_soa.shape[1]
    n_dev = n if isinstance(n, torch.Tensor) else torch.tensor([int(n)], dtype=torch.int32, device=dev)
    T16 = torch.zeros(16, dtype=torch.float64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    check(lib().pcreg_dev_refine_by_distance(_p(pts1_soa), _p(pts2_soa), _p(n_dev), cap, pts1_soa.stride(0), C.c_double(maxDist),
                                             _p(T16), _p(info), _stream()))
    cnt, empty = (int(v) for v in info.cpu())
    return (None if empty else T16.cpu().numpy().reshape(4, 4, order="F")), cnt


class FinalStage:
    """completeExperimentFast.m:280-394 on the device tier: for every cluster of promising spheres, move the surface by the
    cluster's RANSAC transform, describe it again WITHOUT local alignment, match against the model's no-LRF descriptors
    inside the cluster's sphere, keep the matches closer than maxDist; the cluster with the largest share of close matches
    gives T_refine and the final surface.

    TWO host synchronisations for the whole stage, whatever the number of clusters: (A) the sizes that fix the match
    grids -- every cluster's surviving keypoint count and descriptor count in its sphere (like the sweep's first read);
    (B) every cluster's match count, close-match count and refined transform, together.  The final surface
    quickTF(pts_tform, invertTF(T_refine)) is enqueued after (B) and stays on the device.

    ptsSurface [3, N] float64 on the device; featModel_noLRF [VM, 3] / descModel_noLRF [VM, 980] as for SphereSweep."""

    def __init__(self, ptsSurface: torch.Tensor, featModel_noLRF, descModel_noLRF, device: torch.device | None = None):
        self.dev = device or ptsSurface.device
        t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(self.dev).contiguous()
        self.pts = ptsSurface.to(self.dev)
        self.featM, self.descM = t(featModel_noLRF), t(descModel_noLRF)
        self.VM, self.D = self.descM.shape
        self.pipe = DescriptorPipeline(self.dev)

    def run(self, clusters, sample_pts, descOpt: dict, par: dict, R_desc: float, maxDist: float = 1.5, return_matches: bool = True) -> dict:
        """clusters = [(locCur [3], transCur [4,4])] (:283-288); sample_pts[i] = the keypoints drawn for cluster i (:297,
        pcRandomUniformSamples is the caller's: its random stream is not the library's business), [S_i, 3] numpy or [3, S_i]
        device tensors."""
        L = lib()
        dev, K = self.dev, len(clusters)
        i32, f64 = torch.int32, torch.float64
        if K == 0:
            raise ValueError("final stage: no clusters")
        opt = dict(descOpt, ALIGN_POINTS=False, VERBOSE=0)                                         # :300
        tf, feats, descs = [], [], []
        counters = torch.zeros((K, 2), dtype=i32, device=dev)
        for i, ((loc, T), kp) in enumerate(zip(clusters, sample_pts)):
            kp = kp if isinstance(kp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(kp, dtype=np.float64).T)).to(dev)
            pt = quickTF_dev(self.pts, invertTF(np.asarray(T, dtype=np.float64)))                  # :291
            f, d, c = self.pipe.describe_async(pt, kp, opt)                                        # :309-310
            counters[i].copy_(c)
            tf.append(pt); feats.append(f); descs.append(d)
        locs = torch.from_numpy(np.ascontiguousarray([np.asarray(c[0], dtype=np.float64) for c in clusters])).to(dev)
        n_in = torch.zeros(K, dtype=i32, device=dev)
        check(L.pcreg_dev_sphere_counts(_p(self.featM), self.VM, _p(locs), K, C.c_double(R_desc), _p(n_in), _stream()))
        cnt = torch.cat([counters.view(-1), n_in]).cpu().numpy()                                   # ---- sync A: sizes only
        V = cnt[0:2 * K:2].astype(np.int64); over = cnt[1:2 * K:2]; nM = cnt[2 * K:].astype(np.int64)
        if over.any():
            raise ValueError(f"a support holds {int(over.max())} points: more than an LDS-resident support may have (lower max_pts)")
        seg_off_h = np.zeros(K + 1, dtype=np.int32); seg_off_h[1:] = np.cumsum(nM)
        tot = int(seg_off_h[-1])
        seg_off = torch.from_numpy(seg_off_h).to(dev)
        rows_all = torch.empty(max(tot, 1), dtype=i32, device=dev)
        featCur_all = torch.empty((max(tot, 1), 3), dtype=f64, device=dev)
        check(L.pcreg_dev_sphere_select_batched(_p(self.featM), self.VM, _p(locs), K, C.c_double(R_desc), _p(seg_off), _p(rows_all), _p(featCur_all),
                                                None, _stream()))                                  # :319-322, every cluster's sphere
        n_pairs = torch.zeros(K, dtype=i32, device=dev)
        info = torch.zeros((K, 2), dtype=i32, device=dev); info[:, 1] = 1
        T16 = torch.zeros((K, 16), dtype=f64, device=dev)
        pairs = []
        n_tot = torch.tensor([tot], dtype=i32, device=dev)
        for i in range(K):
            v, n, lo = int(V[i]), int(nM[i]), int(seg_off_h[i])
            pr = torch.zeros((max(v, 1), 2), dtype=i32, device=dev)
            pairs.append(pr)
            if v == 0 or n == 0:
                continue
            descCur = torch.empty((n, self.D), dtype=f64, device=dev)
            check(L.pcreg_dev_gather_rows_f64(_p(self.descM), self.D, _p(rows_all[lo:lo + n]), _p(n_tot), n, _p(descCur), _stream()))
            self.pipe.match(descs[i][:v], v, descCur, n, par, pairs_out=pr, n_pairs_out=n_pairs[i:i + 1])          # :344
            p1 = torch.empty((3, v), dtype=f64, device=dev); p2 = torch.empty((3, v), dtype=f64, device=dev)
            check(L.pcreg_dev_gather_matched_rows(_p(pr), _p(n_pairs[i:i + 1]), v, _p(feats[i]), _p(featCur_all[lo:lo + n]), _p(p1), _p(p2), _stream()))
            check(L.pcreg_dev_refine_by_distance(_p(p1), _p(p2), _p(n_pairs[i:i + 1]), v, v, C.c_double(maxDist), _p(T16[i]), _p(info[i]),
                                                 _stream()))                                       # :357-391 for every cluster
        back = torch.cat([n_pairs.to(f64), info.view(-1).to(f64), T16.view(-1)]).cpu().numpy()     # ---- sync B: the results
        npr = back[:K].astype(np.int64); inf = back[K:3 * K].reshape(K, 2).astype(np.int64); Ts = back[3 * K:].reshape(K, 16)
        with np.errstate(invalid="ignore", divide="ignore"):
            prec = np.where(npr > 0, inf[:, 0] / np.maximum(npr, 1) * 100.0, np.nan)              # :373
        best = 0 if np.all(np.isnan(prec)) else int(np.nanargmax(prec))                           # :381, MATLAB's max
        T_refine = None if inf[best, 1] else Ts[best].reshape(4, 4, order="F")
        pts_final = quickTF_dev(tf[best], invertTF(T_refine)) if T_refine is not None else tf[best]   # :394, stays on the device
        out = dict(num_keypoints=V, num_desc=nM, num_matches=npr, num_close=inf[:, 0], precisions=prec, best=best, T_refine=T_refine,
                   pts_final=pts_final, pts_tform=tf, host_syncs=2)
        if return_matches:                                                                        # a third, optional read (tests, plots)
            out["matches"] = [pairs[i][:npr[i]].cpu().numpy().astype(np.uint32) for i in range(K)]
            out["model_rows"] = [rows_all[seg_off_h[i]:seg_off_h[i + 1]].cpu().numpy().astype(np.int64) for i in range(K)]
        return out


__all__ = ["SphereSweep", "FinalStage", "pcUniformSamples", "promising_clusters", "largest_cluster", "quickTF_dev", "refine_by_distance_dev", "invertTF"]
