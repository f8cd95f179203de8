"""Stale workspaces and reused handles change no result (tests/ws_state.py holds the registry and the three checks).

Every device-tier entry with a *_workspace size function in include/pcreg.h has a case; test_every_size_function_has_a_case
parses the header and needs no GPU.  Each case runs `fills` on every shape of its sequence, `sequence` once under every
pcreg_debug_set setting that makes its launcher lay buffers out differently, and `outputs` on its first shape.
"""
import os
import re

import numpy as np
import pytest

import ws_state
from ws_state import CASES

gpu = pytest.mark.gpu
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcreg.h")


def size_functions():
    with open(HEADER) as f:
        return sorted(set(re.findall(r"^size_t\s+(pcreg_\w+_workspace)\s*\(", f.read(), flags=re.M)))


def test_every_size_function_has_a_case():
    declared = size_functions()
    assert len(declared) >= 31, declared
    covered = {c.size_fn for c in CASES.values()}
    assert not [f for f in declared if f not in covered], "a *_workspace size function of include/pcreg.h without a case in tests/ws_state.py"
    assert covered <= set(declared), covered - set(declared)
    for c in CASES.values():
        assert len(c.shapes) >= 2 and callable(c.need) and callable(c.call) and callable(c.expect) and "default" in c.flags, c.name


_FILLS = [pytest.param(name, k, id=f"{name}-{k}") for name, c in CASES.items() for k in range(len(c.shapes))]
_SEQUENCES = [pytest.param(name, flag, id=f"{name}-{flag}") for name, c in CASES.items() for flag in c.flags]


@gpu
@pytest.mark.parametrize("name,k", _FILLS)
def test_fills(name, k):
    ws_state.fills(CASES[name], CASES[name].shapes[k])


@gpu
@pytest.mark.parametrize("name,flag", _SEQUENCES)
def test_sequence(name, flag, debug_set):
    case = CASES[name]
    for key, value in case.flags[flag].items():
        debug_set(key, value)
    ws_state.sequence(case, case.shapes_for(flag))


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_outputs(name):
    ws_state.outputs(CASES[name])


@gpu
def test_sequence_ransac_without_refine():
    ws_state.sequence(CASES["ransac"], CASES["ransac"].norefine)


# ---- handles keep no call's state -----------------------------------------------------------------------------------------------
def _export(pm):
    """perm, the sorted copy, the tile boxes and the preparation record of a prepared model, as bytes-comparable arrays"""
    import ctypes as C
    import torch
    from pcreg_amd._lib import check, lib
    nt = (pm.M + 511) // 512
    perm = torch.full((pm.M,), -7, dtype=torch.int32, device=ws_state.dev())
    ms = torch.zeros(3 * pm.M, dtype=torch.float32, device=ws_state.dev())
    tb = torch.zeros(6 * nt, dtype=torch.float32, device=ws_state.dev())
    prep = (C.c_float * 24)()
    check(lib().pcreg_debug_dev_model_export(pm.handle, ws_state.ptr(perm), ws_state.ptr(ms), ws_state.ptr(tb), prep, ws_state.stream()))
    torch.cuda.synchronize()
    return [perm.cpu().numpy(), ms.cpu().numpy(), tb.cpu().numpy(), np.frombuffer(bytes(prep), np.uint32).copy()]


def _np(res):
    import torch
    torch.cuda.synchronize()
    if isinstance(res, dict):
        return {k: _np(v) for k, v in res.items()}
    if isinstance(res, (tuple, list)):
        return [_np(v) for v in res]
    return None if res is None else res.cpu().numpy()


def _documented(name, res):
    """the part of an operation's result the header documents as written: lists stop at their counts"""
    res = _np(res)
    count, lists = _LISTS.get(name, (None, ()))
    for k in lists:
        res[k] = res[k][:int(res[count][0])]
    return res


_LISTS = {"denoise": ("n_inliers", ("inliers",)), "fps": ("n_out", ("idx", "dist")), "iss": ("n_keypoints", ("keypoints",))}


def _model_ops(pm, surf, T):
    """every operation of a prepared model through PreparedModel's own methods, on the workspaces it caches and reuses"""
    import torch
    q, Td = ws_state.soa32(surf), ws_state.t16(T)
    r2 = np.float32(1.5) ** 2
    nrm = {}

    def normals():
        nrm["n"] = pm.normals(8, viewpoint=(50.0, 28.0, 1000.0))
        return nrm["n"]
    return [("search", lambda: pm.knn(q, 2)), ("knn", lambda: pm.knn(q, 8)), ("range", lambda: pm.rangesearch(q, 9.0)),
            ("score", lambda: pm.score_transforms(q, Td, r2, rows=True)), ("refit", lambda: pm.refit_transforms(q, Td, r2, steps=3)),
            ("cluster", lambda: pm.cluster(r2)), ("dbscan", lambda: pm.dbscan(r2, 4)), ("normals", normals),
            ("denoise", lambda: pm.denoise(4, 1.0)), ("fps", lambda: pm.farthest_points(200)), ("fpfh", lambda: pm.fpfh(8, nrm["n"])),
            ("iss", lambda: pm.iss_keypoints(3.0, 2.0)), ("refit_plane", lambda: pm.refit_plane(q, Td, r2, nrm["n"]))]


def _handle_scene():
    from ws_state import _points, _search_model
    model, surf = _points(50000, 3000, 3)
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1, 3, :3] = [0.05, -0.04, 0.03]
    T[2] = 0.0
    return _search_model(50000), model, surf, T


@gpu
def test_a_prepared_model_is_immutable():
    """M = 50000: the exported perm, sorted copy, tile boxes and preparation record are the same words after every operation has run
    on the handle; each operation, repeated after all the others, gives its first bits (its cached workspace then holds whatever
    the other shapes left)"""
    import torch
    from test_gpu_knn_k import _top2
    pm, model, surf, T = _handle_scene()
    before = _export(pm)
    assert sorted(before[0].tolist()) == list(range(pm.M))
    ops = _model_ops(pm, surf, T)
    first = {name: _documented(name, op()) for name, op in ops}
    top2 = _top2(pm, surf)
    ws_state.same_bits(_np(pm.knn(ws_state.soa32(surf[:70]), 32))[0][:, :2], top2[0][:70], "k = 32 on 70 queries after k = 8 on 3000")
    ws_state.same_bits(_export(pm), before, "the prepared model after every operation")
    for name, op in ops:
        ws_state.same_bits(_documented(name, op()), first[name], name + " repeated")
    ws_state.same_bits(first["search"][0], top2[0], "k = 2 against the top-2 search")
    ws_state.same_bits(_export(pm), before, "the prepared model after every operation, twice")
    torch.cuda.synchronize()


@gpu
def test_two_streams_one_handle_two_workspaces():
    """every operation whose header lets a handle serve several streams at once (the top-2 search under the handle's own statement),
    each stream with buffers of its own, other queries and other parameters on the two streams so that a scratch word shared
    through the handle would show: every result equals its serial result"""
    import torch
    from pcreg_amd._lib import lib
    from pcreg_amd.device import NdtModel
    pm, model, surf, T = _handle_scene()
    L, dev, M = lib(), ws_state.dev(), pm.M
    i32, f32, f64, u8, i64 = torch.int32, torch.float32, torch.float64, torch.uint8, torch.int64
    ws = lambda n: torch.full((max(int(n), 256),), 0xFF, dtype=u8, device=dev)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    nrm = pm.normals(8, viewpoint=(50.0, 28.0, 1000.0))
    nm = NdtModel(ws_state.soa32(model), 4.0, 6)
    P = 3

    def side(k):
        """-> [(name, enqueue)]: k = 0, 1 choose the queries, the transforms and every parameter"""
        q = ws_state.soa32(surf[:2000] if k == 0 else surf[1200:] + np.float32(0.25))
        Td = ws_state.t16(T if k == 0 else T[::-1].copy())
        Q, B = q.shape[1], Td.shape[0]
        qn = pm.normals(8)[:, :Q].contiguous()                                      # any unit vectors serve as query normals
        r2 = np.float32((1.5, 2.0)[k]) ** 2
        kk, K, nt = (8, 5)[k], (200, 120)[k], (128, 192)[k]
        _, so = pm.rangesearch_count(q, float(r2))
        total = int(so[-1].item())
        _, fso = pm.fpfh_radius_count(float(r2))
        ftotal = int(fso[-1].item())
        tb = lambda: new((B, 16), f64)
        fit = lambda tail: [new(M, i32)] + [new((P,) + t, d) for t, d in tail]
        return [
            ("search", lambda: ws_state.top2(pm, q, new((Q, 2), i32), new((Q, 2), f32), ws(L.pcreg_dev_model_search_workspace(Q, M)))),
            ("knn", lambda: pm.knn(q, kk, out=(new((Q, kk), i32), new((Q, kk), f32), ws(L.pcreg_dev_model_knn_workspace(Q, M, kk))))),
            ("range_count", lambda: pm.rangesearch_count(q, r2, out=(new(Q, i32), new(Q + 1, i64), ws(L.pcreg_dev_model_range_workspace(Q, M))))),
            ("range_fill", lambda: pm.rangesearch_fill(q, r2, so, new(total, i32), new(total, f32), ws=ws(L.pcreg_dev_model_range_workspace(Q, M)))),
            ("score", lambda: pm.score_transforms(q, Td, r2, rows=True, out=(new(B, i32), new(B, f64), new((B, Q), i32), new((B, Q), f32),
                                                                           ws(L.pcreg_dev_model_score_workspace(Q, B, M))))),
            ("refit", lambda: pm.refit_transforms(q, Td, r2, steps=2, out=(tb(), tb(), new(B, i32), new(B, f64), new(B, i32),
                                                                           ws(L.pcreg_dev_model_refit_workspace(Q, B, M)), tb()))),
            ("refit_plane", lambda: pm.refit_plane(q, Td, r2, nrm, steps=2, out=(tb(), tb(), new(B, i32), new(B, f64), new(B, i32), new(B, f64), new(B, i32),
                                                                                 ws(L.pcreg_dev_model_refit_plane_workspace(Q, B, M)), tb()))),
            ("refit_gicp", lambda: pm.refit_gicp(q, Td, r2, nrm, qn, steps=2, out=(tb(), tb(), new(B, i32), new(B, f64), new(B, i32), new(B, f64), new(B, i32),
                                                                                   ws(L.pcreg_dev_model_refit_gicp_workspace(Q, B, M)), tb()))),
            ("refit_cpd", lambda: pm.refit_cpd(q[:, :300].contiguous(), Td, sigma2=(1.0, 2.5)[k], outlier=0.1, steps=2,
                                               out=(tb(), tb(), new(B, f64), new(B, f64), new(B, f64), new(B, f64), new(B, i32), new(B, i32),
                                                    ws(L.pcreg_dev_model_refit_cpd_workspace(300, B, M)), tb()))),
            ("ndt_refit", lambda: nm.refit(q, Td, steps=2, out=(tb(), tb(), new(B, i32), new(B, f64), new(B, i32), ws(L.pcreg_dev_ndt_refit_workspace(Q, B)), tb()))),
            ("cluster", lambda: pm.cluster(r2, out=(new(M, i32), new(1, i32), new(M, i32), new(M, i32), ws(L.pcreg_dev_model_cluster_workspace(M))))),
            ("dbscan", lambda: pm.dbscan(r2, (4, 2)[k], out=(new(M, i32), new(1, i32), new(M, u8), new(M, i32), new(M, i32), new(M, i32),
                                                              ws(L.pcreg_dev_model_dbscan_workspace(M))))),
            ("normals", lambda: pm.normals(kk, variation=True, out=(new((3, M), f32), new(M, f32), ws(L.pcreg_dev_model_normals_workspace(M, kk))))),
            ("denoise", lambda: pm.denoise(kk, (1.0, 0.5)[k], out=(new(M, f64), torch.zeros(M, dtype=i32, device=dev), new(1, i32), new(4, f64),
                                                                    ws(L.pcreg_dev_model_denoise_workspace(M, kk))))),
            ("fps", lambda: pm.farthest_points(K, out=(torch.zeros(K, dtype=i32, device=dev), torch.zeros(K, dtype=f32, device=dev), new(1, i32), new(1, f32),
                                                       new(M, f32), new(M, i32), new(1, i32), ws(L.pcreg_dev_model_fps_workspace(M, K))))),
            ("fpfh", lambda: pm.fpfh(kk, nrm, spfh=True, out=(new((M, 33), f64), new((M, 33), u8), ws(L.pcreg_dev_model_fpfh_workspace(M, kk))))),
            ("fpfh_radius", lambda: pm.fpfh_radius(float(r2), nrm, fso, ftotal, spfh=True, out=(new((M, 33), f64), new((M, 33), i32), new(M, i32),
                                                                                                ws(L.pcreg_dev_model_fpfh_radius_workspace(M, ftotal))))),
            ("iss", lambda: pm.iss_keypoints((3.0, 4.0)[k], (2.0, 3.0)[k], out=(new(M, i32), new((M, 3), f64), new(M, f64), torch.zeros(M, dtype=i32, device=dev),
                                                                                  new(1, i32), ws(L.pcreg_dev_model_iss_workspace(M))))),
            ("fit_planes", lambda: pm.fit_planes(0.5, max_planes=P, n_trials=nt, min_inliers=20, seed=7 + k, out=tuple(fit(
                [((4,), f64), ((3,), f64), ((), i32), ((), f64)]) + [new(1, i32), new(P, i32), new(P, i64), new(P, i32), ws(L.pcreg_dev_model_fit_planes_workspace(M, nt))]))),
            ("fit_spheres", lambda: pm.fit_spheres(0.5, max_spheres=P, n_trials=nt, min_inliers=20, seed=7 + k, out=tuple(fit(
                [((4,), f64), ((), i32), ((), f64), ((), i32)]) + [new(1, i32), new(P, i32), new(P, i64), new(P, i32), ws(L.pcreg_dev_model_fit_spheres_workspace(M, nt))]))),
            ("fit_cylinders", lambda: pm.fit_cylinders(0.5, nrm, max_radius=6.0, max_cylinders=P, n_trials=nt, min_inliers=20, seed=7 + k, out=tuple(fit(
                [((7,), f64), ((2,), f64), ((), i32), ((), f64), ((), i32)]) + [new(1, i32), new(P, i32), new(P, i64), new(P, i32),
                                                                              ws(L.pcreg_dev_model_fit_cylinders_workspace(M, nt))]))),
        ]
    sides = [side(0), side(1)]
    serial = [[_np(op()) for _, op in s] for s in sides]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    try:
        for n, (name, _) in enumerate(sides[0]):
            res = []
            for st, s in zip(streams, sides):
                with torch.cuda.stream(st):
                    res.append(s[n][1]())
            torch.cuda.synchronize()
            for i in range(2):
                ws_state.same_bits(_np(res[i]), serial[i][n], f"{name}, stream {i}")
            assert name in ("search",) or not _same_or_none(serial[0][n], serial[1][n]), f"{name}: the two streams must differ in their results"
    finally:
        nm.close()


def _same_or_none(a, b):
    try:
        ws_state.same_bits(a, b)
    except AssertionError:
        return False
    return True


@gpu
def test_a_descriptor_set_keeps_no_calls_options(oracle_c):
    """segmented calls on one pair of pcreg_desc_set handles with options P1, P2 (another metric_factor), CHANGE_METRIC off and P1
    again, plain getMatchesOnSet calls in between: each equals the host form on raw arrays (the lazily made row-major copy and
    the powered rows "of the last call" are remade when the options change)"""
    from pcreg_amd import api as pc
    descS, descM, rows, par = ws_state._seg_scene("ragged")
    rows = [r for r in rows if len(r)]
    P1, P2, P3 = par, dict(par, metric_factor=0.8), dict(par, CHANGE_METRIC=False)
    want = {id(p): [pc.getMatches(descS, descM[r], p) for r in rows] for p in (P1, P2, P3)}
    whole = {id(p): pc.getMatches(descS, descM, p) for p in (P1, P2, P3)}
    for p in (P1, P2, P3):
        np.testing.assert_array_equal(whole[id(p)], oracle_c.getMatches(descS, descM, p))
    with pc.DescSet(descS) as hS, pc.DescSet(descM) as hM:
        for step, p in enumerate((P1, P2, P3, P1, P3, P1)):
            got = pc.getMatchesSegmentedOnSet(hS, hM, rows, p)
            for z, (g, w) in enumerate(zip(got, want[id(p)])):
                np.testing.assert_array_equal(g, w, err_msg=f"step {step}, segment {z}")
            q = (P2, P3, P1)[step % 3]
            np.testing.assert_array_equal(pc.getMatchesOnSet(hS, hM, None, q), whole[id(q)], err_msg=f"step {step}, the plain call")


@gpu
def test_sweep_objects_keep_no_runs_state():
    """SphereSweep.run with parameter set X, then Y (fewer, smaller spheres), then X again on one object: the third run's matches,
    counts and transforms are the first's, bit for bit"""
    from pcreg_amd.sweep import SphereSweep
    from test_gpu_sweep import OPT, PAR, _scene
    featM, descM, featS, descS = _scene()
    sw = SphereSweep(featM, descM, featS, descS)
    X = dict(R_desc=9.0, d_spheres=6.0, min_pts=500, putative_thresh=60, seed=3)
    Y = dict(R_desc=6.0, d_spheres=9.0, min_pts=150, putative_thresh=20, seed=3)
    first = sw.run(PAR, OPT, **X)
    other = sw.run(PAR, OPT, **Y)
    again = sw.run(PAR, OPT, **X)
    assert len(first["trial"]) >= 1 and 0 < len(other["centres"]) < len(first["centres"])
    assert max(other["num_desc"]) < max(first["num_desc"])
    for k in ("centres", "num_desc", "num_putative", "trial", "statsPutative", "statsSuccess", "statsInliers", "statsRatio"):
        ws_state.same_bits(np.asarray(again[k]), np.asarray(first[k]), k)
    for k in ("matches", "model_rows"):
        assert len(again[k]) == len(first[k])
        for a, b in zip(again[k], first[k]):
            ws_state.same_bits(a, b, k)
    for a, b in zip(again["transforms"], first["transforms"]):
        assert (a is None) == (b is None)
        if a is not None:
            ws_state.same_bits(a, b, "transforms")


@gpu
def test_final_stage_keeps_no_runs_state(oracle_c, oracle_py):
    """FinalStage.run on one object with four clusters and R_desc 14, then two clusters with fewer keypoints and R_desc 9, then the
    first set again: the third run's matches, counts, precisions and transforms are the first's, bit for bit"""
    import torch
    from pcreg_amd.device import soa
    from pcreg_amd.sweep import FinalStage
    from test_gpu_descriptors import OPT, keypoints
    from test_gpu_final_stage import PAR, _perturbed, _scene
    model, surface, kpM, T_true = _scene(5)
    featM, descM = oracle_c.getSpacialHistogramDescriptors(model, kpM, dict(OPT, ALIGN_POINTS=False))
    rng = np.random.default_rng(9)
    clusters = [(np.array([25.0, 18.0, 12.0]), _perturbed(T_true, rng, 0.004, 0.03)), (np.array([500.0, 500.0, 500.0]), _perturbed(T_true, rng)),
                (np.array([24.0, 19.0, 12.0]), _perturbed(T_true, rng, 0.012, 0.1)), (np.array([30.0, 12.0, 12.0]), _perturbed(T_true, rng))]
    near = kpM[(kpM[:, 0] > 10) & (kpM[:, 0] < 40)]
    kps = [np.vstack([keypoints(200, 30 + i), near + rng.normal(0, 0.05, near.shape)]) for i in range(4)]
    dev = torch.device("cuda", 0)
    fs = FinalStage(soa(torch.from_numpy(surface).to(dev)), featM, descM, device=dev)
    X = lambda: fs.run(clusters, kps, OPT, PAR, 14.0, maxDist=1.5)
    first = X()
    other = fs.run(clusters[2:], [k[:150] for k in kps[2:]], OPT, PAR, 9.0, maxDist=1.0)
    again = X()
    assert first["T_refine"] is not None and max(first["num_close"]) >= 10 and max(other["num_desc"]) < max(first["num_desc"])
    for k in ("num_keypoints", "num_desc", "num_close", "precisions"):
        ws_state.same_bits(np.asarray(again[k]), np.asarray(first[k]), k)
    assert again["best"] == first["best"]
    ws_state.same_bits(again["T_refine"], first["T_refine"], "T_refine")
    for a, b in zip(again["matches"], first["matches"]):
        ws_state.same_bits(a, b, "matches")
    ws_state.same_bits(again["pts_final"].cpu().numpy(), first["pts_final"].cpu().numpy(), "pts_final")
