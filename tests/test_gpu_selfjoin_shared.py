"""What the self-joins of a prepared model share (knn_walk.hpp, knn_selfjoin.hpp, chunk_scan.hpp), once per pass that uses it: the
row prologue and the search header, the staging rule for non-finite rows, the visit rule, the k-list walk and the compaction of a
per-row predicate into an ascending list.

One model of 1537 rows (three full tiles of 512 and a tile of one row): two cubes of side 10 a thousand units apart, so that the
ordering grid puts each cube in a cell of its own and the tiles are [cube a][both][cube b][one row of cube b], and five rows
that are not finite.  For clusterPoints, normals (k = 6), pcdenoise (k = 4), FPFH (k = 8), ISS and plane fitting:
  * every output with "knn_nocull" set is byte-equal to the outputs without it;
  * with "knn_stats" on, the searches counted per call are the pass's walks, `nominal` is n * n per self-join walk and
    n (n + 1) / 2 for the clustering (n = 4 tiles), every tile pair is visited without culling, and fewer with it.

Two variants of the five rows.  "mixed" is NaN, +inf and -inf, each in a different coordinate.  An infinite coordinate makes the
model's box infinite, the ordering grid then has ONE cell (knn_fast.hip: inv_s = 0) and the sorted order is the arrival order of
an atomic counter: the tiles are no longer compact, and how many pairs the rule skips is neither predictable nor repeatable.  So
"mixed" asserts visited <= nominal and everything else, and "nan" (the same rows with NaN where "mixed" has an infinity) asserts
visited < nominal -- exactly the 4 pairs (2 for the clustering) between the tile of cube a alone and the two of cube b alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N_TILES = 1537, 4
BAD_ROWS = (3, 200, 401, 650, 767)                   # all among cube a's rows


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _model(variant):
    rng = np.random.default_rng(20261020)
    m = rng.uniform(0.0, 10.0, (M, 3))
    m[768:, 0] += 1000.0                             # cube b: rows 768 .. 1536
    m = m.astype(np.float32)
    inf = np.float32(np.inf) if variant == "mixed" else np.float32(np.nan)
    m[BAD_ROWS[0], 0] = np.nan
    m[BAD_ROWS[1], 1] = inf
    m[BAD_ROWS[2], 2] = -inf
    m[BAD_ROWS[3], 2] = np.nan
    m[BAD_ROWS[4], 0] = inf
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _samples():
    s = np.random.default_rng(7).integers(0, M, (2, 16, 3)).astype(np.int32)
    s[0, 0] = (BAD_ROWS[0], 10, 20)                  # a sample with a non-finite row
    return s


def _stats(reset=True):
    from pcreg_amd._lib import check, lib
    out = (C.c_longlong * 4)()
    check(lib().pcreg_debug_knn_stats(out, 1 if reset else 0))
    return [int(v) for v in out]


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8).tobytes()


def _listed(lst, n):
    """an ascending row list: (its number, its first `number` entries)"""
    n = int(n.cpu().item())
    return [np.int32(n).tobytes(), _bytes(lst[:n])]


def _cluster(pm):
    return [_bytes(t) for t in pm.cluster(1.5 ** 2)]


def _normals(pm):
    return [_bytes(t) for t in pm.normals(6, viewpoint=(5.0, 5.0, 100.0), variation=True)]


def _denoise(pm):
    r = pm.denoise(4, 1.0)
    return [_bytes(r["mean_dist"]), _bytes(r["stats"])] + _listed(r["inliers"], r["n_inliers"])


def _fpfh(pm):
    nrm = pm.normals(6, viewpoint=(5.0, 5.0, 100.0))
    _stats()                                          # (the normals' walk is not this pass's)
    return [_bytes(t) for t in pm.fpfh(8, nrm, spfh=True)]


def _iss(pm):
    # gammas no eigenvalue ratio reaches and one neighbour: every finite row of a cube is a candidate, so no workgroup of the
    # suppression walk is without work and it visits what the rule leaves it
    r = pm.iss_keypoints(3.0, 2.0, 1e30, 1e30, 1)
    live = np.ones(M, bool)
    live[list(BAD_ROWS)] = False
    s = r["saliency"].cpu().numpy()
    assert (s[live] > 0).all() and (s[~live] == 0).all()
    return [_bytes(r["n_neighbors"]), _bytes(r["eig"]), _bytes(r["saliency"])] + _listed(r["keypoints"], r["n_keypoints"])


def _planes(pm):
    smp = torch.from_numpy(_samples()).to(_dev())
    r = pm.fit_planes(0.5, max_planes=2, n_trials=16, min_inliers=3, samples=smp)
    return [_bytes(r[key]) for key in ("labels", "planes", "centres", "counts", "rmse", "n_planes", "best_trial", "best_cost", "best_count")]


SELF = N_TILES * N_TILES
# pass: (the call, its walks, nominal per call, the tile pairs the rule skips on the "nan" model)
PASSES = {
    "cluster": (_cluster, 1, N_TILES * (N_TILES + 1) // 2, 2),
    "normals": (_normals, 1, SELF, 4),
    "denoise": (_denoise, 1, SELF, 4),
    "fpfh": (_fpfh, 1, SELF, 4),
    "iss_keypoints": (_iss, 2, 2 * SELF, 8),
    "fit_planes": (_planes, 0, 0, 0),
}


@pytest.mark.parametrize("variant", ["mixed", "nan"])
@pytest.mark.parametrize("name", list(PASSES))
def test_pass(name, variant, debug_set):
    from pcreg_amd.device import PreparedModel
    call, walks, nominal, skipped = PASSES[name]
    t = torch.from_numpy(np.array(_model(variant).T, order="C")).to(_dev())
    pm = PreparedModel(t)
    try:
        debug_set("knn_stats", 1)
        _stats()
        a = call(pm)
        torch.cuda.synchronize()
        culled = _stats()
        debug_set("knn_nocull", 1)
        b = call(pm)
        torch.cuda.synchronize()
        full = _stats()
        debug_set("knn_nocull", 0)
    finally:
        pm.close()
    print(f"{name} [{variant}]: searches, visited, nominal = {culled[:3]} with culling, {full[:3]} without")
    assert len(a) == len(b) and all(x == y for x, y in zip(a, b))
    assert culled[0] == walks and full[0] == walks
    assert culled[2] == nominal and full[2] == nominal
    assert full[1] == nominal
    if variant == "nan":
        assert culled[1] == nominal - skipped
        assert walks == 0 or culled[1] < nominal
    else:
        assert culled[1] <= nominal
