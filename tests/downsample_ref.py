"""The downsampling contract of include/pcreg.h (pcreg_downsample_grid_f32) restated in numpy, literally: cells in float64 on the
widened float32 coordinates, np.unique(cells, axis=0) for the voxel order and the labels, np.add.at for the sums -- it adds
one element after the other in index order, which is the contract's ascending row order (np.sum, np.add.reduceat and
bincount(weights=) add pairwise or in blocks and are NOT used).  The oracle of tests/test_gpu_downsample.py; itself checked
against a triple loop on hand-made clouds in tests/test_downsample_ref.py."""
import numpy as np

MAX_CELLS = 1 << 21


class Refused(Exception):
    """the cloud spans 2^21 or more cells along an axis"""


def live_rows(pts):
    return np.isfinite(np.asarray(pts, np.float32)).all(axis=1)


def cells_of(pts, step, live=None):
    """(lo [3] float32, cells [n_live, 3] int64) of the live rows"""
    p = np.asarray(pts, np.float32)
    live = live_rows(p) if live is None else live
    pl = p[live]
    lo = pl.min(axis=0)                                                   # the float32 minimum
    with np.errstate(over="ignore"):
        q = np.floor((pl.astype(np.float64) - lo.astype(np.float64)) / np.float64(step))
    if not (q < MAX_CELLS).all():
        raise Refused()
    return lo, q.astype(np.int64)


def downsample_ref(pts, step):
    """-> (out [n_out, 3] float32, count [n_out] int32, label [n] int32: 1-based output row, 0 for a dead row)"""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    n = p.shape[0]
    live = live_rows(p)
    label = np.zeros(n, np.int32)
    if not live.any():
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), label
    _, cells = cells_of(p, step, live)
    vox, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    u = vox.shape[0]
    sums = np.zeros((u, 3), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        np.add.at(sums, inv, p[live].astype(np.float64))                  # row after row, in ascending row order
        count = np.zeros(u, np.int64)
        np.add.at(count, inv, 1)
        out = (sums / count[:, None].astype(np.float64)).astype(np.float32)
    label[live] = inv + 1
    return out, count.astype(np.int32), label
