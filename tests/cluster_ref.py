"""fp32 clustering reference (tests/cluster_ref.c), compiled on first use with -ffp-contract=off.

cluster(points, r2) -> (label [M] int32, cl_off [C + 1] int32, members [M] int32): the connected components of the graph in which
rows i != j are adjacent iff their chain distance fmaf(dz,dz,fmaf(dy,dy,dx*dx)) is <= r2 (the SQUARED radius, compared in
float32); a row with a non-finite coordinate is a cluster of its own; clusters are numbered in ascending order of their smallest
row and cluster c is members[cl_off[c] .. cl_off[c + 1]), ascending: the contract of pcreg_cluster_points_f32 and friends, which
must match it bit for bit.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="cluster_ref_"), "libcluster_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               os.path.join(_HERE, "cluster_ref.c"), "-o", out, "-lm"])
        L = C.CDLL(out)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.cluster_ref.restype = C.c_int
        L.cluster_ref.argtypes = [vp, i, i, f, vp, vp, vp, vp]
        _lib = L
    return _lib


def cluster(points, r2):
    m = np.asfortranarray(np.asarray(points, np.float32).reshape(-1, 3))
    M = m.shape[0]
    r2 = float(np.float32(r2))
    assert r2 >= 0.0, "the squared radius is a number >= 0"
    md = m if M else np.zeros((1, 3), np.float32, order="F")
    label = np.zeros(max(M, 1), np.int32)
    cl_off = np.zeros(M + 1, np.int32)
    members = np.zeros(max(M, 1), np.int32)
    nc = C.c_int32(0)
    rc = lib().cluster_ref(md.ctypes.data, M, max(M, 1), r2, label.ctypes.data, C.byref(nc), cl_off.ctypes.data, members.ctypes.data)
    assert rc == 0, rc
    return label[:M].copy(), cl_off[:nc.value + 1].copy(), members[:M].copy()


def first_and_sizes(label, cl_off, members):
    """first[c] = the smallest row of cluster c, sizes[c] = its rows"""
    return members[cl_off[:-1]].astype(np.int32), np.diff(cl_off).astype(np.int32)
