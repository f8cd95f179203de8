"""The "knn_seed_fused" key in one binary: one JSON line.

Median of 20 event-timed two-nearest search calls after 5 warm-ups, the key alternating 0 (seeding and the direct answers in one
launch) and 1 (two launches) three times in one process, on the bench crop and on scattered queries (the shapes of
scripts/knn_k_bench.py); the answers of every setting compared bit for bit, and the direct counters of one search.

    python3 scripts/knn_seed_fused_ab.py [keys, default 0,1]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import BBOX, synth  # noqa: E402
from pcreg_amd._lib import check, lib  # noqa: E402
from pcreg_amd.device import PreparedModel  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_k_bench import _median_ms, _p  # noqa: E402


def main():
    L, dev = lib(), torch.device("cuda", 0)
    model, surf, _ = synth(1_000_000, 50_000)
    rng = np.random.default_rng(1)
    scattered = (rng.random((50_000, 3)) * BBOX).astype(np.float32)
    pm = PreparedModel(torch.from_numpy(np.ascontiguousarray(model.T)).to(dev))
    out = {}
    for name, s in (("bench_crop", surf.astype(np.float32)), ("scattered", scattered)):
        Q = len(s)
        q = torch.from_numpy(np.ascontiguousarray(s.T)).to(dev)
        i2 = torch.empty((Q, 2), dtype=torch.int32, device=dev)
        d2 = torch.empty((Q, 2), dtype=torch.float32, device=dev)
        ws = torch.empty(L.pcreg_dev_model_search_workspace(Q, pm.M), dtype=torch.uint8, device=dev)
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = lambda: check(L.pcreg_dev_model_search_f32(pm.handle, _p(q), Q, Q, C.c_int32(0), _p(i2), _p(d2), _p(ws), C.c_size_t(ws.numel()), stream()))
        keys = tuple(int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else "0,1").split(","))
        res = {k: [] for k in keys}
        ref = None
        for rep in range(3):
            for key in keys:
                check(L.pcreg_debug_set(b"knn_seed_fused", key))
                res[key].append(round(_median_ms(fn, 20, 5), 4))
                torch.cuda.synchronize()
                got = (i2.cpu().numpy().copy(), d2.cpu().numpy().view(np.uint32).copy())
                if ref is None:
                    ref = got
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), "the settings of the key differ"
        check(L.pcreg_debug_set(b"knn_seed_fused", 0))
        check(L.pcreg_debug_set(b"knn_direct_stats", 1))
        st = (C.c_longlong * 3)()
        check(L.pcreg_debug_knn_direct_stats(st, 1))
        fn()
        torch.cuda.synchronize()
        check(L.pcreg_debug_knn_direct_stats(st, 1))
        check(L.pcreg_debug_set(b"knn_direct_stats", 0))
        out[name] = {"ms_by_key": res, "direct_stats": [int(v) for v in st]}
    pm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
