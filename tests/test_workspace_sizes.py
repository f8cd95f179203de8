"""The exported workspace-size functions against the answers of an earlier commit (tests/golden/workspace_sizes.json names it).

Callers allocate what these functions return, so a size may never grow unnoticed.  Each workspace has one layout function that
both its size function and its launcher call; this table is what turns a change of any layout into a
visible diff.  The rules held against the recorded values:

  * pcreg_dev_ransac_workspace(n_cap, it): equal below 2049 correspondences, exactly 768 bytes smaller from 2049 on (the recorded
    commit reserved p32 | perm | bkt as one block with 3 x 256 bytes of slack and carved them as three aligned buffers);
    pcreg_dev_ransac_batched_workspace: equal for B > 1, the line above for B == 1;
  * pcreg_dev_get_matches_workspace(Q, M, D): between recorded - hole(Q) and recorded, hole(Q) = align(q * 8) + align(q * 16) with
    q = max(Q, 1) -- a dead slot of the certified SAD search's workspace, visible only where that term is the largest of the tail;
  * every other size function: equal.

The table is never regenerated from the code under test: `python tests/test_workspace_sizes.py <commit>` rewrites it from the
library that is loaded (PCREG_LIB selects another build), which is done once, on a build of the commit it then names.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

N_CAPS = [0, 3, 1024, 1025, 2048, 2049, 3242, 3243, 4095, 4096, 8192, 32558, 100000]
ITERS = [1, 1000, 2000, 10000]
QS = [0, 1, 1000, 50000]
MS = [0, 1, 16383, 16384, 200000, 1000000]


def shapes():
    """function name -> list of argument tuples (the bench's shapes, the class boundaries, a few batches)"""
    s = {}
    s["pcreg_dev_ransac_workspace"] = [(n, it) for n in N_CAPS for it in ITERS]
    s["pcreg_dev_ransac_batched_workspace"] = [(n, it, B) for n in N_CAPS for it in (1000, 10000) for B in (1, 4, 64, 329)]
    s["pcreg_dev_model_search_workspace"] = [(Q, M) for Q in QS for M in MS]
    s["pcreg_dev_model_knn_workspace"] = [(Q, M, k) for Q in QS for M in (0, 1, 1000000) for k in (1, 8, 32)]
    s["pcreg_dev_knn2_points_f32_workspace"] = [(Q, M) for Q in QS + [3000] for M in MS + [20000]]
    s["pcreg_dev_sphere_select_workspace"] = [(V,) for V in (0, 1, 255, 256, 257, 1533, 60000, 1000000)]
    s["pcreg_dev_spatial_histogram_descriptors_workspace"] = [(P, S) for P in (0, 1, 60000, 1000000) for S in (0, 1, 255, 256, 1533, 50000, 1000000)]
    s["pcreg_dev_get_matches_workspace"] = ([(50000, 200000, 981), (1533, 60000, 980), (2000, 2000, 980), (50000, 50000, 980)] +
                                            [(Q, M, D) for Q in (0, 1, 128, 129, 5000) for M in (0, 1, 300, 70000) for D in (1, 3, 64, 65, 980)])
    # (Q, VM, D, S, total_rows, max_rows): the sweep, a few batches, shapes past the one-chain budget (the batched form's head)
    s["pcreg_dev_get_matches_segmented_workspace"] = [(1533, 60000, 980, 329, 329 * 1800, 2500), (1533, 60000, 980, 329, 0, 0),
                                                      (0, 0, 980, 0, 0, 0), (1, 1, 1, 1, 1, 1), (2000, 60000, 980, 4, 8000, 2000),
                                                      (2000, 60000, 980, 64, 128000, 2000), (6000, 400000, 980, 2000, 2000 * 6000, 6000),
                                                      (3000, 200000, 980, 329, 329 * 4000, 5000), (6000, 400000, 33, 2000, 2000 * 6000, 6000)]
    return s


def measure():
    from pcreg_amd import _lib
    L = _lib.lib()
    return {name: [list(a) + [int(getattr(L, name)(*a))] for a in args] for name, args in shapes().items()}


def _align(x, a=256):
    return (x + a - 1) // a * a


def _ransac_rule(n_cap, single):
    return -768 if single and n_cap >= 2049 else 0


def test_workspace_sizes_against_the_recorded_commit():
    gold = json.load(open(GOLDEN))
    assert gold["commit"], "the table names the commit it was recorded from"
    rec, now = gold["sizes"], measure()
    assert sorted(rec) == sorted(now), "a size function appeared or went: record the table anew, on purpose"
    bad = []
    for name, rows in now.items():
        assert [r[:-1] for r in rows] == [r[:-1] for r in rec[name]], f"{name}: the grid of shapes differs from the recorded one"
        for row, old_row in zip(rows, rec[name]):
            args, new, old = row[:-1], row[-1], old_row[-1]
            if name == "pcreg_dev_ransac_workspace":
                ok = new == old + _ransac_rule(args[0], True)
            elif name == "pcreg_dev_ransac_batched_workspace":
                ok = new == old + _ransac_rule(args[0], args[2] == 1)
            elif name == "pcreg_dev_get_matches_workspace":
                q = max(args[0], 1)
                ok = old - (_align(q * 8) + _align(q * 16)) <= new <= old
            else:
                ok = new == old
            if not ok:
                bad.append((name, args, old, new))
    assert not bad, bad


def test_the_grid_holds_the_shapes_the_table_exists_for():
    s = shapes()
    assert (32558, 10000) in s["pcreg_dev_ransac_workspace"] and (50000, 1000000) in s["pcreg_dev_model_search_workspace"]
    assert (50000, 200000, 981) in s["pcreg_dev_get_matches_workspace"] and (1000000, 1000000) in s["pcreg_dev_spatial_histogram_descriptors_workspace"]
    assert s["pcreg_dev_get_matches_segmented_workspace"][0][:4] == (1533, 60000, 980, 329)
    assert {0, 3, 1024, 1025, 2048, 2049, 3242, 3243, 4095, 4096, 8192} <= {a[0] for a in s["pcreg_dev_ransac_workspace"]}
    assert {4, 64, 329} <= {a[2] for a in s["pcreg_dev_ransac_batched_workspace"]}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if len(sys.argv) != 2:
        sys.exit("usage: test_workspace_sizes.py <commit the loaded library was built from>")
    with open(GOLDEN, "w") as f:
        json.dump({"commit": sys.argv[1], "sizes": measure()}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN)
