"""The reference restatement of [C, ia] = unique(A, 'rows') and of completeExperiment.m:424-458 for the tests: numpy on the host, the
C oracle's ransac and the Python oracle's estimateTransform.  Nothing here calls the library under test."""
import numpy as np


def unique_rows_ref(A):
    """(ia, n_unique): the 0-based index of every run's FIRST occurrence, in sorted row order.  A stable lexsort over (column 3,
    column 2, column 1) orders the rows by column 1, then 2, then 3 and keeps equal rows in their original order (-0 == +0: the
    comparison is numeric); a run starts where any column differs from the row before under `!=`."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 3)
    n = A.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), 0
    order = np.lexsort((A[:, 2], A[:, 1], A[:, 0]))                 # stable; the LAST key is the primary one
    S = A[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (S[1:] != S[:-1]).any(axis=1)
    ia = order[head].astype(np.int64)
    return ia, int(len(ia))


def aggregate_ref(pts1, pts2):
    """completeExperiment.m:440-443 -> (pts1u, pts2u, ia): the surviving pairs (sorted by pts2u) and their 0-based rows in the input."""
    pts1 = np.asarray(pts1, dtype=np.float64).reshape(-1, 3)
    pts2 = np.asarray(pts2, dtype=np.float64).reshape(-1, 3)
    ia1, _ = unique_rows_ref(pts1)                                   # [pts1_agg, ia, ic] = unique(pts1_agg, 'rows');
    p1, p2 = pts1[ia1], pts2[ia1]                                    # pts2_agg = pts2_agg(ia, :);
    ia2, _ = unique_rows_ref(p2)                                     # [pts2_agg, ia, ~] = unique(pts2_agg, 'rows');
    return p1[ia2], p2[ia2], ia1[ia2]                                # pts1_agg = pts1_agg(ia, :);


def stack_ref(result, members, featS, featM):
    """:424-437: the putative matches of the spheres `members` (indices into result["centres"]), in that order, pairs in each
    sphere's own order.  matches are 1-based (surface keypoint, row of the sphere's model_rows)."""
    p1, p2 = [np.zeros((0, 3))], [np.zeros((0, 3))]
    for i in members:
        m = np.asarray(result["matches"][i], dtype=np.int64).reshape(-1, 2)
        rows = np.asarray(result["model_rows"][i], dtype=np.int64)
        p1.append(np.asarray(featS, dtype=np.float64)[m[:, 0] - 1])
        p2.append(np.asarray(featM, dtype=np.float64)[rows[m[:, 1] - 1]])
    return np.vstack(p1), np.vstack(p2)


def aggregated_stage_ref(result, members, featS, featM, options, seed=0):
    """:424-458 from a sweep's result dict: stack, unique twice, ONE ransac (the oracle's, built-in sampler), estimateTransform
    over its inliers."""
    from oracle import c_oracle
    from oracle.pcreg_oracle import estimateTransform
    a1, a2 = stack_ref(result, members, featS, featM)
    ia1, n1 = unique_rows_ref(a1)
    p1, p2, ia = aggregate_ref(a1, a2)
    out = dict(n_total=len(a1), n_unique1=n1, n_unique2=len(p1), pts1=p1, pts2=p2, ia=ia, T=None, inlierIdx=np.zeros(0, np.int64),
               numSuccess=0, maxInliers=0, T_final=None)
    if len(p1) == 0:
        return out
    r = c_oracle.ransac(p1, p2, options, seed=seed)
    out.update(T=r["T"], inlierIdx=r["inlierIdx"], numSuccess=r["numSuccess"], maxInliers=r["maxInliers"])
    if not r["failed"]:
        inl = r["inlierIdx"] - 1
        out["T_final"] = estimateTransform(p1[inl], p2[inl])
    return out
