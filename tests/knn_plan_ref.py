"""The partition of a query block's visit plan over the candidate kernel's workgroups ("The visit plan").

knn_plan_kernel lists, per block of 512 query slots, the `n_vis` tiles the culling rule cannot skip, in ascending order.  The
candidate kernel's grid keeps W workgroups per block; `live_workgroups` of them walk the list, workgroup w taking the
positions w, w + W_eff, w + 2 W_eff, ..., and the others leave at once.  C is the tiles-per-workgroup target
(PCREG_PLAN_C in knn_mfma16.hip)."""
from __future__ import annotations

PLAN_C = 4


def live_workgroups(n_vis: int, W: int, C: int = PLAN_C) -> int:
    """W_eff: 0 for an empty plan, else ceil(n_vis / C) clamped to [1, W]"""
    if n_vis <= 0:
        return 0
    return min(max(-(-n_vis // C), 1), W)


def positions(n_vis: int, W: int, w: int, C: int = PLAN_C) -> range:
    """the plan positions workgroup w of a block walks, in the order it walks them"""
    w_eff = live_workgroups(n_vis, W, C)
    if w >= w_eff:
        return range(0)
    return range(w, n_vis, w_eff)
