"""Scenes that drive the rarely taken branches of the descriptor kernel (pcreg_amd/csrc/descriptors.hip), and the host facts
their tests rest on.  Plain numpy in float64: no GPU, no library.

  grid_pick        grid_setup_kernel's cell growth and choice among its seven subdivisions, with the kernel's expressions
  support_sizes    brute-force |p - c| < R counts: with thVar = [1, 1] a surviving row's sum is its support size (minus a cloud
                   point equal to the keypoint, which lies in no bin) -- a check that does not go through the oracle
  select_facts     which way the K-nearest selection goes for a support (crowded bin, tie group kept in part, ...)
  *_scene          cloud, keypoints, options and the facts the GPU test asserts as its premises

The scenes avoid one thing on purpose: a quantity that is zero in exact arithmetic and rounding noise in both implementations
(a frame tilted by 1e-17 turns y == 0 into a coin toss between two phi bins).  Where a scene holds such zeros they are exact in
ANY summation order: dyadic coordinates, symmetric supports."""
import numpy as np

R0 = 3.5
SUBDIVISIONS = [(4, 2, 2), (2, 2, 2), (4, 2, 1), (8, 1, 1), (4, 1, 1), (2, 1, 1), (1, 1, 1)]
MAX_CELLS = 1 << 16
K_SMALL = 256               # keys of the K-th key's bin the selection ranks directly
K_DEF = 128                 # deferred points / votes a keypoint handles one by one
# words of pcreg_debug_desc_stats
SELECT, BISECT, RECOUNT, TIE_RANK, VOTE64, REBIN, LITERAL, RETEST, SUBDIV, DEFERRED = range(10)


def subdiv_word(f):
    return f[0] << 16 | f[1] << 8 | f[2]


def grid_pick(lo, hi, R):
    """-> dict(option, f, cell, h[3], n[3], origin): the grid grid_setup_kernel builds on the box [lo, hi]."""
    ext = [float(hi[c]) - float(lo[c]) for c in range(3)]
    cell = float(R)
    while True:
        n = [np.floor(ext[c] / cell) + 1 for c in range(3)]
        if n[0] * n[1] * n[2] <= float(MAX_CELLS):
            break
        cell *= 1.26
    pick = 6
    for k, f in enumerate(SUBDIVISIONS):
        cnt = 1.0
        for c in range(3):
            cnt *= np.floor(ext[c] * (f[c] / cell)) + 1
        if cnt <= float(MAX_CELLS):
            pick = k
            break
    f = SUBDIVISIONS[pick]
    inv = [f[c] / cell for c in range(3)]
    return dict(option=pick, f=f, cell=cell, h=[cell / f[c] for c in range(3)], n=[int(np.floor(ext[c] * inv[c]) + 1) for c in range(3)],
                origin=[float(lo[c]) for c in range(3)])


def support_sizes(pts, kp, R):
    """#{p : sqrt(dx^2 + dy^2 + dz^2) < R} per keypoint (getLocalPoints.m:23-25, the sum in the reference's order) and how many of
    them EQUAL the keypoint (r = 0: acos(0 / 0) is NaN, the point is in the support and in no bin)."""
    pts, kp = np.asarray(pts, np.float64), np.asarray(kp, np.float64)
    n = np.zeros(len(kp), np.int64); at = np.zeros(len(kp), np.int64)
    for s, c in enumerate(kp):
        d = pts - c
        inside = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < R
        n[s] = inside.sum(); at[s] = (inside & (d == 0).all(axis=1)).sum()
    return n, at


def expected_row_sums(pts, kp, opt):
    """Row sums of the surviving keypoints under thVar = [1, 1] (every keypoint inside the size gates survives), and who survives."""
    n, at = support_sizes(pts, kp, opt["R"])
    k = n if opt["k"] == "all" or opt["k"] >= 1 else np.floor(n * opt["k"] + 0.5)
    alive = (n >= max(opt["min_pts"], 1)) & (n <= opt["max_pts"]) & (k >= 2)
    return (n - at)[alive], alive


def sqrt_threshold(r):
    """the smallest double t with sqrt(t) >= r (r > 0)"""
    t = np.float64(r) * np.float64(r)
    while t > 0 and np.sqrt(t) >= r:
        t = np.nextafter(t, 0.0)
    while np.sqrt(t) < r:
        t = np.nextafter(t, np.inf)
    return t


def select_facts(rel, k):
    """rel: a support relative to its keypoint, in any order.  -> which branches the selection of the K nearest to the centroid
    takes: the kernel's 256-bin histogram over [min, max] of the squared distances, restated with its expressions.  The squared
    distances must be exact (dyadic coordinates, a dyadic centroid) for this to hold whatever the order of the sums."""
    n = len(rel)
    K = int(np.floor(n * k + 0.5))
    g = rel.sum(axis=0) / n
    q = rel - g
    d2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    lo, hi = d2.min(), d2.max()
    scale = 256.0 / (hi - lo) if hi > lo else 0.0
    bin_of = lambda v: np.minimum(((v - lo) * scale).astype(np.int64), 255)
    b = bin_of(d2)
    cum = np.cumsum(np.bincount(b, minlength=256))
    bstar = int(np.searchsorted(cum, K))
    m = int((b == bstar).sum())
    vK = np.sort(d2)[K - 1]
    sK = np.sqrt(vK)
    t_lo, t_hi = sqrt_threshold(sK), sqrt_threshold(np.nextafter(sK, np.inf))
    n_less, n_eq = int((d2 < t_lo).sum()), int(((d2 >= t_lo) & (d2 < t_hi)).sum())
    inside_bin = int(bin_of(np.array([max(t_lo, lo)]))[0]) == bstar and int(bin_of(np.array([min(np.nextafter(t_hi, 0.0), hi)]))[0]) == bstar
    return dict(n=n, K=K, m=m, bisect=m > K_SMALL, recount=m > K_SMALL or not inside_bin, tie_rank=n_eq != K - n_less, n_eq=n_eq,
                all_equal=bool(hi == lo))


# ---- a. the seven grid subdivisions ----------------------------------------------------------------------------------------
# box extents at R = 3.5 (grid_pick confirms the option; tests/test_desc_scene_ref.py asserts it)
GRID_EXTENTS = {0: (60.0, 48.0, 10.0), 1: (150.0, 100.0, 20.0), 2: (0.8, 600.0, 600.0), 3: (0.4, 880.0, 880.0), 4: (600.0, 30.0, 30.0),
                5: (400.0, 100.0, 20.0), 6: (400.0, 200.0, 30.0)}
GRID_OPT = dict(min_pts=10, max_pts=8000, R=R0, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=True, VERBOSE=0)


def _corner_slabs(corner, inward, rng):
    """Three thin slabs (0.004 deep, 0.1 x 0.1 wide, 40 points each) against the three faces that meet in a box corner, the corner
    itself included: what a keypoint on or just outside the box's boundary finds."""
    out = [np.zeros((1, 3))]
    for a in range(3):
        t = rng.uniform(0.0, 0.1, (40, 3))
        t[:, a] = rng.uniform(0.0, 0.004, 40)
        out.append(t)
    return corner + inward * np.vstack(out)


def grid_scene(option, offset=(0.0, 0.0, 0.0), seed=0, n_dense=24000):
    """A strip bundle in the middle of a box whose corners are pinned by two small clusters, sized so that the grid takes
    `option`.  Keypoints: on cell faces in y and z (exactly, one ulp below, one ulp above), at the box's corners and on its faces,
    outside the box by just under and just over R, and generic ones.  -> pts, kp, opt, facts."""
    rng = np.random.default_rng(100 + option + seed)
    E = np.array(GRID_EXTENTS[option]); off = np.asarray(offset, np.float64)
    R = R0
    ns = 8 if E[1] >= 48.0 else 4; per = n_dense // ns; vc = 3.0 * (ns - 1)     # strips 6 apart: a narrow box holds four
    u = rng.uniform(0, 60, (ns, per)); sidx = np.arange(ns)[:, None]
    v = 6 * sidx + rng.uniform(-1.2, 1.2, (ns, per))
    if E[0] < 1.0:                          # a box thin in x: the strips lie in the (y, z) plane, x fills the box
        dense = np.column_stack([rng.uniform(0, E[0], ns * per), u.ravel() + (E[1] / 2 - 30), v.ravel() + (E[2] / 2 - vc)])
    else:
        w = 5 + 0.05 * u * np.sin(sidx) + rng.normal(0, 0.25, (ns, per))
        dense = np.column_stack([u.ravel() + (E[0] / 2 - 30), v.ravel() + (E[1] / 2 - vc), w.ravel() + (E[2] / 2 - 5)])
    lo, hi = np.zeros(3), E.copy()
    pts = np.vstack([dense, _corner_slabs(lo, 1.0, rng), _corner_slabs(hi, -1.0, rng)]) + off
    pts = pts[rng.permutation(len(pts))]
    lo, hi = pts.min(axis=0), pts.max(axis=0)           # what the kernel's bounding box finds
    g = grid_pick(lo, hi, R)
    dlo, dhi = dense.min(axis=0) + off, dense.max(axis=0) + off
    kp, kind = [], []
    # cell faces in y and z inside the dense part: oy + j hy with the kernel's own product and sum
    zmid = off[2] + E[2] / 2                 # (a thick box: the strips' sheets run through the box's middle height)
    for axis in (1, 2):
        if E[0] >= 1.0 and axis == 2:        # the face nearest to the level sheet of strip 0 (at most hz / 2 <= 1.75 away), at three places
            jm = int(np.rint((zmid - lo[2]) / g["h"][2]))
            js = [jm, jm, jm]
        else:
            j0 = int(np.ceil((dlo[axis] - lo[axis]) / g["h"][axis])) + 1
            j1 = int(np.floor((dhi[axis] - lo[axis]) / g["h"][axis])) - 1
            js = sorted(set(np.linspace(j0, j1, 4).astype(int)))
        for t, j in enumerate(js):
            face = lo[axis] + j * g["h"][axis]
            for name, val in (("face", face), ("face-ulp", np.nextafter(face, -np.inf)), ("face+ulp", np.nextafter(face, np.inf))):
                c = dlo + rng.uniform(0.25, 0.75, 3) * (dhi - dlo)
                if E[0] >= 1.0:
                    c[2] = zmid
                    if axis == 2:
                        c[1] = off[1] + E[1] / 2 - vc + rng.uniform(-1.0, 1.0)
                c[axis] = val
                kp.append(c); kind.append(name)
    # the box's corners and faces, and outside it by just under / just over R
    mid = np.array([0.05, 0.05, 0.05])
    for corner, inward in ((lo, 1.0), (hi, -1.0)):
        kp.append(corner.copy()); kind.append("corner")
        for a in range(3):
            c = corner + inward * mid; c[a] = corner[a]
            kp.append(c.copy()); kind.append("on a face")
            c[a] = corner[a] - inward * (R - 0.006)
            kp.append(c.copy()); kind.append("outside, under R")
            c[a] = corner[a] - inward * (R + 0.006)
            kp.append(c.copy()); kind.append("outside, over R")
    # generic positions along the strips
    for _ in range(24):
        kp.append(dlo + rng.uniform(0.0, 1.0, 3) * (dhi - dlo)); kind.append("generic")
    kp = np.array(kp)
    return pts, kp, dict(GRID_OPT), dict(grid=g, kind=kind, subdiv=subdiv_word(g["f"]), lo=lo, hi=hi)


# ---- b. the exact lattice -----------------------------------------------------------------------------------------------
LATTICE_C = np.array([20.0, 10.0, 5.0])
LATTICE_R = 5.5                              # every keypoint below sees the whole lattice: all sums stay dyadic
LATTICE_KP = LATTICE_C + np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.1875, 0.0625, 0.03125]])     # centre, a neighbour, off the lattice (dyadic)


def lattice_scene(seed=0):
    """17^3 points with spacings (0.5, 0.25, 0.125) about a representable centre, rows shuffled.  Every coordinate relative to a
    keypoint is a multiple of 2^-5 below 2^3, so every sum and product the kernel or the oracle forms with k = "all" is exact in
    any order.  For the two keypoints on the plane y = 0: 289 points with y == 0 (> 128 deferred: the literal re-bin and its
    store loop), 17 on the frame's z axis, one at the keypoint; for the centre 289 kept points with a zero vote in x."""
    a = np.arange(-8, 9, dtype=np.float64)
    X, Y, Z = np.meshgrid(a * 0.5, a * 0.25, a * 0.125, indexing="ij")
    pts = np.column_stack([X.ravel(), Y.ravel(), Z.ravel()]) + LATTICE_C
    pts = pts[np.random.default_rng(seed).permutation(len(pts))]
    opt = dict(min_pts=100, max_pts=8000, R=LATTICE_R, thVar=[1.0, 1.0], k="all", ALIGN_POINTS=True, VERBOSE=0)
    return pts, LATTICE_KP.copy(), opt


def shell_scene(seed=0):
    """Supports whose distances to their centroid collide massively.  Keypoint 0: the eight corners of a dyadic box, 40 copies
    each, and nothing else -- 320 equal keys (dhi == dlo, scale = 0), all in bin 0, more than 256: bisection on an empty
    interval, the full recount, and the tie group kept in part.  Keypoint 1: the same shell plus an inner and an outer box of
    8 x 3 points: the shell's 320 keys crowd ONE bin of a histogram that has a range, so the bisection iterates.  Keypoint 2:
    a shell of 8 x 20 = 160 points with the inner and outer box: the crowded bin holds at most 256 keys (ranked directly).
    ALIGN_POINTS is off: a tie group kept in part is cut by original index, the frame tilts."""
    rng = np.random.default_rng(seed)
    sg = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    box = lambda a, copies: np.repeat(sg * np.asarray(a), copies, axis=0)
    c = np.array([[16.0, 8.0, 4.0], [48.0, 8.0, 4.0], [80.0, 8.0, 4.0]])
    parts = [c[0] + box((2.0, 1.0, 0.5), 40),
             c[1] + np.vstack([box((2.0, 1.0, 0.5), 40), box((1.0, 0.5, 0.25), 3), box((2.5, 1.25, 0.625), 3)]),
             c[2] + np.vstack([box((2.0, 1.0, 0.5), 20), box((1.0, 0.5, 0.25), 3), box((2.5, 1.25, 0.625), 3)])]
    pts = np.vstack(parts)
    pts = pts[rng.permutation(len(pts))]
    opt = dict(min_pts=100, max_pts=8000, R=R0, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=False, VERBOSE=0)
    facts = [select_facts(pts[np.sqrt(((pts - ci) ** 2).sum(axis=1)) < R0] - ci, 0.85) for ci in c]
    return pts, c, opt, facts


def tie_order_scene(reverse=False):
    """Where WHICH members of a tie group are kept decides a keypoint's fate.  Per keypoint: a core of 200 points (the corners of
    a flat dyadic box, 25 copies each), a tie group of 120 points at distance 2 from the centroid -- 60 on the x axis, 60 on the
    y axis -- and 20 points farther out; k = 0.765 keeps K = 260 = the core and HALF the tie group, the half with the lowest
    original indices (the reference's sort is stable).  Keypoint 0 has its x-axis ties first in the cloud: they are kept, the
    kept set is elongated (variance ratios 35 and 4) and passes thVar = [3, 1.5].  Keypoint 1 has its y-axis ties first: ratio
    1.26, rejected.  Keeping the highest indices instead swaps the two.  ALIGN_POINTS off: the histogram does not depend on
    the frame.  reverse: the same cloud in reverse order."""
    sg = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    kp = np.array([[16.0, 8.0, 4.0], [48.0, 8.0, 4.0]])
    xt = np.repeat(np.array([[2.0, 0, 0], [-2.0, 0, 0]]), 30, axis=0)
    yt = np.repeat(np.array([[0, 2.0, 0], [0, -2.0, 0]]), 30, axis=0)
    core = np.repeat(sg * [1.0, 0.25, 0.125], 25, axis=0)
    far = np.repeat(np.array([[3.0, 0.5, 0], [-3.0, 0.5, 0], [3.0, -0.5, 0], [-3.0, -0.5, 0]]), 5, axis=0)
    rng = np.random.default_rng(0)
    mid = np.vstack([kp[0] + core, kp[0] + far, kp[1] + core, kp[1] + far])
    pts = np.vstack([kp[0] + xt, kp[1] + yt, mid[rng.permutation(len(mid))], kp[0] + yt, kp[1] + xt])
    if reverse:
        pts = pts[::-1].copy()
    opt = dict(min_pts=100, max_pts=8000, R=R0, thVar=[3.0, 1.5], k=0.765, ALIGN_POINTS=False, VERBOSE=0)
    return pts, kp, opt


# ---- c. planted bin edges ---------------------------------------------------------------------------------------------
def radial_edges(R):
    """nthroot(0:R^3/10:R^3, 3) with the C library's cbrt, which the oracle and the launcher call (numpy's own differs from it
    by an ulp at one of the eleven edges for R = 3.5)"""
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.cbrt.restype = ctypes.c_double; m.cbrt.argtypes = [ctypes.c_double]
    return np.array([m.cbrt(k * (R * R * R / 10)) for k in range(11)])


def theta_edges():
    return np.array([k * (np.pi / 7) for k in range(8)])                      # 0:pi/7:pi


def _norm(p):
    return np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])       # the reference's order


def _filler(n, R, rng):
    """n generic points well inside 0.9 R, an elongated blob (distinct variances)"""
    out = np.zeros((0, 3))
    while len(out) < n:
        t = rng.uniform(-1, 1, (4 * n, 3))
        out = np.vstack([out, (t[(t ** 2).sum(axis=1) < 1] * [0.85 * R, 0.4 * R, 0.15 * R])])
    return out[:n]


def radial_edge_scene(n_dirs, seed=0):
    """Keypoint at the origin (p - c is p itself, exactly).  Along n_dirs generic directions and for each edge r[1..9] and R,
    points scaled so that the reference's sqrt(x^2 + y^2 + z^2) lands 0, 1, 2, 3 ulps above or below the edge.
    -> pts, kp, opt, facts: per edge the number of planted points on / above / below it (each positive)."""
    rng = np.random.default_rng(seed)
    R = R0
    edges = radial_edges(R)
    planted, cases = [], []
    for e in edges[1:]:
        targets = [e]
        for _ in range(3):
            targets = [np.nextafter(targets[0], 0.0)] + targets + [np.nextafter(targets[-1], np.inf)]
        on = above = below = done = 0
        while done < n_dirs:                                                    # (a direction whose walk misses a target is dropped)
            u = rng.normal(size=3)
            u[1] = np.sign(u[1]) * max(abs(u[1]), 0.2)                          # generic: not screened out as y ~ 0
            u /= np.linalg.norm(u)
            if abs(u[2]) > 0.95:
                continue
            found = []
            for t in targets:
                p = u * t
                w = int(np.argmax(np.abs(p)))
                for _ in range(200):                                            # walk the largest coordinate by ulps until the norm is the target
                    d = _norm(p)
                    if d == t:
                        break
                    p[w] = np.nextafter(p[w], np.inf * np.sign(p[w]) if d < t else 0.0)
                if _norm(p) == t:
                    found.append(p.copy())
            if len(found) == len(targets):
                planted += found; done += 1; on += 1; above += 3; below += 3
        cases.append((int(on), int(above), int(below)))
    planted = np.array(planted)
    pts = np.vstack([planted, _filler(300, R, rng)])
    pts = pts[rng.permutation(len(pts))]
    opt = dict(min_pts=50, max_pts=8000, R=R, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=False, VERBOSE=0)
    return pts, np.zeros((1, 3)), opt, dict(cases=cases, planted=len(planted))


def theta_edge_scene(seed=0):
    """Keypoint at the origin.  For each edge t[1..6], 8 points on either side at a relative offset of 1e-9: inside the fp32
    screen's band (deferred), outside the fp64 images' 1e-12 band (no acos decides).  96 <= 128 deferred points."""
    rng = np.random.default_rng(seed)
    R = R0
    planted = []
    for t in theta_edges()[1:7]:
        for side in (-1.0, 1.0):
            for _ in range(8):
                th = t * (1.0 + side * 1e-9)
                ph = rng.uniform(0.3, 1.2) * rng.choice([-1.0, 1.0]) + rng.choice([0.0, np.pi / 2])      # away from y = 0
                r = rng.choice([0.45, 0.62, 0.77, 0.9]) * R * (1 + rng.uniform(-0.01, 0.01))
                planted.append([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)])
    planted = np.array(planted)
    pts = np.vstack([planted, _filler(300, R, rng)])
    pts = pts[rng.permutation(len(pts))]
    opt = dict(min_pts=50, max_pts=8000, R=R, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=False, VERBOSE=0)
    return pts, np.zeros((1, 3)), opt, dict(planted=len(planted))


def literal_scene(seed=0):
    """Keypoint at the origin, ALIGN_POINTS off: 20 points on the plane y = 0, 5 on the z axis and one at the keypoint among 300
    generic ones.  None of the 26 can be decided by the fp64 images (y == 0, or x = y = 0)."""
    rng = np.random.default_rng(seed)
    R = R0
    plane = np.column_stack([rng.uniform(-0.6 * R, 0.6 * R, 20), np.zeros(20), rng.uniform(-0.5 * R, 0.5 * R, 20)])
    axis = np.column_stack([np.zeros(5), np.zeros(5), np.array([-0.7, -0.3, 0.2, 0.5, 0.8]) * R])
    pts = np.vstack([plane, axis, np.zeros((1, 3)), _filler(300, R, rng)])
    pts = pts[rng.permutation(len(pts))]
    opt = dict(min_pts=50, max_pts=8000, R=R, thVar=[1.0, 1.0], k=0.85, ALIGN_POINTS=False, VERBOSE=0)
    return pts, np.zeros((1, 3)), opt, dict(literal=26)


# ---- d. capacity and size gates -----------------------------------------------------------------------------------------
def ball_scene(sizes, seed=0, R=R0):
    """One elongated blob of exactly sizes[i] points inside 0.95 R of keypoint i; the keypoints are 12 R apart, so everything else
    is beyond 1.5 R.  -> pts (shuffled), kp"""
    rng = np.random.default_rng(seed)
    kp = np.array([[12.0 * R * i, 1.0, 2.0] for i in range(len(sizes))])
    parts = []
    for c, n in zip(kp, sizes):
        out = np.zeros((0, 3))
        while len(out) < n:
            t = rng.uniform(-1, 1, (2 * n + 64, 3))
            out = np.vstack([out, t[(t ** 2).sum(axis=1) < 1] * [0.94 * R, 0.45 * R, 0.2 * R]])
        parts.append(c + out[:n])
    pts = np.vstack(parts)
    return pts[rng.permutation(len(pts))], kp
