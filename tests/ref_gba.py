"""NumPy statements for the GlobalBundleAdjustment tests: the scenes, the symbolic work of the
sparse Schur plan (block pattern of S, minimum-degree order, fill by a dense boolean
elimination, the level rule, the figures of the plan's info) and the map-point correction of
LoopClosing::RunGlobalBundleAdjustment.  The numeric reference is tests/ref_optim.py, unchanged:
a global BA has LocalBundleAdjustment's edge types and LM, only more free poses.
"""
import numpy as np

import ref_optim as R

# Optimizer.cc:157-158: thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815), stored as float
DELTA_MONO_GBA = float(np.float32(np.sqrt(5.99)))
DELTA_STEREO_GBA = float(np.float32(np.sqrt(7.815)))


# --------------------------------------------------------------------------- scenes
def gba_scene(n_kf, n_points, band, loops=(), stereo_frac=0.6, robust=True, seed=0, noise=0.5,
              s_pose=2e-3, s_point=5e-2, islands=1, fixed=(0,)):
    """Keyframes along a path (1.5 m apart, small rotations); point j is anchored at keyframe
    j % n_kf, lies 8 .. 40 m in front of it and is observed by the keyframes within `band` of
    its anchor (within the anchor's island: `islands` splits the path into parts that share no
    point).  loops = ((a, b, count), ...) adds `count` points in front of keyframe max(a, b)
    seen by a and b alone.  Observations are float-exact (cv::KeyPoint), noise in pixels; the
    free poses' translations and the points start s_pose / s_point off the truth.  Returns
    (poses, points, edges) in orb_slam2_test_amd._lib's record types, edges in point order."""
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd import synthetic as S
    rng = np.random.default_rng(seed)
    poses = np.zeros(n_kf, L.POSE_DTYPE)
    cams = []
    for i in range(n_kf):
        a = rng.normal(size=3)
        q = S._quat_from_axis_angle(a, rng.uniform(0, 0.1))
        Rcw = R.quat_to_rot(np.asarray(q))
        center = np.array([rng.normal(0, 0.5), rng.normal(0, 0.1), 1.5 * i])
        poses["q"][i], poses["t"][i] = q, -Rcw @ center
        poses["fixed"][i] = 1 if i in fixed else 0
        cams.append((Rcw, -Rcw @ center))
    per = -(-n_kf // islands)
    seen, pts = [], []
    for j in range(n_points):
        a = j % n_kf
        lo, hi = max(a - band, a // per * per), min(a + band, min(n_kf, (a // per + 1) * per) - 1)
        seen.append((a, list(range(lo, hi + 1))))
    for a, b, count in loops:
        seen += [(max(a, b), [min(a, b), max(a, b)])] * count
    inv_sigma2 = [1.0 / float(np.float32(np.float32(1.2) ** (2 * l))) for l in range(8)]
    edges = []
    for j, (a, kfs) in enumerate(seen):
        Rcw, t = cams[a]
        depth = rng.uniform(8, 40) + 1.5 * (max(kfs) - a)     # in front of its last observer too
        xc = np.array([rng.uniform(-0.4, 0.4) * depth, rng.uniform(-0.15, 0.15) * depth, depth])
        pts.append(Rcw.T @ (xc - t))
        for i in kfs:
            Rcw, t = cams[i]
            xc = Rcw @ pts[j] + t
            assert xc[2] > 1.0
            e = np.zeros((), L.EDGE_DTYPE)
            e["point"], e["pose"] = j, i
            e["inv_sigma2"] = float(np.float32(inv_sigma2[int(rng.integers(0, 8))]))
            e["fx"], e["fy"], e["cx"], e["cy"], e["bf"] = R.CAM
            u = R.CAM[0] * xc[0] / xc[2] + R.CAM[2]
            v = R.CAM[1] * xc[1] / xc[2] + R.CAM[3]
            nz = rng.normal(0, noise, 3)
            stereo = rng.random() < stereo_frac
            e["obs"][0] = float(np.float32(u + nz[0]))
            e["obs"][1] = float(np.float32(v + nz[1]))
            if stereo:
                e["stereo"] = 1
                e["obs"][2] = float(np.float32(u - R.CAM[4] / xc[2] + nz[2]))
            e["huber_delta"] = DELTA_STEREO_GBA if stereo else DELTA_MONO_GBA
            e["robust"] = 1 if robust else 0
            e["active"] = 1
            edges.append(e)
    pts = np.array(pts)
    free = poses["fixed"] == 0
    poses["t"][free] += rng.normal(0, s_pose, (int(free.sum()), 3))
    return poses, pts + rng.normal(0, s_point, pts.shape), np.array(edges, dtype=L.EDGE_DTYPE)


# The smallest scenes at which each part of the sparse solve can still go wrong.
def two_kf_mono(**kw):
    """CreateInitialMapMonocular's call: one free pose, mono only, the scale is free gauge."""
    return gba_scene(2, 80, 1, stereo_frac=0.0, seed=11, **kw)


def ring12(**kw):
    """Band 1 plus one loop: S is a cycle, so L has fill and the graph is not a tree.  Stereo
    only: a chain held by one fixed pose and partly mono points is so weakly conditioned that
    the reference's own estimates move by 5e-10 with the order of its sums."""
    return gba_scene(12, 180, 1, loops=((1, 11, 2),), stereo_frac=1.0, seed=12, **kw)


def clique14(**kw):
    """14 mutually covisible keyframes: 13 columns, every block present, update lists of up to
    12 entries (more than the kernels' staging batch of 8) and one column per level."""
    return gba_scene(14, 140, 14, seed=13, **kw)


def two_islands(**kw):
    """Two components with no shared point: the elimination tree is a forest.  The second has
    no fixed pose; stereo only, for ring12's reason."""
    return gba_scene(16, 240, 2, islands=2, stereo_frac=1.0, seed=14, **kw)


def band40(**kw):
    """40 keyframes, band 3, two loops: several levels with many columns."""
    return gba_scene(40, 600, 3, loops=((2, 30, 8), (10, 39, 8)), stereo_frac=0.6, seed=15, **kw)


SCENES = dict(two_kf_mono=two_kf_mono, ring12=ring12, clique14=clique14, two_islands=two_islands,
              band40=band40)


def with_lone_pose(scene):
    """+ a free pose without any edge."""
    poses, pts, edges = scene
    lone = poses[-1:].copy()
    lone["fixed"] = 0
    return np.concatenate([poses, lone]), pts, edges


def with_lone_point(scene):
    """+ a point without any edge."""
    poses, pts, edges = scene
    return poses, np.concatenate([pts, pts[:1] + 1.0]), edges


def with_fixed(scene, fixed):
    """The fixed poses replaced by `fixed`."""
    poses, pts, edges = scene
    poses = poses.copy()
    poses["fixed"] = 0
    poses["fixed"][list(fixed)] = 1
    return poses, pts, edges


def third_inactive(scene, need_pair=True):
    """Every third edge inactive, from the first of the three phases at which a covisibility
    pair (a block of S) disappears: the plan that set_active rebuilds has another pattern.
    Without need_pair, a scene where no phase removes a pair gets phase 0."""
    poses, pts, edges = scene
    full = s_pattern(edges, len(poses), poses["fixed"])[1].sum()
    for phase in range(3):
        e = edges.copy()
        e["active"][phase::3] = 0
        if s_pattern(e, len(poses), poses["fixed"])[1].sum() < full:
            return e["active"].astype(np.uint8)
    assert not need_pair, "no covisibility pair rests on a third of the edges"
    e = edges.copy()
    e["active"][::3] = 0
    return e["active"].astype(np.uint8)


def variants(name):
    """The scene and its variants: a pose without any edge, a point without any edge, a fixed
    pose that is not index 0, a second fixed pose, one third of the edges inactive.  Yields
    (label, poses, points, edges)."""
    sc = SCENES[name]()
    n = len(sc[0])
    yield (name,) + sc
    yield (name + "+lone_pose",) + with_lone_pose(sc)
    yield (name + "+lone_point",) + with_lone_point(sc)
    yield (name + "+fixed_last",) + with_fixed(sc, (n - 1,))
    yield (name + "+two_fixed",) + with_fixed(sc, (0, n // 2))
    e = sc[2].copy()
    e["active"] = third_inactive(sc, need_pair=False)
    yield (name + "+third_inactive", sc[0], sc[1], e)


# LM cases: every scene at the reference's two calls (CreateInitialMapMonocular: 20 iterations,
# robust; RunGlobalBundleAdjustment: 10, not robust), and one start far enough off that the LM
# rejects trials.  label -> (scene factory, iterations)
LM_CASES = {}
for _n, _f in SCENES.items():
    LM_CASES[_n + "/robust20"] = (lambda f=_f: f(robust=True), 20)
    LM_CASES[_n + "/plain10"] = (lambda f=_f: f(robust=False), 10)
LM_CASES["clique14/far"] = (lambda: clique14(robust=True, s_pose=0.1, s_point=2.0), 10)


def permuted(poses, pts, edges, seed=1):
    """The same problem with its vertices renumbered at random and its edges shuffled: every
    sum of the reference then runs in another order.  Returns ((poses, pts, edges), (pose
    permutation, point permutation)): new vertex k is old vertex perm[k]."""
    rng = np.random.default_rng(seed)
    pp, pq = rng.permutation(len(poses)), rng.permutation(len(pts))
    ip, iq = np.argsort(pp), np.argsort(pq)
    e = edges[rng.permutation(len(edges))].copy()
    e["pose"], e["point"] = ip[e["pose"]], iq[e["point"]]
    return (poses[pp], pts[pq], e), (pp, pq)


# --------------------------------------------------------------------------- symbolic
def s_pattern(edges, npose, fixed):
    """(free poses, A): A[i1, i2] is True when free poses i1 != i2 (free indices) share a point
    through active edges -- the off-diagonal blocks of S."""
    free = np.flatnonzero(np.asarray(fixed) == 0)
    fidx = -np.ones(npose, np.int64)
    fidx[free] = np.arange(len(free))
    act = np.asarray(edges["active"]) != 0
    npt = int(edges["point"].max()) + 1 if len(edges) else 0
    M = np.zeros((npt, len(free)), bool)
    fe = fidx[edges["pose"]]
    ok = act & (fe >= 0)
    M[edges["point"][ok], fe[ok]] = True
    A = (M.T.astype(np.int64) @ M.astype(np.int64)) > 0
    np.fill_diagonal(A, False)
    return free, A


def min_degree_order(A):
    """Elimination order by minimum degree in the graph as it fills, the smallest index among
    the vertices of least degree."""
    A = A.copy()
    left = np.ones(len(A), bool)
    order = []
    for _ in range(len(A)):
        deg = np.where(left, A.sum(1), len(A) + 1)
        v = int(np.argmin(deg))            # the first minimum: the smallest index
        nb = np.flatnonzero(A[v])
        A[np.ix_(nb, nb)] = True
        A[nb, nb] = False
        A[v, :] = A[:, v] = False
        left[v] = False
        order.append(v)
    return np.array(order, np.int64)


def fill_pattern(A, order):
    """The lower-triangular pattern of L (positions, diagonal included) by a dense boolean
    elimination of A under `order`."""
    n = len(order)
    B = A[np.ix_(order, order)].copy()
    np.fill_diagonal(B, True)
    for k in range(n):
        r = np.flatnonzero(B[k + 1:, k]) + k + 1
        B[np.ix_(r, r)] = True
    return np.tril(B)


def pattern_of(colptr, rowidx, n):
    """The boolean lower-triangular matrix of a column-compressed pattern; asserts its form:
    rows ascending, the diagonal first."""
    Lp = np.zeros((n, n), bool)
    for j in range(n):
        r = rowidx[colptr[j]:colptr[j + 1]]
        assert len(r) >= 1 and r[0] == j and np.all(np.diff(r) > 0), (j, r)
        Lp[r, j] = True
    return Lp


def level_rule_holds(Lp, level):
    """Every column's level is greater than the level of every column in its row of L (its
    update lists name a subset of those)."""
    for j in range(len(Lp)):
        k = np.flatnonzero(Lp[j, :j])
        if len(k) and not level[j] > level[k].max():
            return False
    return True


def plan_figures(A, Lp, level):
    """The info a plan reports, from the patterns: blocks of S and of L (lower triangles with
    the diagonals), block updates, levels, columns of the single-column levels at the top."""
    n = len(Lp)
    G = Lp.astype(np.int64)
    strict = np.tril(G, -1)
    # block (r, j), r >= j, takes one update per k < j with L(r, k) and L(j, k)
    common = strict @ strict.T
    updates = int((common * Lp).sum())
    counts = np.bincount(level, minlength=(int(level.max()) + 1) if n else 0)
    tail = 0
    for c in counts[::-1]:
        if c != 1:
            break
        tail += 1
    return dict(nfree=n, s_blocks=int(A.sum()) // 2 + n, l_blocks=int(Lp.sum()), updates=updates,
                levels=len(counts), tail_columns=tail)


def longest_update_list(Lp):
    """The most updates any one block of L takes (the longest list a wave stages)."""
    strict = np.tril(Lp.astype(np.int64), -1)
    return int(((strict @ strict.T) * Lp).max()) if len(Lp) else 0


# --------------------------------------------------------------------------- point correction
def _gemm34(T, x):
    """cv::gemm of a float 3x4 [R | t] with float points: R x + t, each entry's three products
    and t summed in double in order, rounded once."""
    T = np.asarray(T, np.float32).astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.zeros(x.shape)
    for k in range(3):
        s = s + T[:, :, k] * x[:, k:k + 1]
    return (s + T[:, :, 3]).astype(np.float32)


def correct_points(Tcw_before, Twc_after, ref, pts):
    """LoopClosing.cc:1101-1113 for the points global BA did not optimise."""
    ref = np.asarray(ref)
    pts = np.asarray(pts, np.float32)
    out = pts.copy()
    on = (ref >= 0) & (ref < len(Tcw_before))
    r = ref[on]
    xc = _gemm34(np.asarray(Tcw_before)[r][:, :3, :4], pts[on])
    out[on] = _gemm34(np.asarray(Twc_after)[r][:, :3, :4], xc)
    return out
