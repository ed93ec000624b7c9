"""Scenes for the KeyFrame-side matchers: test_kf_matching_ref.py (CPU) and
test_gpu_kf_matching_ref.py.

A scene is a dict of host arrays for one call of SearchByBoW KeyFrame-Frame ("bow"),
KeyFrame-KeyFrame ("bowkf"), SearchForTriangulation ("tri"), the two Fuse forms ("fuse",
"fuse_sim3") or SearchBySim3 ("sim3").  The FeatureVector family is built node by node, so a
candidate's position in its node (the lane and 64-chunk a kernel holds it in) is designed, and
feature indices are permuted so position and index never coincide.  The grid family places
keypoints and projections at exact float32 coordinates (FX = FY = 512, power-of-two depths,
identity poses) on the cell, window, image, distance, level and chi-square boundaries.
filtered() asks ref_kf_matching for its float margins and removes what an ambiguous decision
names (a whole node in the two BoW forms, whose walk is order dependent; the query alone
elsewhere) until none is left, at most DROP_CAP of a scene; the comparison with the oracle or
the kernels is then exact.
"""
import numpy as np

import ref_kf_matching as R
from matching_scenes import (BF, CX, CY, DROP_CAP, FX, FY, HISTS, IMG, KP_DTYPE, flip, pose)

MAPPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"),
                           ("ny", "<f4"), ("nz", "<f4"), ("min_dist", "<f4"),
                           ("max_dist", "<f4"), ("flags", "<i4")])
FRUSTUM_DTYPE = np.dtype([("Tcw", "<f4", 12), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                          ("cy", "<f4"), ("bf", "<f4"), ("log_scale_factor", "<f4"),
                          ("nlevels", "<i4"), ("min_x", "<f4"), ("max_x", "<f4"),
                          ("min_y", "<f4"), ("max_y", "<f4")])
SIM3_PAIR_DTYPE = np.dtype([("T1w", "<f4", 12), ("T2w", "<f4", 12), ("R12", "<f4", 9),
                            ("t12", "<f4", 3), ("s12", "<f4"), ("fx", "<f4"), ("fy", "<f4"),
                            ("cx", "<f4"), ("cy", "<f4"), ("log_scale_factor", "<f4"),
                            ("nlevels", "<i4"), ("min_x", "<f4"), ("max_x", "<f4"),
                            ("min_y", "<f4"), ("max_y", "<f4")])
TRI_GEOM_DTYPE = np.dtype([("F12", "<f4", 9), ("Cw1", "<f4", 3), ("Tcw2", "<f4", 12),
                           ("fx2", "<f4"), ("fy2", "<f4"), ("cx2", "<f4"), ("cy2", "<f4")])
SF, SIGMA2, INV_SIGMA2 = R.level_tables(1.2, 8)
LOG_SF = float(np.float32(np.log(np.float32(1.2))))   # mfLogScaleFactor = log(mfScaleFactor)
TUM1 = (10.80118465423584, 1230.0478515625, 14.668615341186523, 370.3119896484375)
POW2 = (0.0, 512.0, 0.0, 384.0)      # 64 / 512 and 48 / 384 are exact: grid positions too
F_ROWS = (0, 0, 0, 0, 0, -1, 0, 1, 0)   # F12 of a sideways motion: the line of (x1, y1) is y = y1


# ================================================================ the FeatureVector family
class FV:
    """Two sides of features grouped in nodes.  Side 0 is walked (the KeyFrame / pKF1), side 1
    holds the candidates (the Frame / pKF2).  ok = the guard of the loop passes (a good
    MapPoint in the BoW forms, no MapPoint in the triangulation search)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.f = ([], [])
        self.nodes = {}
        self.next_node = 10

    def rand(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def near(self, d, k):
        return flip(self.rng, d, k)

    def node(self, step=3):
        self.next_node += step
        return self.next_node

    def add(self, side, node, desc, ok=True, angle=0.0, x=None, y=100.0, octave=0, uright=1.0):
        if x is None:
            x = 20.0 + 0.25 * (len(self.f[side]) % 2000)
        self.f[side].append(dict(desc=np.asarray(desc, np.uint8), ok=ok, angle=angle, x=x, y=y,
                                 octave=octave, uright=uright))
        self.nodes.setdefault(node, ([], []))[side].append(len(self.f[side]) - 1)
        return len(self.f[side]) - 1

    def fill(self, side, node, n):
        """n unrelated features (random descriptors, about 128 bits from anything)."""
        for _ in range(n):
            self.add(side, node, self.rand())

    def side(self, s):
        n = len(self.f[s])
        perm = self.rng.permutation(n)
        kps = np.zeros(n, KP_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        ok = np.zeros(n, np.uint8)
        ur = np.zeros(n, np.float32)
        for j, f in enumerate(self.f[s]):
            i = perm[j]
            desc[i], ok[i], ur[i] = f["desc"], f["ok"], f["uright"]
            kps["x"][i], kps["y"][i], kps["octave"][i], kps["angle"][i] = (f["x"], f["y"],
                                                                         f["octave"], f["angle"])
        kps["size"] = 31
        ids = sorted(k for k, v in self.nodes.items() if v[s])
        off = np.zeros(len(ids) + 1, np.int32)
        feats = []
        for k, nid in enumerate(ids):
            feats += [perm[j] for j in self.nodes[nid][s]]
            off[k + 1] = len(feats)
        return dict(kps=kps, desc=desc, ok=ok, uright=ur,
                    fv=(np.asarray(ids, np.int32), off, np.asarray(feats, np.int32)))

    def scene(self, kind, nnratio=0.75, ori=False, only_stereo=False, geom=None):
        return dict(kind=kind, s1=self.side(0), s2=self.side(1), nnratio=nnratio, ori=ori,
                    only_stereo=only_stereo, geom=tri_geom() if geom is None else geom)


def tri_geom(F=F_ROWS, Cw1=(-8.0, -8.0, 1.0)):
    """F12 and the epipole of Cw1 under an identity pKF2 pose: (512 x / z + 320, 512 y / z +
    240), far outside the image by default."""
    g = np.zeros((), TRI_GEOM_DTYPE)
    g["F12"], g["Cw1"], g["Tcw2"] = F, Cw1, pose().reshape(-1)
    g["fx2"], g["fy2"], g["cx2"], g["cy2"] = FX, FY, CX, CY
    return g


def fv_chunks(kind, seed=21):
    """Candidate node sizes around the 64-chunks; one walker per chunk, its match planted at
    the chunk's last position."""
    b = FV(seed)
    for size in (1, 63, 64, 65, 127, 128, 129, 192, 193):
        nid = b.node()
        ends = sorted({min(64 * c + 63, size - 1) for c in range((size + 63) // 64)})
        W = [b.rand() for _ in ends]
        for w in W:
            b.add(0, nid, w)
        for pos in range(size):
            b.add(1, nid, b.near(W[ends.index(pos)], 7 + ends.index(pos)) if pos in ends
                  else b.rand())
    return b.scene(kind)


def fv_ties(kind, seed=22):
    """A distance tie between position 63 and position 64 (BoW keeps the first - observable
    with nnratio 2, since a tied second fails every ratio below 1 - triangulation the last),
    ties inside a chunk, and a tie of three."""
    b = FV(seed)
    for size, tied in ((130, (63, 64)), (130, (5, 40)), (200, (127, 128)), (200, (3, 63, 64, 191))):
        nid = b.node()
        w = b.rand()
        b.add(0, nid, w)
        for pos in range(size):
            b.add(1, nid, b.near(w, 10) if pos in tied else b.rand())
    return b.scene(kind, nnratio=2.0)


def fv_second(kind, seed=23):
    """Best and second best in the same lane of different chunks (p, p + 64), in different
    lanes of one chunk, and a second equal to the best; each once with a ratio that passes
    and once with one that fails."""
    b = FV(seed)
    for pb, ps in ((5, 69), (69, 5), (70, 134), (5, 9), (100, 70), (130, 2)):
        for d2 in (20, 12, 10):
            nid = b.node()
            w = b.rand()
            b.add(0, nid, w)
            for pos in range(140):
                b.add(1, nid, b.near(w, 10) if pos == pb else b.near(w, d2) if pos == ps
                      else b.rand())
    return b.scene(kind)


def fv_walk(kind, seed=24):
    """Walked node sizes 1, 64, 65, 129: the features at batch positions 0, 63 and 64 fail the
    guard although a candidate sits right next to them; the node's last feature matches."""
    b = FV(seed)
    for size in (1, 64, 65, 129):
        nid = b.node()
        for pos in range(size):
            w = b.rand()
            last = pos == size - 1
            b.add(0, nid, w, ok=last or pos not in (0, 63, 64))
            if last or pos in (0, 63, 64):
                b.add(1, nid, b.near(w, 6))
        b.fill(1, nid, 3)
    return b.scene(kind)


def fv_shared(kind, seed=25):
    """Two and three walked features of a node with the same nearest candidate S, placed in
    chunk 0, 1 and 2: in the BoW forms the second takes its next candidate and the third
    fails the ratio; the triangulation search gives S to all three."""
    b = FV(seed)
    for chunk in (0, 1, 2):
        for walkers in (2, 3):
            nid = b.node()
            D = b.rand()
            W = [b.near(D, 5), b.near(D, 6), b.near(D, 7)][:walkers]
            for w in W:
                b.add(0, nid, w)
            plant = {64 * chunk + 7: D, 64 * ((chunk + 1) % 3) + 11: b.near(W[1], 20)}
            if walkers == 3:
                plant[64 * ((chunk + 2) % 3) + 1] = b.near(W[2], 30)
                plant[64 * chunk + 30] = b.near(W[2], 32)
            for pos in range(150):
                b.add(1, nid, plant[pos] if pos in plant else b.rand())
    return b.scene(kind)


def fv_invalid(kind, seed=26):
    """Candidates failing their guard in each of the three chunks, one of them the nearest."""
    b = FV(seed)
    for near_chunk in (0, 1, 2):
        nid = b.node()
        w = b.rand()
        b.add(0, nid, w)
        bad = (3, 70, 135)
        for pos in range(140):
            if pos in bad:
                b.add(1, nid, b.near(w, 2) if pos == bad[near_chunk] else b.near(w, 30), ok=False)
            else:
                b.add(1, nid, b.near(w, 10) if pos == 20 + 40 * near_chunk else b.rand())
    return b.scene(kind)


def fv_thresholds(kind, nnratio, seed=27):
    """Best distances 49, 50, 51 with a far second; the ratio on, below and above equality."""
    b = FV(seed)
    for d in (49, 50, 51):
        nid = b.node()
        w = b.rand()
        b.add(0, nid, w)
        b.add(1, nid, b.rand())
        b.add(1, nid, b.near(w, d))
    eq = 30 if nnratio == 0.75 else 20
    for d in (eq, eq - 1, eq + 1):
        for first in (0, 1):
            nid = b.node()
            w = b.rand()
            b.add(0, nid, w)
            c = [b.near(w, d), b.near(w, 40)]
            b.add(1, nid, c[first])
            b.add(1, nid, c[1 - first])
    return b.scene(kind, nnratio=nnratio)


def fv_join(kind, n_nodes, seed=28):
    """n_nodes walked nodes of one feature; the common ones are the first and last node of
    every pass of 1024, which are also the first and last id of the other side's list; ids
    on one side only lie between them."""
    b = FV(seed + n_nodes)
    common = sorted({0, n_nodes - 1} | {k for k in range(n_nodes)
                                        if k % 1024 in (0, 1023)})
    for k in range(n_nodes):
        nid = 2 * k + 2
        w = b.rand()
        b.add(0, nid, w, x=20.0 + 0.25 * (k % 2000))
        if k in common:
            b.add(1, nid, b.rand())
            b.add(1, nid, b.near(w, 8))
    for k in range(1, n_nodes - 1, max(1, n_nodes // 12)):
        b.fill(1, 2 * k + 3, 1)                     # odd ids: on the other side only
    return b.scene(kind)


def fv_rotation(kind, hist, seed=29):
    """One match per node; hist = [(bin, count)]: rot = 30 * bin + (-8 .. 8) degrees."""
    b = FV(seed)
    for bn, cnt in hist:
        for _ in range(cnt):
            nid = b.node()
            w = b.rand()
            a2 = float(np.float32(b.rng.uniform(0, 360)))
            a1 = float(np.float32((a2 + 30.0 * bn + float(b.rng.uniform(-8, 8))) % 360))
            b.add(0, nid, w, angle=a1)
            b.add(1, nid, b.near(w, 3), angle=a2)
            b.add(1, nid, b.rand(), angle=a2)
    return b.scene(kind, ori=True)


def fv_random(kind, seed, n=500, nnodes=40, ori=True):
    """A generated pair: features spread over nnodes nodes, two thirds with a counterpart a few
    bits away, guards failing at random, angles at random (the rotation filter bites)."""
    b = FV(seed)
    rng = b.rng
    for _ in range(n):
        nid = 5 * int(rng.integers(nnodes))
        w = b.rand()
        rot = float(rng.choice([0.0, 0.0, 0.0, 33.0, 95.0])) + float(rng.uniform(-9, 9))
        a2 = float(rng.uniform(0, 360))
        x, y = float(rng.integers(30, 600)), float(rng.integers(30, 440))
        u = rng.random()
        if u < 0.85:
            b.add(0, nid, w, ok=rng.random() < 0.8, angle=(a2 + rot) % 360, x=x, y=y,
                  octave=int(rng.integers(8)), uright=float(rng.choice([-1.0, 0.0, x - 7.0])))
        if u > 0.2:
            b.add(1, nid + (3 if rng.random() < 0.1 else 0), b.near(w, int(rng.integers(0, 70))),
                  ok=rng.random() < 0.8, angle=a2, x=x + float(rng.integers(-30, 30)),
                  y=y + float(rng.integers(-4, 5)) * 0.5, octave=int(rng.integers(8)),
                  uright=float(rng.choice([-1.0, 0.0, x - 7.0])))
    return b.scene(kind, ori=ori, geom=tri_geom(Cw1=(0.25, 0.125, 1.0)))


def tri_geometry(only_stereo, seed=31):
    """The triangulation search's own rules, each group in a node of its own.  Epipole at
    (320, 240); the line of a KF1 feature at (x1, y1) is y = y1."""
    b = FV(seed)

    def group(kp1, cands, **kw1):
        nid = b.node()
        w = b.rand()
        b.add(0, nid, w, x=kp1[0], y=kp1[1], uright=kp1[2], **kw1)
        for x, y, ur, octv, d in cands:
            b.add(1, nid, b.near(w, d), x=x, y=y, uright=ur, octave=octv)
    # mono - mono: on, inside and outside the epipole radius 100 * scale (octave 0: 100;
    # octave 7: 358.318): the nearer candidate is the one inside
    for octv, pts in ((0, ((6, 8, 0), (6, 7, 1), (6, 9, 0))), (7, ((18, 5, 1), (18, 6, 0)))):
        for dx, dy, inside in pts:
            for ur1 in (-1.0, 0.0, 5.0):       # mono, stereo by uRight == 0, stereo
                group((100.0, CY + dy, ur1),
                      [(CX + dx, CY + dy, -1.0, octv, 5), (CX + 60.0, CY + dy, -1.0, octv, 20)])
            group((100.0, CY + dy, -1.0), [(CX + dx, CY + dy, 3.0, octv, 5)])   # stereo KF2
    # the epipolar distance on either side of 3.84 * sigma2 (octave 0: 3.84; 7: 49.30)
    for octv, dys in ((0, (1.5, 2.0, -1.5, -2.0)), (7, (7.0, 7.25, -7.0, -7.25))):
        for dy in dys:
            group((100.0, 100.0, 5.0), [(50.0, 100.0 + dy, 5.0, octv, 5),
                                        (60.0, 100.0, 5.0, octv, 20)])
    # bOnlyStereo: mono on either side
    group((100.0, 50.0, -1.0), [(50.0, 50.0, 5.0, 0, 5)])
    group((100.0, 50.0, 5.0), [(50.0, 50.0, -1.0, 0, 5), (55.0, 50.0, 5.0, 0, 30)])
    group((100.0, 50.0, 0.0), [(50.0, 50.0, 0.0, 0, 5)])
    # distances 50 and 51; a later equal distance wins; a later larger one does not
    group((100.0, 60.0, 5.0), [(50.0, 60.0, 5.0, 0, 50)])
    group((100.0, 60.0, 5.0), [(50.0, 60.0, 5.0, 0, 51)])
    group((100.0, 60.0, 5.0), [(50.0, 60.0, 5.0, 0, 9), (51.0, 60.0, 5.0, 0, 9),
                               (52.0, 60.0, 5.0, 0, 10), (53.0, 63.0, 5.0, 0, 9)])
    return b.scene("tri", only_stereo=only_stereo, geom=tri_geom(Cw1=(0.0, 0.0, 1.0)))


def tri_degenerate(seed=32):
    """An F12 whose line is (0, y1 - 100, 0): a = b = 0 for the KF1 feature at y1 = 100, which
    therefore matches nothing; for the others dsqr = y2^2."""
    b = FV(seed)
    for y1, y2 in ((100.0, 0.0), (101.0, 1.0), (103.0, 1.5), (97.0, 2.0), (100.0, 1.0)):
        nid = b.node()
        w = b.rand()
        b.add(0, nid, w, x=33.0, y=y1)
        b.add(1, nid, b.near(w, 4), x=70.0, y=y2)
    return b.scene("tri", geom=tri_geom(F=(0, 0, 0, 0, 1, 0, 0, -100, 0)))


# ================================================================ the grid family
def spot(k):
    return 63.25 + 70.0 * (k % 8), 63.25 + 70.0 * (k // 8)


def log_level(v):
    """max_dist / dist3D that puts log(ratio) / log(1.2) at v."""
    return float(np.exp(v * LOG_SF))


class GridDesigner:
    """Queries (map points) at separate spots; each sees only its own keypoints.  Identity
    pose, depth 4: a projection at (u, v) is exact for coordinates in eighths of a pixel.
    cam_scale = |camera-frame point| / |world point| (1 / s12 in SearchBySim3's first
    direction)."""

    def __init__(self, seed, bounds=IMG, cam_scale=1.0):
        self.rng = np.random.default_rng(seed)
        self.bounds, self.cs = bounds, cam_scale
        self.kp, self.q, self.owner = [], [], []
        self.n_spot = 0

    def rand(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def add_kp(self, x, y, octave, desc, uright=-1.0, owner=-1):
        self.kp.append((x, y, octave, np.asarray(desc, np.uint8), uright))
        self.owner.append(owner)
        return len(self.kp) - 1

    def point(self, u, v, members, level=0, lv=None, z=4.0, P=None, min_dist=None,
              max_dist=None, normal=None, flags=1, desc=None):
        """members = (dx, dy, octave, distance[, uRight - ur]).  The point's max_dist puts
        PredictScale at lv (default level - 0.5, a clear margin) unless given."""
        D = self.rand() if desc is None else desc
        ur = u - BF / (z * self.cs)
        for m in members:
            self.add_kp(u + m[0], v + m[1], m[2], flip(self.rng, D, m[3]),
                        ur + m[4] if len(m) > 4 else -1.0, owner=len(self.q))
        if P is None:
            P = ((u - CX) / FX * z, (v - CY) / FY * z, z)
        P32 = np.asarray(P, np.float32).astype(np.float64)
        dist = float(np.sqrt((P32 * P32).sum())) * self.cs
        if max_dist is None:
            max_dist = dist * log_level(level - 0.5 if lv is None else lv)
        if min_dist is None:
            min_dist = 0.25 * min(dist, max_dist)
        if normal is None:
            normal = P32 / max(np.sqrt((P32 * P32).sum()), 1e-30)
        self.q.append(dict(P=P, min_dist=min_dist, max_dist=max_dist, normal=normal, flags=flags,
                           desc=D, uv=(u, v), level=level, members=len(members)))
        return len(self.q) - 1

    def at_spot(self, members, shift=(0.0, 0.0), **kw):
        u, v = spot(self.n_spot)
        self.n_spot += 1
        return self.point(u + shift[0], v + shift[1], members, **kw)

    # ---- arrays
    def keyframe(self, stereo=True):
        n = len(self.kp)
        kps = np.zeros(n, KP_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        ur = np.zeros(n, np.float32)
        for i, (x, y, o, d, r) in enumerate(self.kp):
            kps["x"][i], kps["y"][i], kps["octave"][i], desc[i], ur[i] = x, y, o, d, r
        kps["size"] = 31
        return dict(kps=kps, desc=desc, uright=ur if stereo else None)

    def points(self):
        n = len(self.q)
        mps = np.zeros(n, MAPPOINT_DTYPE)
        md = np.zeros((n, 32), np.uint8)
        for i, q in enumerate(self.q):
            mps["x"][i], mps["y"][i], mps["z"][i] = q["P"]
            mps["nx"][i], mps["ny"][i], mps["nz"][i] = q["normal"]
            mps["min_dist"][i], mps["max_dist"][i], mps["flags"][i] = (q["min_dist"],
                                                                     q["max_dist"], q["flags"])
            md[i] = q["desc"]
        return mps, md


def frustum(bounds, Tcw=None, scale=1.0):
    c = np.zeros((), FRUSTUM_DTYPE)
    T = pose() if Tcw is None else np.asarray(Tcw, np.float32)
    c["Tcw"] = (T * np.float32(scale)).reshape(-1)
    c["fx"], c["fy"], c["cx"], c["cy"], c["bf"] = FX, FY, CX, CY, BF
    c["log_scale_factor"], c["nlevels"] = LOG_SF, 8
    c["min_x"], c["max_x"], c["min_y"], c["max_y"] = bounds
    return c


def next32(v, up=True):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def common_groups(d, r=4.0, gate=50):
    """The rules the three grid searches share (th = 4, so r = 4 at level 0)."""
    # equal distances (a spot shifted by 1 has the cell boundary at 65 between x - 1 and x + 1):
    # the lower column wins although its index is higher, then the lower row; in one cell
    # the lower index; three ways with the best elsewhere; four cells
    d.at_spot([(1.0, 0.0, 0, 3), (-1.0, 0.0, 0, 3)], shift=(1.0, 0.0))
    d.at_spot([(0.0, 1.0, 0, 3), (0.0, -1.0, 0, 3)], shift=(0.0, 1.0))
    d.at_spot([(0.25, 0.0, 0, 4), (0.5, 0.125, 0, 4)])
    d.at_spot([(1.0, 0.0, 0, 6), (-1.0, 0.0, 0, 6), (0.0, 0.0, 0, 30)], shift=(1.0, 0.0))
    d.at_spot([(1.0, 1.0, 0, 7), (-1.0, 1.0, 0, 7), (1.0, -1.0, 0, 7), (-1.0, -1.0, 0, 7)],
              shift=(1.0, 1.0))
    # |dx| == r exactly: outside
    d.at_spot([(r, 0.0, 0, 0), (1.0, 1.0, 0, 20)])
    d.at_spot([(0.0, -r, 0, 0), (1.0, 1.0, 0, 20)])
    d.at_spot([(-r, r, 0, 0)])
    # PredictScale: the exact level 0, the two clamps, either side of an integer; the nearest
    # descriptor two levels down or one up loses
    def level_group(level, true_oct, **kw):
        m = [(1.0, 1.0, true_oct, 10)]
        if level >= 2:
            m.append((0.5, -1.0, level - 2, 0))
        if level <= 6:
            m.append((-1.0, 0.5, level + 1, 1))
        d.at_spot(m, level=level, **kw)
    level_group(0, 0, lv=0.0, P=(0.0, 0.0, 4.0), max_dist=4.0 * d.cs)    # ratio == 1: v = 0
    level_group(0, 0, lv=-0.5)
    level_group(1, 0, lv=0.25)
    level_group(1, 1, lv=0.75)
    level_group(3, 2, lv=2.75)
    level_group(3, 3, lv=2.25)
    level_group(4, 3, lv=3.25)
    level_group(7, 6, lv=6.75)
    level_group(7, 7, lv=9.0)
    level_group(7, 6, lv=7.5)
    # the acceptance threshold
    d.at_spot([(1.0, 1.0, 0, gate)])
    d.at_spot([(1.0, 1.0, 0, gate + 1)])
    d.at_spot([(1.0, 1.0, 0, gate + 1), (-1.0, 1.0, 0, gate)])
    # depth: z == 0, z < 0, a tiny z (2^-100, still on the optical axis).  Every query on the
    # axis projects to (CX, CY) and brings its own keypoint, 5 bits away, to (CX - 1, CY + 1)
    own = [(-1.0, 1.0, 0, 5)]
    for P in ((1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -4.0), (0.5, 0.25, -2.0 ** -100)):
        d.point(CX, CY, own, P=P, min_dist=0.0, max_dist=8.0)
    t = 2.0 ** -100
    d.point(CX, CY, own, P=(0.0, 0.0, t), min_dist=0.0, max_dist=t * d.cs)
    # dist3D on and either side of 0.8f * min_dist and 1.2f * max_dist (on the optical axis
    # dist3D = z exactly; min_dist = 4 and max_dist = 2 make both products float32 numbers)
    lo = float(np.float32(0.8) * np.float32(4.0))
    hi = float(np.float32(1.2) * np.float32(2.0))
    for z in (lo, next32(lo, False), next32(lo)):
        d.point(CX, CY, own, P=(0.0, 0.0, z / d.cs), min_dist=4.0, max_dist=z)
    for z in (hi, next32(hi, False), next32(hi)):
        d.point(CX, CY, own, P=(0.0, 0.0, z / d.cs), min_dist=0.5, max_dist=2.0)


def bounds_groups(d):
    """Keypoints in the last half cell and before the first; projections between the int
    and the float bounds (fractional bounds only) and exactly on the int bounds."""
    x0, x1, y0, y1 = [float(np.float32(b)) for b in d.bounds]
    cw, ch = (x1 - x0) / 64, (y1 - y0) / 48
    ym, xm = round(0.5 * (y0 + y1)) + 0.5, round(0.5 * (x0 + x1)) + 0.5
    exact = d.bounds == POW2
    hi, lo, last = (63.5, -0.5, 63.49) if exact else (63.51, -0.51, 63.49)
    # level 3: r = 4 * 1.728 = 6.9, enough to reach across the half cell
    q = lambda v: float(np.round(v * 8) / 8) if not exact else v
    for p, found in ((hi, 0), (last, 1)):
        kx = q(x0 + p * cw)
        d.point(q(kx - 2.0), ym, [(kx - q(kx - 2.0), 0.0, 3, 2)], level=3)
        ky = q(y0 + (p - 16) * ch)
        d.point(xm, q(ky - 2.0), [(0.0, ky - q(ky - 2.0), 3, 2)], level=3)
    kx = q(x0 + lo * cw)
    u = float(int(x0)) + 0.5 if x0 >= 0 else q(x0 + 0.5)
    d.point(u, ym + 40, [(kx - u, 0.0, 5, 2), (3.0, 1.0, 5, 30)], level=5)
    ky = q(y0 + lo * ch)
    v = float(int(y0)) + 0.5 if y0 >= 0 else q(y0 + 0.5)
    d.point(xm + 40, v, [(0.0, ky - v, 3, 2), (1.0, 3.0, 3, 30)], level=3)
    # exactly on the int bounds: (int)min is inside, (int)max outside.  The keypoint next to a
    # max bound sits at grid position 63.4 / 47.4 (the last cell), octave 7, where the
    # chi-square gate of Fuse still admits it (except across TUM1's 9.5 px half cell in x)
    ix0, ix1, iy0, iy1 = float(int(x0)), float(int(x1)), float(int(y0)), float(int(y1))
    lx, ly = q(x0 + 63.4 * cw), q(y0 + 47.4 * ch)
    d.point(ix0, ym - 40, [(3.0, 1.0, 0, 5)])
    d.point(ix1, ym - 40, [(lx - ix1, 1.0, 7, 5)], level=7)
    d.point(xm - 40, iy0, [(1.0, 3.0, 0, 5)])
    d.point(xm - 40, iy1, [(1.0, ly - iy1, 7, 5)], level=7)
    d.point(ix1 - 0.125, ym - 80, [(lx - ix1 + 0.125, 1.0, 7, 5)], level=7)       # just inside
    d.point(xm - 80, iy1 - 0.125, [(1.0, ly - iy1 + 0.125, 7, 5)], level=7)
    if ix0 < x0:
        # [(int)min, min): in the image by the int bounds, left of the grid
        d.point(ix0 + 0.5, ym + 80, [(2.0, 1.0, 0, 5)])
        d.point(xm + 80, iy0 + 0.25, [(1.0, 2.0, 0, 5)])
        # [(int)max, max): out by the int bounds
        d.point(ix1 + 0.03125, ym + 120, [(lx - ix1 - 0.03125, 1.0, 7, 5)], level=7)
        d.point(xm + 120, iy1 + 0.25, [(1.0, ly - iy1 - 0.25, 7, 5)], level=7)


def fuse_designed(bounds=IMG, stereo=True, seed=41):
    d = GridDesigner(seed, bounds)
    if bounds == IMG:
        common_groups(d)
        # the viewing cosine on and either side of 0.5 (Pn need not be a unit vector)
        for nz in (0.5, next32(0.5, False), next32(0.5)):
            d.point(CX, CY, [(2.0, -1.0, 0, 9)], P=(0.0, 0.0, 4.0), max_dist=4.0,
                    normal=(0.0, 0.0, nz))
        # the chi-square gates at level 0 (invSigma2 = 1): 5.99 for a monocular keypoint, 7.8
        # with uRight >= 0; the nearest descriptor is the one outside
        d.at_spot([(2.0, 1.5, 0, 0), (1.0, 2.0, 0, 5)])              # 6.25 out, 5 in
        d.at_spot([(2.0, 2.0, 0, 0, 0.0), (2.0, 1.5, 0, 5, 1.0)])    # 8 out, 7.25 in
        d.at_spot([(2.0, 1.5, 0, 5, -1.0), (1.0, 1.0, 0, 0, 2.5)])   # 7.25 in, 8.25 out
        # uRight == 0 is a stereo keypoint: er = ur - 0 is large
        u, v = spot(d.n_spot)
        d.n_spot += 1
        D = d.rand()
        d.add_kp(u + 1.0, v + 1.0, 0, D, 0.0)
        d.add_kp(u - 1.0, v + 1.0, 0, flip(d.rng, D, 12), -1.0)
        d.point(u, v, [], desc=D)
        # level 2 (invSigma2 = 1 / 2.0736): e2 = 12.25 -> 5.9076 in, 13 -> 6.27 out
        d.at_spot([(3.5, 0.0, 2, 5), (3.0, 2.0, 2, 0)], level=2)
        for f in (0, 1):
            d.at_spot([(1.0, 1.0, 0, 3)], flags=f)
    bounds_groups(d)
    mps, md = d.points()
    return dict(kind="fuse", kf=d.keyframe(stereo), fcam=frustum(bounds), mps=mps, mdesc=md,
                th=4.0)


def fuse_window_th2(seed=44):
    """th = 2 puts |dx| == r where the chi-square gate of Fuse still admits the keypoint
    (e2 = 4 < 5.99), so the strict window test is visible in Fuse too."""
    d = GridDesigner(seed)
    d.at_spot([(2.0, 0.0, 0, 0), (1.0, 1.0, 0, 20)])
    d.at_spot([(0.0, -2.0, 0, 0), (1.0, 1.0, 0, 20)])
    d.at_spot([(-2.0, 2.0, 0, 0)])
    mps, md = d.points()
    return dict(kind="fuse", kf=d.keyframe(True), fcam=frustum(IMG), mps=mps, mdesc=md, th=2.0)


def fuse_sim3_designed(bounds=IMG, scale=2.0, seed=42):
    d = GridDesigner(seed, bounds)
    if bounds == IMG:
        common_groups(d)
        d.at_spot([(2.0, 2.0, 0, 0), (1.0, 1.0, 0, 9)])       # no chi-square gate: 8 is in
        d.at_spot([(1.0, 1.0, 0, 3)], normal=(0.0, 0.0, -1.0))  # facing away: gated here too
        d.at_spot([(1.0, 1.0, 0, 3)], flags=0)
    bounds_groups(d)
    mps, md = d.points()
    return dict(kind="fuse_sim3", kf=d.keyframe(False), fcam=frustum(bounds, scale=scale),
                mps=mps, mdesc=md, th=4.0)


def sim3_pair(bounds, T1w=None, T2w=None, R12=None, t12=(0, 0, 0), s12=1.0):
    g = np.zeros((), SIM3_PAIR_DTYPE)
    g["T1w"] = (pose() if T1w is None else T1w).reshape(-1)
    g["T2w"] = (pose() if T2w is None else T2w).reshape(-1)
    g["R12"] = (np.eye(3) if R12 is None else R12).reshape(-1)
    g["t12"], g["s12"] = t12, s12
    g["fx"], g["fy"], g["cx"], g["cy"] = FX, FY, CX, CY
    g["log_scale_factor"], g["nlevels"] = LOG_SF, 8
    g["min_x"], g["max_x"], g["min_y"], g["max_y"] = bounds
    return g


def sim3_designed(bounds=IMG, s12=2.0, seed=43):
    """pKF1 at the identity, pKF2 = pKF1 seen through s12 = 2 (R12 = I, t12 = 0): a world point
    lands on the same pixel in both, at half the distance in pKF2.  pKF1 holds one keypoint
    per query, pKF2 the query's group; every pKF2 keypoint carries a map point that finds
    the query's pKF1 keypoint on the way back, so the first direction decides the result."""
    d = GridDesigner(seed, bounds, cam_scale=1.0 / s12)
    if bounds == IMG:
        common_groups(d, gate=100)
    bounds_groups(d)
    special = {}
    if bounds == IMG:
        special["one_way"] = d.at_spot([(1.0, 1.0, 0, 3)])     # nothing comes back
        special["matched1"] = d.at_spot([(1.0, 1.0, 0, 3)])
        special["matched2"] = d.at_spot([(1.0, 1.0, 0, 3)])
        special["invalid2"] = d.at_spot([(1.0, 1.0, 0, 3)])
        special["invalid1"] = d.at_spot([(1.0, 1.0, 0, 3)], flags=0)
        special["other_back"] = d.at_spot([(1.0, 1.0, 0, 3)])  # comes back to another keypoint
    kf2 = d.keyframe(False)
    mp1, md1 = d.points()
    n1, n2 = len(mp1), len(kf2["kps"])
    # pKF1: keypoint i at query i's pixel, octave = the query's level
    k1 = np.zeros(n1, KP_DTYPE)
    d1 = np.zeros((n1, 32), np.uint8)
    for i, q in enumerate(d.q):
        k1["x"][i], k1["y"][i], k1["octave"][i] = q["uv"][0], q["uv"][1], q["level"]
        d1[i] = flip(d.rng, q["desc"], 2)
    k1["size"] = 31
    # pKF2's map points: keypoint j of query i's group looks back at keypoint i
    mp2 = np.zeros(n2, MAPPOINT_DTYPE)
    md2 = d.rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    owner = np.asarray(d.owner)
    for j in range(n2):
        i = int(owner[j])
        z = 4.0
        x, y = float(kf2["kps"]["x"][j]), float(kf2["kps"]["y"][j])
        Q = np.array([(x - CX) / FX * z, (y - CY) / FY * z, z]) / s12   # lands on (x, y) in pKF1
        dist = float(np.sqrt((Q * Q).sum())) * s12
        mp2["x"][j], mp2["y"][j], mp2["z"][j] = Q
        mp2["max_dist"][j] = dist * log_level(d.q[i]["level"] - 0.5)
        mp2["min_dist"][j] = 0.25 * min(dist, float(mp2["max_dist"][j]))
        mp2["flags"][j] = 1
        md2[j] = flip(d.rng, d1[i], 4)
    matched1 = np.zeros(n1, np.uint8)
    matched2 = np.zeros(n2, np.uint8)
    if special:
        js = {k: int(np.nonzero(owner == v)[0][0]) for k, v in special.items()}
        md2[js["one_way"]] = d.rng.integers(0, 256, 32, dtype=np.uint8)
        matched1[special["matched1"]] = 1
        matched2[js["matched2"]] = 1
        mp2["flags"][js["invalid2"]] = 0
        md2[js["other_back"]] = flip(d.rng, d1[special["one_way"]], 1)
        mp2["x"][js["other_back"]], mp2["y"][js["other_back"]] = (
            mp2["x"][js["one_way"]], mp2["y"][js["one_way"]])
    return dict(kind="sim3", kf1=dict(kps=k1, desc=d1), mp1=mp1, md1=md1, matched1=matched1,
                kf2=kf2, mp2=mp2, md2=md2, matched2=matched2, g=sim3_pair(bounds, s12=s12),
                th=4.0)


def _world(uv, z, T):
    T = np.asarray(T, np.float64)
    cam = np.stack([(uv[:, 0] - CX) / FX * z, (uv[:, 1] - CY) / FY * z, z], 1)
    return (cam - T[:, 3]) @ T[:, :3]


def _random_kf(rng, n, bounds):
    b = [float(np.float32(v)) for v in bounds]
    k = np.zeros(n, KP_DTYPE)
    k["x"] = (rng.integers(int(b[0]) + 1, int(b[1]) - 1, n) + rng.integers(1, 8, n) / 8.0)
    k["y"] = (rng.integers(int(b[2]) + 1, int(b[3]) - 1, n) + rng.integers(1, 8, n) / 8.0)
    k["octave"] = rng.integers(0, 8, n)
    k["size"] = 31
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _random_points(rng, kps, desc, nmp, T, cam_scale=1.0, spread=3.0):
    """nmp map points projecting near random keypoints under the pose T, their level window
    around the keypoint's octave, their descriptor 0 .. 60 bits from the keypoint's."""
    n = len(kps)
    mps = np.zeros(nmp, MAPPOINT_DTYPE)
    md = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    j = rng.integers(0, max(n, 1), nmp)
    uv = np.stack([rng.uniform(0, 640, nmp), rng.uniform(0, 480, nmp)], 1)
    if n:
        uv = np.stack([kps["x"][j] + rng.uniform(-spread, spread, nmp),
                       kps["y"][j] + rng.uniform(-spread, spread, nmp)], 1)
    z = rng.uniform(2, 12, nmp)
    z[rng.random(nmp) < 0.03] *= -1
    W = _world(uv, z, T)
    mps["x"], mps["y"], mps["z"] = W[:, 0], W[:, 1], W[:, 2]
    Tm = np.asarray(T, np.float64)
    Ow = -Tm[:, :3].T @ Tm[:, 3]
    PO = W - Ow
    dist = np.sqrt((PO * PO).sum(1)) * cam_scale
    lv = (kps["octave"][j] if n else np.zeros(nmp)) + rng.uniform(-0.9, 0.9, nmp)
    mps["max_dist"] = dist * np.exp(lv * LOG_SF)
    mps["min_dist"] = mps["max_dist"] / SF[7]
    e = rng.random(nmp)
    mps["min_dist"][e < 0.03] = dist[e < 0.03] * 1.3
    mps["max_dist"][(e >= 0.03) & (e < 0.06)] = dist[(e >= 0.03) & (e < 0.06)] * 0.8
    nrm = PO / np.sqrt((PO * PO).sum(1))[:, None] + rng.normal(0, 0.5, (nmp, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    mps["nx"], mps["ny"], mps["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    mps["flags"] = rng.random(nmp) < 0.93
    for q in range(nmp if n else 0):
        md[q] = flip(rng, desc[j[q]], rng.integers(0, 60))
    return mps, md


def grid_random(kind, seed, nk=300, nmp=400, bounds=IMG, scale=1.0, th=3.0):
    rng = np.random.default_rng(seed)
    kps, desc = _random_kf(rng, nk, bounds)
    T = pose((0.02, -0.03, 0.01), (0.1, -0.05, 0.2))
    mps, md = _random_points(rng, kps, desc, nmp, T)
    ur = (kps["x"] - 8.0 + rng.uniform(-1, 1, nk)).astype(np.float32)
    e = rng.random(nk)
    ur[e < 0.4] = -1.0
    ur[(e >= 0.4) & (e < 0.45)] = 0.0
    return dict(kind=kind, kf=dict(kps=kps, desc=desc, uright=ur if kind == "fuse" else None),
                fcam=frustum(bounds, T, scale), mps=mps, mdesc=md, th=th)


def sim3_random(seed, n=300, bounds=IMG, s12=1.03, th=7.5):
    """One point set seen by two KeyFrames; S12 = (s12, R1 R2^T, t1 - s12 R12 t2) maps pKF2's
    camera frame (at 1 / s12 of the true size) to pKF1's."""
    rng = np.random.default_rng(seed)
    T1 = pose((0.01, 0.02, -0.01), (0.05, 0.0, 0.1)).astype(np.float64)
    T2 = pose((-0.02, 0.01, 0.02), (-0.1, 0.05, 0.0)).astype(np.float64)
    k1, d1 = _random_kf(rng, n, bounds)
    W = _world(np.stack([k1["x"], k1["y"]], 1).astype(np.float64) + rng.uniform(-1, 1, (n, 2)),
               rng.uniform(3, 10, n), T1)
    c2 = (W @ T2[:, :3].T + T2[:, 3])
    perm = rng.permutation(n)
    k2 = np.zeros(n, KP_DTYPE)
    k2["x"][perm] = FX * c2[:, 0] / c2[:, 2] + CX + rng.uniform(-1, 1, n)
    k2["y"][perm] = FY * c2[:, 1] / c2[:, 2] + CY + rng.uniform(-1, 1, n)
    k2["octave"][perm] = np.clip(k1["octave"] + rng.integers(-1, 2, n), 0, 7)
    k2["size"] = 31
    d2 = np.zeros((n, 32), np.uint8)
    for i in range(n):
        d2[perm[i]] = flip(rng, d1[i], rng.integers(0, 90))
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = T1[:, 3] - R12 @ T2[:, 3]
    mp1 = np.zeros(n, MAPPOINT_DTYPE)
    mp2 = np.zeros(n, MAPPOINT_DTYPE)
    for mp, order, o_other, Tother in ((mp1, np.arange(n), k2["octave"][perm], T2),
                                       (mp2, perm, k1["octave"], T1)):
        mp["x"][order], mp["y"][order], mp["z"][order] = W[:, 0], W[:, 1], W[:, 2]
        co = W @ Tother[:, :3].T + Tother[:, 3]
        dist = np.sqrt((co * co).sum(1))
        lv = o_other + rng.uniform(-0.9, 0.9, n)
        mp["max_dist"][order] = dist * np.exp(lv * LOG_SF)
        mp["min_dist"][order] = mp["max_dist"][order] / SF[7]
        mp["flags"][order] = rng.random(n) < 0.9
    md1 = np.array([flip(rng, d1[i], 3) for i in range(n)], np.uint8)
    md2 = np.array([flip(rng, d2[i], 3) for i in range(n)], np.uint8)
    g = sim3_pair(bounds, T1.astype(np.float32), T2.astype(np.float32), R12, t12, s12)
    return dict(kind="sim3", kf1=dict(kps=k1, desc=d1), mp1=mp1, md1=md1,
                matched1=(rng.random(n) < 0.1).astype(np.uint8), kf2=dict(kps=k2, desc=d2),
                mp2=mp2, md2=md2, matched2=(rng.random(n) < 0.1).astype(np.uint8), g=g, th=th)


# ================================================================ runners
def run_ref(s, variant=None):
    k = s["kind"]
    if k in ("bow", "bowkf", "tri"):
        a, b = s["s1"], s["s2"]
        if k == "bow":
            return R.search_by_bow(a["desc"], a["kps"]["angle"], a["ok"], a["fv"], b["desc"],
                                   b["kps"]["angle"], b["fv"], s["nnratio"], s["ori"], variant)
        if k == "bowkf":
            return R.search_by_bow_kf(a["desc"], a["kps"]["angle"], a["ok"], a["fv"], b["desc"],
                                      b["kps"]["angle"], b["ok"], b["fv"], s["nnratio"], s["ori"],
                                      variant)
        return R.search_for_triangulation(_tri_side(a), _tri_side(b), s["geom"], SF, SIGMA2,
                                          s["only_stereo"], s["ori"], variant)
    if k == "fuse":
        return R.fuse(s["kf"], s["fcam"], s["mps"], s["mdesc"], s["th"], SF, INV_SIGMA2, variant)
    if k == "fuse_sim3":
        return R.fuse_sim3(s["kf"], s["fcam"], s["mps"], s["mdesc"], s["th"], SF, variant)
    return R.search_by_sim3(s["kf1"], s["mp1"], s["md1"], s["matched1"], s["kf2"], s["mp2"],
                            s["md2"], s["matched2"], s["g"], s["th"], SF, variant)


def _tri_side(a):
    return dict(kps=a["kps"], desc=a["desc"], uright=a["uright"], has_mp=1 - a["ok"], fv=a["fv"])


def outputs(r, kind):
    """The result as the tuple the oracle and the host entries return."""
    if kind in ("fuse", "fuse_sim3"):
        return r.n, r.best_idx, r.best_dist
    return r.nmatches, r.match


def run_oracle(o, s):
    k = s["kind"]
    if k in ("bow", "bowkf", "tri"):
        a, b = s["s1"], s["s2"]
        if k == "bow":
            return o.search_by_bow(a["desc"], a["kps"]["angle"], a["ok"], a["fv"], b["desc"],
                                   b["kps"]["angle"], b["fv"], s["nnratio"], s["ori"])
        if k == "bowkf":
            return o.search_by_bow_kf(a["desc"], a["kps"]["angle"], a["ok"], a["fv"], b["desc"],
                                      b["kps"]["angle"], b["ok"], b["fv"], s["nnratio"], s["ori"])
        return o.search_for_triangulation(_tri_side(a), _tri_side(b),
                                          s["geom"].view(o.TRI_GEOM_DTYPE), SF, SIGMA2,
                                          s["only_stereo"], s["ori"])
    if k in ("fuse", "fuse_sim3"):
        kf = dict(s["kf"])
        if kf.get("uright") is None:
            kf["uright"] = np.full(len(kf["kps"]), -1.0, np.float32)
        fc, mp = s["fcam"].view(o.FRUSTUM_DTYPE), s["mps"].view(o.MAPPOINT_DTYPE)
        if k == "fuse":
            return o.fuse_search(kf, fc, mp, s["mdesc"], s["th"], SF, INV_SIGMA2)
        return o.fuse_sim3_search(kf, fc, mp, s["mdesc"], s["th"], SF)
    return o.search_by_sim3(s["kf1"], s["mp1"].view(o.MAPPOINT_DTYPE), s["md1"], s["matched1"],
                            s["kf2"], s["mp2"].view(o.MAPPOINT_DTYPE), s["md2"], s["matched2"],
                            s["g"].view(o.SIM3_PAIR_DTYPE), s["th"], SF)


def run_gpu(s):
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import Frame, ORBmatcher
    k = s["kind"]
    m = ORBmatcher(s.get("nnratio", 0.6), s.get("ori", False))
    if k in ("bow", "bowkf"):
        a, b = s["s1"], s["s2"]
        A = Frame(a["kps"].astype(L.KP_DTYPE), a["desc"], mFeatVec=a["fv"], map_valid=a["ok"])
        B = Frame(b["kps"].astype(L.KP_DTYPE), b["desc"], mFeatVec=b["fv"], map_valid=b["ok"])
        return m.SearchByBoW(A, B) if k == "bow" else m.SearchByBoW_KF(A, B)
    if k == "tri":
        fr = [Frame(a["kps"].astype(L.KP_DTYPE), a["desc"], mvuRight=a["uright"],
                    mFeatVec=a["fv"], has_mp=1 - a["ok"]) for a in (s["s1"], s["s2"])]
        return m.SearchForTriangulation(fr[0], fr[1], s["geom"].view(L.TRI_GEOM_DTYPE),
                                        s["only_stereo"])
    if k in ("fuse", "fuse_sim3"):
        kf = s["kf"]
        F = Frame(kf["kps"].astype(L.KP_DTYPE), kf["desc"], mvuRight=kf.get("uright"))
        fn = m.Fuse if k == "fuse" else m.FuseSim3
        return fn(F, s["fcam"].view(L.FRUSTUM_DTYPE), s["mps"].view(L.MAPPOINT_DTYPE), s["mdesc"],
                  s["th"])
    F1 = Frame(s["kf1"]["kps"].astype(L.KP_DTYPE), s["kf1"]["desc"])
    F2 = Frame(s["kf2"]["kps"].astype(L.KP_DTYPE), s["kf2"]["desc"])
    return m.SearchBySim3(F1, F2, s["mp1"].view(L.MAPPOINT_DTYPE), s["md1"],
                          s["mp2"].view(L.MAPPOINT_DTYPE), s["md2"], s["g"].view(L.SIM3_PAIR_DTYPE),
                          s["th"], s["matched1"], s["matched2"])


def check_equal(got, s, what):
    """got = the tuple of the oracle or the kernels; every array and count equal."""
    r = run_ref(s)
    want = outputs(r, s["kind"])
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        if np.ndim(w):
            assert np.array_equal(np.asarray(g, np.int64), w), what
        else:
            assert int(g) == int(w), what
    return r


# ================================================================ the margin filter
def _drop_nodes(side, ids):
    nodes, off, feats = side["fv"]
    keep = [k for k in range(len(nodes)) if int(nodes[k]) not in ids]
    new_off, new_feats = [0], []
    for k in keep:
        new_feats += list(feats[off[k]:off[k + 1]])
        new_off.append(len(new_feats))
    gone = len(feats) - len(new_feats)
    return dict(side, fv=(np.asarray(nodes[keep], np.int32), np.asarray(new_off, np.int32),
                          np.asarray(new_feats, np.int32))), gone


def _drop_feats(side, idx):
    nodes, off, feats = side["fv"]
    new_off, new_feats = [0], []
    for k in range(len(nodes)):
        new_feats += [f for f in feats[off[k]:off[k + 1]] if int(f) not in idx]
        new_off.append(len(new_feats))
    return dict(side, fv=(nodes, np.asarray(new_off, np.int32), np.asarray(new_feats, np.int32)))


def filtered(s):
    """Remove what an ambiguous decision names, repeat until none is left; at most DROP_CAP."""
    s = dict(s)
    k = s["kind"]
    dropped, total = 0, 1
    s["ori_dropped"] = False
    for _ in range(10):
        M = run_ref(s).margins
        amb = [a for a in M.ambiguous() if a[1][0] != "range"]   # a cell-range flip changes nothing
        if not amb:
            break
        who = lambda tag: sorted({a[1][1] for a in amb if a[1][0] == tag})
        assert not who("pose"), amb
        if k in ("bow", "bowkf", "tri"):
            total = len(s["s1"]["desc"]) + len(s["s2"]["desc"])
            if who("ori") or who("call"):
                s["ori"], s["ori_dropped"] = False, True
            if who("n1"):
                ids = set(who("n1"))
                s["s1"], g1 = _drop_nodes(s["s1"], ids)
                s["s2"], g2 = _drop_nodes(s["s2"], ids)
                dropped += g1 + g2
            if who("f1"):
                s["s1"] = _drop_feats(s["s1"], set(who("f1")))
                dropped += len(who("f1"))
        elif k in ("fuse", "fuse_sim3"):
            total = len(s["kf"]["kps"]) + len(s["mps"])
            kk, qq = who("kp"), who("q")
            keep = np.ones(len(s["kf"]["kps"]), bool)
            keep[kk] = False
            s["kf"] = {a: (None if v is None else np.ascontiguousarray(v[keep]))
                       for a, v in s["kf"].items()}
            keep = np.ones(len(s["mps"]), bool)
            keep[qq] = False
            s["mps"], s["mdesc"] = s["mps"][keep], np.ascontiguousarray(s["mdesc"][keep])
            dropped += len(kk) + len(qq)
        else:
            total = len(s["kf1"]["kps"]) + len(s["kf2"]["kps"])
            # a keypoint carries its map point: dropping either invalidates the slot's point
            # and moves the keypoint out of every window
            for tags, kf, mp in ((("kp1", "q"), "kf1", "mp1"), (("kp", "q2"), "kf2", "mp2")):
                idx = sorted(set(who(tags[0])) | set(who(tags[1])))
                if idx:
                    s[mp] = s[mp].copy()
                    s[mp]["flags"][idx] = 0
                    kps = s[kf]["kps"].copy()
                    kps["x"][idx], kps["y"][idx] = -1000.0, -1000.0
                    s[kf] = dict(s[kf], kps=kps)
                    dropped += len(idx)
    M = run_ref(s).margins
    assert not [a for a in M.ambiguous() if a[1][0] != "range"], M.ambiguous()[:5]
    s["dropped"] = dropped / max(total, 1)
    assert s["dropped"] <= DROP_CAP, s["dropped"]
    return s


# ================================================================ the scenes by name
FV_KINDS = ("bow", "bowkf", "tri")


def scene_builders():
    sc = {}
    for k in FV_KINDS:
        sc[k + "_chunks"] = lambda k=k: fv_chunks(k)
        sc[k + "_ties"] = lambda k=k: fv_ties(k)
        sc[k + "_second"] = lambda k=k: fv_second(k)
        sc[k + "_walk"] = lambda k=k: fv_walk(k)
        sc[k + "_shared"] = lambda k=k: fv_shared(k)
        sc[k + "_invalid"] = lambda k=k: fv_invalid(k)
        sc[k + "_thresholds75"] = lambda k=k: fv_thresholds(k, 0.75)
        sc[k + "_thresholds50"] = lambda k=k: fv_thresholds(k, 0.5)
        for n in (1023, 1024, 1025, 2049):
            sc["%s_join%d" % (k, n)] = lambda k=k, n=n: fv_join(k, n)
        for h in HISTS:
            sc["%s_rot_%s" % (k, h)] = lambda k=k, h=h: fv_rotation(k, HISTS[h])
        sc[k + "_random"] = lambda k=k: fv_random(k, 51)
        sc[k + "_random_few_nodes"] = lambda k=k: fv_random(k, 52, n=600, nnodes=3, ori=False)
    sc["tri_geometry"] = lambda: tri_geometry(False)
    sc["tri_geometry_only_stereo"] = lambda: tri_geometry(True)
    sc["tri_degenerate_line"] = tri_degenerate
    for bn, b in (("img", IMG), ("tum1", TUM1), ("pow2", POW2)):
        sc["fuse_designed_" + bn] = lambda b=b: fuse_designed(b)
        sc["fuse_sim3_designed_" + bn] = lambda b=b: fuse_sim3_designed(b)
        sc["sim3_designed_" + bn] = lambda b=b: sim3_designed(b)
    sc["fuse_designed_mono"] = lambda: fuse_designed(IMG, stereo=False)
    sc["fuse_window_th2"] = fuse_window_th2
    sc["fuse_random"] = lambda: grid_random("fuse", 61, bounds=TUM1)
    sc["fuse_sim3_random"] = lambda: grid_random("fuse_sim3", 62, scale=1.7, th=4.0)
    sc["sim3_random"] = lambda: sim3_random(63)
    for nmp in (1, 255, 256, 257, 1023, 1024, 1025):
        sc["fuse_n%d" % nmp] = lambda nmp=nmp: grid_random("fuse", 70 + nmp % 7, nmp=nmp)
        sc["fuse_sim3_n%d" % nmp] = lambda nmp=nmp: grid_random("fuse_sim3", 80 + nmp % 7, nmp=nmp,
                                                               scale=0.5, th=4.0)
    for nk in (0, 1):
        sc["fuse_kf%d" % nk] = lambda nk=nk: grid_random("fuse", 90, nk=nk, nmp=40)
        sc["fuse_sim3_kf%d" % nk] = lambda nk=nk: grid_random("fuse_sim3", 91, nk=nk, nmp=40)
    for n in (1, 255, 256, 257, 1023, 1024, 1025):
        sc["sim3_n%d" % n] = lambda n=n: sim3_random(100 + n % 7, n=n)
    return sc


DESIGNED_ROTATION = tuple("%s_rot_%s" % (k, h) for k in FV_KINDS for h in HISTS)
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = filtered(scene_builders()[name]())
    return _cache[name]


SCENE_NAMES = sorted(scene_builders())
