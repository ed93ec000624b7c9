"""Synthetic matcher scenes for test_matching_ref.py (CPU) and test_gpu_matching_ref.py.

A scene is a dict of host arrays for one call of SearchForInitialization ("sfi"), of the
last-frame SearchByProjection ("last") or of the local-map one ("local"); keypoints are drawn,
not extracted, so they reach the image border, the last half cell and non-integer bounds.
filtered() asks ref_matching for its float margins and drops the keypoints and queries with an
ambiguous decision until none is left (at most 2 % of a scene, asserted), after which the
comparison with the oracle or the kernels is exact.  Sizes cross the kernels' boundaries: 128
queries per k_track_cands workgroup, resolver chunks of 64, K-lists of 8.
"""
import numpy as np

import ref_matching as R

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
LF_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("octave", "<i4"),
                     ("angle", "<f4"), ("flags", "<i4")])
MP_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("level", "<i4"),
                     ("view_cos", "<f4"), ("flags", "<i4")])
SF = R.scale_factors(1.2, 8)
IMG = (0.0, 640.0, 0.0, 480.0)
DIST = (-12.3, 655.7, -9.6, 489.1)
FX = FY = 512.0
CX, CY, BF = 320.0, 240.0, 40.0
NK, NQ = 601, 259
DROP_CAP = 0.02


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(rot=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = _rot(*rot)
    T[:, 3] = t
    return T


def camera(Tcw=None, Tlw=None, mono=True):
    return dict(Tcw=pose() if Tcw is None else Tcw, Tlw=pose() if Tlw is None else Tlw, fx=FX,
                fy=FY, cx=CX, cy=CY, bf=BF, b=BF / FX, mono=mono)


def flip(rng, d, k):
    """d with exactly k bits flipped: Hamming distance k."""
    bits = np.unpackbits(np.asarray(d, np.uint8))
    bits[rng.choice(256, int(k), replace=False)] ^= 1
    return np.packbits(bits)


def _lattice(rng, lo, hi, n):
    """Coordinates k + j / 8, j = 1..7: exact in float32 and never on a cell boundary of the
    10-pixel grid of IMG, nor a half cell."""
    return (rng.integers(int(lo), int(hi), n) + rng.integers(1, 8, n) / 8.0).astype(np.float32)


def frame(rng, n, bounds, lattice=False, p_oct0=0.3):
    b = [float(np.float32(v)) for v in bounds]
    k = np.zeros(n, KP_DTYPE)
    if lattice:
        k["x"], k["y"] = _lattice(rng, b[0], b[1], n), _lattice(rng, b[2], b[3], n)
    else:
        k["x"] = rng.uniform(b[0] + 0.3, b[1] - 0.3, n)
        k["y"] = rng.uniform(b[2] + 0.3, b[3] - 0.3, n)
        cw, ch = (b[1] - b[0]) / 64, (b[3] - b[2]) / 48
        e = rng.random(n)
        # the last half cell of the right and bottom edges (in no cell), the first half cell
        m = e < 0.06
        k["x"][m] = b[1] - rng.uniform(0.03, 0.47, m.sum()) * cw
        m = (e >= 0.06) & (e < 0.12)
        k["y"][m] = b[3] - rng.uniform(0.03, 0.47, m.sum()) * ch
        m = (e >= 0.12) & (e < 0.15)
        k["x"][m] = b[0] + rng.uniform(0.03, 0.47, m.sum()) * cw
        m = (e >= 0.15) & (e < 0.18)
        k["y"][m] = b[2] + rng.uniform(0.03, 0.47, m.sum()) * ch
    p = np.full(8, (1 - p_oct0) / 7)
    p[0] = p_oct0
    k["octave"] = rng.choice(8, n, p=p)
    k["angle"] = rng.uniform(0, 360, n)
    k["size"] = 31
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def edge_targets(bounds, step=0.05):
    """(u, v) just inside and just outside each bound, and windows clipped at each edge."""
    x0, x1, y0, y1 = [float(np.float32(v)) for v in bounds]
    mx, my = 0.5 * (x0 + x1) + 1.7, 0.5 * (y0 + y1) + 2.3
    out = []
    for s in (-step, step):
        out += [(x0 + s, my), (x1 + s, my), (mx, y0 + s), (mx, y1 + s)]
    out += [(x0 + 3.3, my + 40), (x1 - 3.3, my - 40), (mx + 50, y0 + 3.3), (mx - 50, y1 - 3.3),
            (x0 + 2.1, y0 + 2.1), (x1 - 2.1, y1 - 2.1), (x1 + 30.0, my), (mx, y0 - 30.0)]
    return out


def uright_of(rng, kps, disp=8.0):
    ur = (kps["x"] - np.float32(disp) + rng.uniform(-6, 6, len(kps))).astype(np.float32)
    e = rng.random(len(kps))
    ur[e < 0.25] = -1.0
    ur[(e >= 0.25) & (e < 0.30)] = 0.0
    ur[(e >= 0.30) & (e < 0.33)] = -3.5
    return ur


def targets(rng, kps, desc, nq, spread, extra=()):
    """nq query positions near random keypoints, their descriptors a few bits away."""
    n = len(kps)
    j = rng.integers(0, max(n, 1), nq)
    uv = np.zeros((nq, 2))
    qd = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    if n:
        uv[:, 0] = kps["x"][j] + rng.uniform(-spread, spread, nq)
        uv[:, 1] = kps["y"][j] + rng.uniform(-spread, spread, nq)
        for q in range(nq):
            qd[q] = flip(rng, desc[j[q]], rng.integers(0, 40))
    for q, t in enumerate(extra[:nq]):
        uv[q] = t
    return j, uv, qd


def world_points(uv, zc, Tcw):
    """float32 world points that project near uv at depth zc under Tcw."""
    T = np.asarray(Tcw, np.float64)
    cam = np.stack([(uv[:, 0] - CX) / FX * zc, (uv[:, 1] - CY) / FY * zc, zc], 1)
    return ((cam - T[:, 3]) @ T[:, :3]).astype(np.float32)   # R^T (cam - t)


def last_scene(seed, bounds=IMG, nk=NK, nq=NQ, th=15.0, mono=True, tz=0.0, taken_frac=0.0,
               stereo=False, ori=True, rot=(0.01, -0.02, 0.015), spread=6.0):
    rng = np.random.default_rng(seed)
    kps, desc = frame(rng, nk, bounds)
    Tcw = pose(rot, (0.05, -0.02, tz))
    j, uv, qd = targets(rng, kps, desc, nq, spread, edge_targets(bounds))
    pts = np.zeros(nq, LF_DTYPE)
    w = world_points(uv, rng.uniform(4, 20, nq), Tcw)
    pts["x"], pts["y"], pts["z"] = w[:, 0], w[:, 1], w[:, 2]
    if nk:
        pts["octave"] = np.clip(kps["octave"][j] + rng.integers(-1, 2, nq), 0, 7)
        pts["angle"] = (kps["angle"][j] + rng.choice([0.0, 0.0, 0.0, 95.0], nq)
                        + rng.uniform(-10, 10, nq)) % 360
    pts["flags"] = R.MP_VALID * (rng.random(nq) < 0.95) + R.MP_HAS_OBS * (rng.random(nq) < 0.7)
    if nq > 8:
        pts["z"][5] = -pts["z"][5]     # behind the camera
    taken = (rng.random(nk) < taken_frac).astype(np.uint8) if taken_frac else None
    return dict(kind="last", kps=kps, desc=desc, bounds=bounds, pts=pts, pdesc=qd, th=th,
                cam=camera(Tcw, pose(), mono), ori=ori, taken=taken,
                uright=uright_of(rng, kps) if stereo else None)


def local_scene(seed, bounds=IMG, nk=NK, nq=NQ, th=1.0, nnratio=0.8, taken_frac=0.0,
                stereo=False, spread=2.0):
    rng = np.random.default_rng(seed)
    kps, desc = frame(rng, nk, bounds)
    j, uv, qd = targets(rng, kps, desc, nq, spread * th, edge_targets(bounds))
    mps = np.zeros(nq, MP_DTYPE)
    mps["u"], mps["v"] = uv[:, 0], uv[:, 1]
    mps["ur"] = mps["u"] - 8.0 + rng.uniform(-5, 5, nq)
    if nk:
        mps["level"] = np.clip(kps["octave"][j] + rng.integers(0, 2, nq), 0, 7)
    mps["view_cos"] = rng.choice(np.array([0.9, 0.998, 0.9985, 1.0], np.float32), nq)
    mps["flags"] = R.MP_VALID * (rng.random(nq) < 0.95) + R.MP_HAS_OBS * (rng.random(nq) < 0.7)
    taken = (rng.random(nk) < taken_frac).astype(np.uint8) if taken_frac else None
    return dict(kind="local", kps=kps, desc=desc, bounds=bounds, mps=mps, mdesc=qd, th=th,
                nnratio=nnratio, taken=taken, uright=uright_of(rng, kps) if stereo else None)


def sfi_scene(seed, bounds=IMG, n1=NK, n2=NK, window=30, nnratio=0.9, ori=True):
    rng = np.random.default_rng(seed)
    k2, d2 = frame(rng, n2, bounds, p_oct0=0.7)
    j, uv, d1 = targets(rng, k2, d2, n1, 0.4 * window, edge_targets(bounds))
    k1 = np.zeros(n1, KP_DTYPE)
    k1["x"], k1["y"] = uv[:, 0], uv[:, 1]
    k1["octave"] = rng.choice(3, n1, p=[0.8, 0.1, 0.1])
    if n2:
        k1["angle"] = (k2["angle"][j] + rng.choice([0.0, 0.0, 0.0, 95.0], n1)
                       + rng.uniform(-10, 10, n1)) % 360
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    return dict(kind="sfi", kps=k2, desc=d2, bounds=bounds, kps1=k1, desc1=d1, prev=prev,
                window=window, nnratio=nnratio, ori=ori)


# ---- designed scenes: exact coordinates (eighths of a pixel, identity pose, depth 1)
def spots(k):
    return 63.5 + 70.0 * (k % 8), 63.5 + 70.0 * (k // 8)


class Designer:
    """Keypoints and queries at separate spots of IMG; every query sees only its own group
    (every other descriptor is random, about 128 bits away)."""

    def __init__(self, seed, n_background=200):
        self.rng = np.random.default_rng(seed)
        self.kps, self.desc = frame(self.rng, n_background, IMG, lattice=True)
        # keep the background clear of the spots
        far = np.ones(n_background, bool)
        for k in range(40):
            sx, sy = spots(k)
            far &= (np.abs(self.kps["x"] - sx) > 24) | (np.abs(self.kps["y"] - sy) > 24)
        self.kps, self.desc = self.kps[far], self.desc[far]
        self.uright = np.full(len(self.kps), -1.0, np.float32)
        self.q = []          # (u, v, level, desc, angle, ur)
        self.spot = 0

    def kp(self, x, y, octave, desc, angle=0.0, uright=-1.0):
        k = np.zeros(1, KP_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"], k["size"] = x, y, octave, angle, 31
        self.kps = np.concatenate([self.kps, k])
        self.desc = np.concatenate([self.desc, np.asarray(desc, np.uint8).reshape(1, 32)])
        self.uright = np.concatenate([self.uright, np.float32([uright])])

    def group(self, level, members, angle=0.0, q_angle=0.0, dxy=(0.0, 0.0)):
        """One query at the next spot; members = (dx, dy, octave, distance[, uright - ur])."""
        sx, sy = spots(self.spot)
        sx, sy = sx + dxy[0], sy + dxy[1]
        self.spot += 1
        D = self.rng.integers(0, 256, 32, dtype=np.uint8)
        ur = sx - BF     # depth 1
        for m in members:
            self.kp(sx + m[0], sy + m[1], m[2], flip(self.rng, D, m[3]), angle,
                    ur + m[4] if len(m) > 4 else -1.0)
        self.q.append((sx, sy, level, D, q_angle, ur))

    def last(self, th=7.0, ori=False, stereo=False, flags=R.MP_VALID | R.MP_HAS_OBS):
        n = len(self.q)
        pts = np.zeros(n, LF_DTYPE)
        uv = np.array([[q[0], q[1]] for q in self.q]).reshape(n, 2)
        w = world_points(uv, np.ones(n), pose())
        pts["x"], pts["y"], pts["z"] = w[:, 0], w[:, 1], w[:, 2]
        pts["octave"] = [q[2] for q in self.q]
        pts["angle"] = [q[4] for q in self.q]
        pts["flags"] = flags
        return dict(kind="last", kps=self.kps, desc=self.desc, bounds=IMG, pts=pts,
                    pdesc=np.array([q[3] for q in self.q], np.uint8).reshape(n, 32), th=th,
                    cam=camera(mono=not stereo), ori=ori, taken=None,
                    uright=self.uright if stereo else None)

    def local(self, th=1.0, nnratio=0.75, stereo=False):
        n = len(self.q)
        mps = np.zeros(n, MP_DTYPE)
        mps["u"], mps["v"] = [q[0] for q in self.q], [q[1] for q in self.q]
        mps["ur"] = [q[5] for q in self.q]
        mps["level"] = [q[2] for q in self.q]
        mps["view_cos"] = 0.9
        mps["flags"] = R.MP_VALID | R.MP_HAS_OBS
        return dict(kind="local", kps=self.kps, desc=self.desc, bounds=IMG, mps=mps,
                    mdesc=np.array([q[3] for q in self.q], np.uint8).reshape(n, 32), th=th,
                    nnratio=nnratio, taken=None, uright=self.uright if stereo else None)

    def sfi(self, window=10, nnratio=0.9, ori=False):
        n = len(self.q)
        k1 = np.zeros(n, KP_DTYPE)
        k1["x"], k1["y"] = [q[0] for q in self.q], [q[1] for q in self.q]
        k1["angle"] = [q[4] for q in self.q]
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
        return dict(kind="sfi", kps=self.kps, desc=self.desc, bounds=IMG, kps1=k1,
                    desc1=np.array([q[3] for q in self.q], np.uint8).reshape(n, 32), prev=prev,
                    window=window, nnratio=nnratio, ori=ori)


def tie_groups(d, level=0, r=4.0):
    """Identical descriptors in different cells of one window, later index first in grid
    order (lower column, then lower row); two in one cell; a keypoint exactly on the window
    edge (|dx| == r) that is closer than the one inside."""
    h = r - 0.5
    d.group(level, [(h, 0.0, level, 0), (-h, 0.0, level, 0)])            # columns
    d.group(level, [(0.0, h, level, 0), (0.0, -h, level, 0)], dxy=(3.0, 0.0))  # rows
    d.group(level, [(0.25, 0.0, level, 4), (0.5, 0.125, level, 4)])      # one cell
    d.group(level, [(h, 0.0, level, 6), (-h, 0.0, level, 6), (0.0, 0.0, level, 30)])
    d.group(level, [(r, 0.0, level, 0), (1.0, 1.0, level, 20)])          # on the edge
    d.group(level, [(0.0, -r, level, 0), (1.0, 1.0, level, 20)])


def designed_last(seed=7):
    d = Designer(seed)
    tie_groups(d, 0, 7.0)
    # uRight: er == radius passes, either side of it, uRight <= 0 skips the test
    for off in (7.0, 7.5, 6.5, -7.0, -7.5, -6.5):
        d.group(0, [(1.0, 1.0, 0, 5, off)])
    d.group(0, [(1.0, 1.0, 0, 5, -9999.0)])      # uRight < 0: no test
    # a projection exactly on mnMaxX / mnMaxY (inside) and one eighth beyond (outside)
    for (u, v), (kx, ky) in (((640.0, 200.5), (634.0, 201.5)), ((640.125, 270.5), (634.0, 271.5)),
                             ((300.5, 480.0), (301.5, 474.0)), ((370.5, 480.125), (371.5, 474.0)),
                             ((0.0, 100.5), (6.0, 101.5)), ((-0.125, 170.5), (6.0, 171.5)),
                             ((100.5, 0.0), (101.5, 6.0)), ((170.5, -0.125), (171.5, 6.0))):
        D = d.rng.integers(0, 256, 32, dtype=np.uint8)
        d.kp(kx, ky, 0, flip(d.rng, D, 3))
        d.q.append((u, v, 0, D, 0.0, u - BF))
    return d.last(stereo=True)


def designed_local(seed=8):
    d = Designer(seed)
    # level-0 windows of r = 4 exactly (view_cos 0.9, th 1)
    tie_groups(d, 0, 4.0)
    # best / second straddling nnratio = 0.75 on equal and on different levels (query level 2:
    # r = 4 * 1.44, candidates of levels 1 and 2)
    for best, second in ((30, 40), (31, 40), (29, 40), (20, 20), (0, 0)):
        for lev2 in (2, 1):
            d.group(2, [(1.0, 0.5, 2, best), (-1.0, 0.5, lev2, second)])
            d.group(2, [(1.0, 0.5, lev2, second), (-1.0, 0.5, 2, best)])
    # levels 0 and 7
    d.group(7, [(3.0, 1.0, 7, 10), (-2.0, 1.0, 6, 30), (1.0, -2.0, 5, 0)])
    d.group(0, [(1.0, 1.0, 0, 10), (-1.0, 1.0, 1, 0)])
    # uRight on the edge r = 4
    for off in (4.0, 4.5, 3.5, -4.0, -4.5):
        d.group(0, [(1.0, 1.0, 0, 5, off)])
    return d.local(stereo=True)


def designed_sfi(seed=9):
    d = Designer(seed)
    tie_groups(d, 0, 10.0)
    d.group(0, [(2.0, 0.0, 0, 5), (-2.0, 0.0, 0, 5), (0.0, 2.0, 0, 30)])   # tied best
    d.group(0, [(2.0, 0.0, 0, 45), (-2.0, 0.0, 0, 50)])                    # 45 < 0.9 * 50 is false
    d.group(0, [(2.0, 0.0, 0, 44), (-2.0, 0.0, 0, 50)])
    d.group(0, [(2.0, 0.0, 0, 50)])
    d.group(0, [(2.0, 0.0, 0, 51)])
    d.group(0, [(2.0, 0.0, 1, 0)])                                         # level 1: not searched
    return d.sfi()


def rotation_scene(kind, hist, seed=11):
    """One keypoint per query; hist = [(bin, count)]: rot = 30 * bin + (-8..8) degrees."""
    d = Designer(seed, n_background=60)
    for b, cnt in hist:
        for _ in range(cnt):
            a = float(np.float32(d.rng.uniform(0, 360)))
            delta = 30.0 * b + float(d.rng.uniform(-8, 8))
            d.group(0, [(1.0, 1.0, 0, 3)], angle=a, q_angle=float(np.float32((a + delta) % 360)))
    assert d.spot <= 40
    return d.last(ori=True) if kind == "last" else d.sfi(ori=True)


HISTS = {"dominant": [(0, 25), (3, 2), (5, 3), (7, 1)],          # cut at 0.1 * 25: 3 stays, 2 goes
         "near_equal": [(2, 9), (4, 8), (6, 8), (9, 7), (12, 1)],
         "wrap": [(0, 6), (11, 5), (12, 5), (1, 4)]}


# ---- the margin filter and the three runners
def run_ref(s, variant=None):
    if s["kind"] == "sfi":
        return R.search_for_initialization(s["kps1"], s["desc1"], s["kps"], s["desc"], s["prev"],
                                           s["bounds"], s["window"], s["nnratio"], s["ori"],
                                           variant=variant)
    if s["kind"] == "last":
        return R.search_by_projection_lastframe(s["kps"], s["desc"], s["uright"], s["taken"],
                                                s["bounds"], SF, s["pts"], s["pdesc"], s["cam"],
                                                s["th"], s["ori"], variant=variant)
    return R.search_by_projection_local(s["kps"], s["desc"], s["uright"], s["taken"], s["bounds"],
                                        SF, s["mps"], s["mdesc"], s["th"], s["nnratio"],
                                        variant=variant)


_QUERY_KEYS = {"sfi": ("kps1", "desc1", "prev"), "last": ("pts", "pdesc"),
               "local": ("mps", "mdesc")}


def filtered(s):
    """Drop what an ambiguous decision names, repeat until none is left; at most 2 % go."""
    s = dict(s)
    nk0, nq0 = len(s["kps"]), len(s[_QUERY_KEYS[s["kind"]][0]])
    for _ in range(10):
        M = run_ref(s).margins
        if not M.ambiguous():
            break
        assert not M.who("call"), M.ambiguous()
        kk, qq = M.who("kp"), M.who("q")
        keep = np.ones(len(s["kps"]), bool)
        keep[kk] = False
        for key in ("kps", "desc", "uright", "taken"):
            if s.get(key) is not None:
                s[key] = np.ascontiguousarray(s[key][keep])
        keep = np.ones(len(s[_QUERY_KEYS[s["kind"]][0]]), bool)
        keep[qq] = False
        for key in _QUERY_KEYS[s["kind"]]:
            s[key] = np.ascontiguousarray(s[key][keep])
    assert not run_ref(s).margins.ambiguous()
    s["dropped"] = (nk0 - len(s["kps"]) + nq0 - len(s[_QUERY_KEYS[s["kind"]][0]])) \
        / max(nk0 + nq0, 1)
    assert s["dropped"] <= DROP_CAP, s["dropped"]
    return s


def run_oracle(o, s):
    if s["kind"] == "sfi":
        n, m, prev = o.search_for_initialization(s["kps1"], s["desc1"], s["kps"], s["desc"],
                                                 s["prev"], s["bounds"], s["window"],
                                                 s["nnratio"], s["ori"])
        return n, m, prev
    if s["kind"] == "last":
        c = s["cam"]
        cam = o.track_cam(c["Tcw"], c["Tlw"], c["fx"], c["fy"], c["cx"], c["cy"], c["bf"],
                          c["b"], c["mono"])
        n, m = o.search_by_projection_lastframe(s["kps"], s["desc"], s["uright"], s["taken"],
                                                s["bounds"], SF, s["pts"], s["pdesc"], cam,
                                                s["th"], s["ori"])
        return n, m, None
    n, m = o.search_by_projection_local(s["kps"], s["desc"], s["uright"], s["taken"],
                                        s["bounds"], SF, s["mps"], s["mdesc"], s["th"],
                                        s["nnratio"])
    return n, m, None


def run_gpu(s):
    from orb_slam2_test_amd import Frame, MapPointProjections, ORBmatcher
    b = [float(np.float32(v)) for v in s["bounds"]]
    F = Frame(s["kps"], s["desc"], *b)
    if s["kind"] == "sfi":
        prev = s["prev"].copy()
        F1 = Frame(s["kps1"], s["desc1"], *b)
        n, m = ORBmatcher(s["nnratio"], s["ori"]).SearchForInitialization(F1, F, prev,
                                                                          s["window"])
        return n, m, prev
    F.mvuRight, F.taken = s["uright"], s["taken"]
    if s["kind"] == "last":
        c = s["cam"]
        F.mTcw, F.fx, F.fy, F.cx, F.cy, F.mbf, F.mb = (c["Tcw"], c["fx"], c["fy"], c["cx"],
                                                       c["cy"], c["bf"], c["b"])
        last = Frame(s["kps"][:0], s["desc"][:0], *b)
        last.mTcw, last.points, last.point_desc = c["Tlw"], s["pts"], s["pdesc"]
        n, m = ORBmatcher(0.9, s["ori"]).SearchByProjection(F, last, s["th"], c["mono"])
        return n, m, None
    n, m = ORBmatcher(s["nnratio"]).SearchByProjection(
        F, MapPointProjections(s["mps"], s["mdesc"]), s["th"])
    return n, m, None


def check_equal(got, s, what):
    """got = (nmatches, match, prev or None) of the oracle or the kernels against the
    reference, exactly."""
    r = run_ref(s)
    n, m, prev = got
    assert np.array_equal(np.asarray(m, np.int64), r.match), what
    assert n == r.nmatches, what
    if s["kind"] == "sfi":
        assert np.array_equal(prev, r.prev), what
    return r


def scene_builders():
    """name -> builder.  Built lazily and once (see the tests' module fixtures)."""
    sc = {}
    for bn, b in (("img", IMG), ("dist", DIST)):
        sc["sfi_" + bn] = lambda b=b: sfi_scene(101, b)
        sc["last_" + bn] = lambda b=b: last_scene(102, b, stereo=True, mono=False)
        sc["local_" + bn] = lambda b=b: local_scene(103, b, stereo=True)
    sc["sfi_wide"] = lambda: sfi_scene(104, DIST, window=100, nnratio=0.6, ori=False)
    sc["local_th3"] = lambda: local_scene(105, DIST, th=3.0, nnratio=0.6)
    sc["last_forward"] = lambda: last_scene(106, IMG, mono=False, tz=-1.0, stereo=True, nq=130)
    sc["last_backward"] = lambda: last_scene(107, DIST, mono=False, tz=1.0, nq=130)
    sc["last_mono"] = lambda: last_scene(108, IMG, mono=True, tz=1.0, th=7.0, ori=False, nq=130)
    for frac in (0.33, 0.9):
        t = int(frac * 100)
        sc["last_taken%d" % t] = lambda frac=frac: last_scene(110, IMG, th=60.0,
                                                              taken_frac=frac, spread=20.0)
        sc["local_taken%d" % t] = lambda frac=frac: local_scene(111, IMG, th=10.0,
                                                                taken_frac=frac)
    sc["last_dense"] = lambda: last_scene(112, DIST, th=60.0, spread=20.0)
    sc["local_dense"] = lambda: local_scene(113, DIST, th=10.0)
    sc["designed_last"] = designed_last
    sc["designed_local"] = designed_local
    sc["designed_sfi"] = designed_sfi
    for h in HISTS:
        sc["rot_last_" + h] = lambda h=h: rotation_scene("last", HISTS[h])
        sc["rot_sfi_" + h] = lambda h=h: rotation_scene("sfi", HISTS[h])
    # counts at 0, 1 and one past the chunk / workgroup size
    for nk, nq in ((0, 5), (1, 1), (601, 0), (601, 1), (601, 65), (601, 129), (65, 259)):
        sc["last_%d_%d" % (nk, nq)] = lambda nk=nk, nq=nq: last_scene(120 + nq, IMG, nk=nk, nq=nq)
        sc["local_%d_%d" % (nk, nq)] = lambda nk=nk, nq=nq: local_scene(130 + nq, DIST, nk=nk,
                                                                        nq=nq, th=3.0)
        sc["sfi_%d_%d" % (nk, nq)] = lambda nk=nk, nq=nq: sfi_scene(140 + nq, IMG, n1=nq, n2=nk)
    return sc


_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = filtered(scene_builders()[name]())
    return _cache[name]


SCENE_NAMES = sorted(scene_builders())
