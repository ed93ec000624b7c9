"""A pure-Python statement of Optimizer::GlobalBundleAdjustemnt's walk over the map
(src/Optimizer.cc:105-246), of its store (:273-318) and of the map update of
LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:1056-1116), written from the
reference's text, loop by loop in the reference's order, over tests/ref_lba_map.py's RefLbaMap.
Converter::toSE3Quat / toCvMat are ref_lba_map's, the float cv::Mat product is
ref_loop_correct.cv_mul44 and the map-point move is ref_gba.correct_points.  Nothing here imports
the library or oracle/.

State added to the map: per slot mTcwGBA, mTcwBefGBA (float32 3x4) and mnBAGlobalForKF, per point
mPosGBA and mnBAGlobalForKF (0 by default, and for a slot that becomes live).

One departure from the reference, the library's (include/orbg.h): in the update a point whose
reference keyframe is -1, is dead, or carries loop_kf but was not visited stays where it is and is
counted, where the reference dereferences a null pointer or reads a stale mTcwBefGBA.

The scenes are written against the duck-typed interface (gba_window, gba_store, gba_update,
set_gba_state, gba_state, ...) so one function drives this class and the GPU adapter.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402
import ref_culling as RC  # noqa: E402
import ref_map_edit as RE  # noqa: E402
import ref_loop_correct as RL  # noqa: E402
import ref_lba_map as RB  # noqa: E402

F = np.float32
D = np.float64
HUBER_MONO = float(F(math.sqrt(5.99)))       # const float thHuber2D (Optimizer.cc:157)
HUBER_STEREO = float(F(math.sqrt(7.815)))    # const float thHuber3D (:158)
POSE_DTYPE, EDGE_DTYPE = RB.POSE_DTYPE, RB.EDGE_DTYPE


class UpdateError(ValueError):
    """what the library reports as ORBG_EINVAL from the update: a failing origin, a parent cycle,
    loop_kf == 0"""


def gba_window(M, robust, isg=None):
    """Optimizer.cc:113-246 over GetAllKeyFrames() / GetAllMapPoints() in slot / id order: a dict of
    kf_slots, poses, point_ids, points, edges, edge_feat and left_out (vbNotIncludedMP's count)"""
    isg = RB.inv_level_sigma2() if isg is None else isg
    d = getattr(M, "d", None)
    if d is None:
        raise RB.WindowError("nothing attached")
    # :140-152: the keyframes that are not bad; fixed iff mnId == 0
    kfs, max_kf_id = [], 0
    for s in sorted(M.kf):
        k = M.kf[s]
        if not k["live"] or k["bad"]:
            continue
        if s not in M.pose:
            raise RB.WindowError("a vertex keyframe has no pose")
        kfs.append(s)
        max_kf_id = max(max_kf_id, M.id_of(s))
    poses = np.zeros(len(kfs), POSE_DTYPE)
    for i, s in enumerate(kfs):
        poses["q"][i], poses["t"][i] = RB.se3quat_of(M.pose[s])
        poses["fixed"][i] = 1 if M.id_of(s) == 0 else 0
    pose_of = {s: i for i, s in enumerate(kfs)}
    # :160-246: the points that are not bad, their edges, removeVertex without one
    points, pts, edges, feat, left_out = [], [], [], [], 0
    for p in sorted(M.mp):
        if M.mp[p]["bad"]:
            continue
        mine = []
        for s, idx in M.observations(p):
            if M.kf[s]["bad"] or M.id_of(s) > max_kf_id:   # (the second never holds: s is not bad)
                continue
            if idx >= len(d["kps"][s]):
                raise RB.WindowError("feature index past the attached count")
            kp, ur, cam = d["kps"][s][idx], F(d["uright"][s][idx]), d["cams"][s]
            st = 0 if ur < 0 else 1
            e = np.zeros((), EDGE_DTYPE)
            e["point"], e["pose"], e["stereo"] = len(points), pose_of[s], st
            e["robust"], e["active"] = 1 if robust else 0, 1
            e["obs"] = (D(kp["x"]), D(kp["y"]), D(ur) if st else 0.0)
            e["inv_sigma2"] = D(isg[int(kp["octave"])])
            for key in ("fx", "fy", "cx", "cy", "bf"):
                e[key] = D(cam[key])
            e["huber_delta"] = HUBER_STEREO if st else HUBER_MONO
            mine.append((e, idx))
        if not mine:
            left_out += 1
            continue
        points.append(p)
        pts.append(M.mp[p]["pos"].astype(D))
        edges += [e for e, _ in mine]
        feat += [i for _, i in mine]
    return dict(kf_slots=np.array(kfs, np.int32), poses=poses, point_ids=np.array(points, np.int32),
                points=np.array(pts, D).reshape(-1, 3), edges=np.array(edges, EDGE_DTYPE).reshape(-1),
                edge_feat=np.array(feat, np.int32), left_out=left_out)


def gba_store(M, w, poses, points, loop_kf, cams=None):
    """Optimizer.cc:273-318: returns (keyframes written, points written)"""
    nkf = npt = 0
    for i, s in enumerate(w["kf_slots"]):
        s = int(s)
        if M.is_bad_kf(s):                                  # :279
            continue
        T = RB.tcw_of(poses["q"][i], poses["t"][i])
        if loop_kf == 0:
            M.set_pose(s, T)
            if cams is not None:
                cams["Tcw"][s] = T.reshape(12)
        else:
            M.TcwGBA[s] = T
            M.kf_gba[s] = int(loop_kf)
        nkf += 1
    written = []
    for i, p in enumerate(w["point_ids"]):
        p = int(p)
        if M.mp[p]["bad"]:                                  # :303
            continue
        X = np.asarray(points[i], D).astype(F)
        if loop_kf == 0:
            M.mp[p]["pos"] = X
            written.append(p)
        else:
            M.PosGBA[p] = X
            M.mp_gba[p] = int(loop_kf)
        npt += 1
    M.apply_normal_and_depth(written)       # UpdateNormalAndDepth reads the centres SetPose wrote
    return nkf, npt


def _m44(T):
    return np.concatenate([np.asarray(T, F).reshape(3, 4), np.array([[0, 0, 0, 1]], F)], 0)


def pose_inverse(M, s):
    """KeyFrame::GetPoseInverse(): [Rcw^T | Ow] with the stored Ow"""
    T = np.zeros((3, 4), F)
    T[:, :3] = M.pose[s][:, :3].T
    T[:, 3] = M.kf[s]["centre"]
    return T


def gba_update(M, loop_kf, origins, cams=None):
    """LoopClosing.cc:1056-1116: [visited, propagated, points from mPosGBA, points moved, points
    skipped by the departure, 0]"""
    import ref_gba as RG
    loop_kf = int(loop_kf)
    if loop_kf == 0:
        raise UpdateError("loop_kf is 0")
    for o in origins:
        k = M.kf.get(int(o))
        if k is None or not k["live"] or int(o) not in M.pose or M.kf_gba.get(int(o), 0) != loop_kf:
            raise UpdateError("origin")
    live = [s for s in M.kf if M.kf[s]["live"]]
    for s in live:                                          # a cycle of parents among live slots
        u, steps = s, 0
        while u is not None and u >= 0 and u in M.kf and M.kf[u]["live"]:
            u = M.kf[u]["parent"]
            steps += 1
            if steps > len(live) + 1:
                raise UpdateError("cycle")
    childs = {}
    for s in sorted(live):
        par = M.kf[s]["parent"]
        if par is not None and par >= 0:
            childs.setdefault(par, []).append(s)            # GetChilds(): pointer order = slot order
    queue, seen, visited, propagated = [], set(), [], 0
    for o in origins:
        if int(o) not in seen:
            seen.add(int(o))
            queue.append(int(o))
    while queue:
        s = queue.pop(0)
        Twc = _m44(pose_inverse(M, s))
        for c in childs.get(s, []):
            if c in seen:
                continue
            if M.kf_gba.get(c, 0) != loop_kf:
                Tchildc = RL.cv_mul44(_m44(M.pose[c]), Twc)
                M.TcwGBA[c] = RL.cv_mul44(Tchildc, _m44(M.TcwGBA[s]))[:3].copy()
                M.kf_gba[c] = loop_kf
                propagated += 1
            seen.add(c)
            queue.append(c)
        M.TcwBef[s] = np.array(M.pose[s], F)
        M.set_pose(s, M.TcwGBA[s])
        if cams is not None:
            cams["Tcw"][s] = np.asarray(M.TcwGBA[s], F).reshape(12)
        visited.append(s)
    vis = set(visited)
    n_gba = n_moved = n_skipped = 0
    for p in sorted(M.mp):
        m = M.mp[p]
        if m["bad"]:
            continue
        if M.mp_gba.get(p, 0) == loop_kf:
            m["pos"] = np.array(M.PosGBA[p], F)
            n_gba += 1
            continue
        r = m["ref"]
        if r is None or r < 0 or r not in M.kf or not M.kf[r]["live"]:
            n_skipped += 1
            continue
        if r not in vis:
            if M.kf_gba.get(r, 0) == loop_kf:
                n_skipped += 1
            continue
        m["pos"] = RG.correct_points([M.TcwBef[r]], [pose_inverse(M, r)], [0], [m["pos"]])[0]
        n_moved += 1
    return [len(visited), propagated, n_gba, n_moved, n_skipped, 0]


class RefGbaMap(RB.RefLbaMap):
    """the duck-typed interface of the scenes below over the reference model"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.TcwGBA, self.TcwBef, self.kf_gba = {}, {}, {}
        self.PosGBA, self.mp_gba = {}, {}

    def set_keyframe(self, slot, points, octaves=None, centre=(0.0, 0.0, 0.0), root=False,
                     bad=False):
        k = self.kf.get(slot)
        if k is None or not k["live"]:
            self.kf_gba[slot] = 0
        super().set_keyframe(slot, points, octaves, centre, root, bad)

    def set_gba_state(self, first_slot=0, TcwGBA=None, TcwBef=None, kf_gba=None, first_point=0,
                      PosGBA=None, mp_gba=None):
        for dst, src, first in ((self.TcwGBA, TcwGBA, first_slot), (self.TcwBef, TcwBef, first_slot),
                                (self.PosGBA, PosGBA, first_point)):
            if src is not None:
                for i, v in enumerate(src):
                    dst[first + i] = np.array(v, F)
        for dst, src, first in ((self.kf_gba, kf_gba, first_slot), (self.mp_gba, mp_gba, first_point)):
            if src is not None:
                for i, v in enumerate(src):
                    dst[first + i] = int(v)

    def gba_state(self, nkf, npts):
        out = dict(TcwGBA=np.zeros((nkf, 3, 4), F), TcwBefGBA=np.zeros((nkf, 3, 4), F),
                   kf_ba_global=np.zeros(nkf, np.int32), PosGBA=np.zeros((npts, 3), F),
                   mp_ba_global=np.zeros(npts, np.int32))
        for s in range(nkf):
            if s in self.TcwGBA:
                out["TcwGBA"][s] = self.TcwGBA[s]
            if s in self.TcwBef:
                out["TcwBefGBA"][s] = self.TcwBef[s]
            out["kf_ba_global"][s] = self.kf_gba.get(s, 0)
        for p in range(npts):
            if p in self.PosGBA:
                out["PosGBA"][p] = self.PosGBA[p]
            out["mp_ba_global"][p] = self.mp_gba.get(p, 0)
        return out

    def gba_window(self, robust):
        return gba_window(self, robust)

    def gba_store(self, w, poses, points, loop_kf, cams=None):
        return gba_store(self, w, poses, points, loop_kf, cams)

    def gba_update(self, loop_kf, origins, cams=None):
        return gba_update(self, loop_kf, origins, cams)


def state_bytes(M, nkf, npts):
    """the float state as bytes: poses, has-pose, centres, point records, the GBA state"""
    T, has, ids, c = M.get_poses(nkf)
    g = M.gba_state(nkf, npts)
    return ([np.asarray(T, F).tobytes(), np.asarray(has, bool).tobytes(),
             np.asarray(ids, np.int32).tobytes(), np.asarray(c, F).tobytes(),
             M.records(npts).tobytes()] + [np.ascontiguousarray(g[k]).tobytes() for k in sorted(g)])


def window_lists(w):
    """(kf_slots, fixed flags, point_ids, the (point id, slot, feature, stereo) edges, left out)"""
    e = w["edges"]
    return (w["kf_slots"].tolist(), w["poses"]["fixed"].tolist(), w["point_ids"].tolist(),
            [(int(w["point_ids"][e["point"][k]]), int(w["kf_slots"][e["pose"][k]]),
              int(w["edge_feat"][k]), int(e["stereo"][k])) for k in range(len(e))],
            int(w["left_out"]))


def big_rot(rng):
    """a rotation far from identity"""
    w = rng.normal(size=3)
    return RL._rot(w / np.linalg.norm(w) * rng.uniform(0.6, 3.0))


def rand_pose(rng, Rm=None, scale=1.0):
    Rm = big_rot(rng) if Rm is None else Rm
    return np.concatenate([Rm, rng.uniform(-scale, scale, (3, 1))], 1).astype(F)


# ---------------------------------------------------------------------------
# a small hand scene whose lists are literals in tests/test_gba_map_ref.py
# ---------------------------------------------------------------------------
HAND_K, HAND_CAP, HAND_POINTS = RB.HAND_K, RB.HAND_CAP, 16


def hand_window(M, stereo_slots=(1,)):
    """Slot 2 carries mnId 0 (fixed; the slot does not decide it), slot 3 is bad, slot 4 is dead,
    slot 5 has no points.  Point 6 is bad, point 7 is seen by nobody, point 8 by the bad slot only
    (both left out, as are the other eight unobserved points), point 9 by slot 1 and the bad slot
    (one edge).  Slot 1 is stereo: its
    features 0, 3, ... carry mvuRight."""
    R._plain_points(M, HAND_POINTS)
    M.set_point_bad(6)
    M.set_keyframe(0, [0, 1, 2], root=True)
    M.set_keyframe(1, [2, 1, 9, 3])
    M.set_keyframe(2, [3, 0, 6])
    M.set_keyframe(3, [8, 9, 0])
    M.set_keyframe(4, [0, 1])
    M.set_keyframe(5, [])
    RB.hand_attach(M, stereo_slots=stereo_slots)
    M.set_poses([0, 1, 2, 3, 4, 5], [RL.eye_pose((0.5 * s, 0.0, 0.0)) for s in range(6)],
                [10, 11, 0, 13, 14, 15])
    M.set_keyframe(3, [8, 9, 0], bad=True)
    M.erase_keyframe(4)
    return M.gba_window(True)


HAND_WINDOW = ([0, 1, 2, 5], [0, 0, 1, 0], [0, 1, 2, 3, 9],
               [(0, 0, 0, 0), (0, 2, 1, 0), (1, 0, 1, 0), (1, 1, 1, 0), (2, 0, 2, 0), (2, 1, 0, 1),
                (3, 1, 3, 1), (3, 2, 0, 0), (9, 1, 2, 0)], 10)


def hand_tree_build(M, loop_kf=7):
    """Origin 0 (in the BA) with children 1 (in the BA) and 2 (not); 3 below 2 (not), 4 below 3 (in
    the BA: keeps its own mTcwGBA); 5 is dead with 6 below it (not visited).  Points: 0 in the BA;
    1 outside with reference 1; 2 with the propagated reference 3; 3 with reference 6 (unvisited,
    carries loop_kf): skipped; 4 with a dead reference: skipped; 5 with reference -1: skipped; 6
    is bad; 7 with reference 6 after its mark is cleared stays uncounted (see the test)."""
    rng = np.random.default_rng(41)
    pos = [(0.5 * i, 0.25, 4.0 + 0.125 * i) for i in range(8)]
    M.set_points(0, pos, [False] * 6 + [True, False], [[0] * 32] * 8, [0, 1, 3, 6, 5, -1, 0, 6])
    for s in range(7):
        M.set_keyframe(s, [], root=(s == 0))
    for s, par in ((1, 0), (2, 0), (3, 2), (4, 3), (6, 5)):
        M.set_parent(s, par)
    M.set_parent(5, 1)
    M.set_poses(list(range(7)), [rand_pose(rng) for _ in range(7)])
    M.erase_keyframe(5)
    gba = [rand_pose(rng) for _ in range(7)]
    M.set_gba_state(0, TcwGBA=gba, kf_gba=[loop_kf, loop_kf, 0, 0, loop_kf, 0, loop_kf],
                    first_point=0, PosGBA=[(9.0, 8.0, 7.0)] * 8,
                    mp_gba=[loop_kf, 0, 0, 0, 0, 0, loop_kf, 0])


def hand_tree(M, loop_kf=7):
    hand_tree_build(M, loop_kf)
    return M.gba_update(loop_kf, [0])


HAND_TREE = [5, 2, 1, 2, 4, 0]


# ---------------------------------------------------------------------------
# the window scene of tests/test_gpu_gba_map.py: max_keyframes 300, max_points 4200
# ---------------------------------------------------------------------------
WIN_K, WIN_CAP, WIN_POINTS, WIN_NATT = 300, 8, 4200, 260
WIN_ROWS = {3: [0, 1, 2, 2046, 2047, 4095], 5: [0, 1, 103, 2048, 2049, 4096, 100],
            7: [102, 103, 2, 2050], 11: [], 254: [2050, 3, 4095], 255: [3, 4, 4097],
            256: [4, 5, 2046], 257: [5, 0], 258: [1, 4096, 4097]}
WIN_BAD_SLOT, WIN_DEAD_SLOT, WIN_STEREO = 7, 9, (5, 255, 258)


def win_attach_data(stereo=True):
    """keypoint idx of slot s at (s + 1.5 idx, 100 + idx), octave 7 for odd idx else 0; in a
    stereo slot every third feature has mvuRight = x - 2; camera s has fx = 500 + s / 4"""
    kps, ur = [], []
    for s in range(WIN_NATT):
        kp = np.zeros(WIN_CAP, RE.KP_DTYPE)
        kp["x"], kp["y"] = s + 1.5 * np.arange(WIN_CAP), 100 + np.arange(WIN_CAP)
        kp["octave"] = np.where(np.arange(WIN_CAP) % 2 == 1, 7, 0)
        u = np.full(WIN_CAP, -1, F)
        if stereo and s in WIN_STEREO:
            u[::3] = kp["x"][::3] - 2
        kps.append(kp)
        ur.append(u)
    cams = np.zeros(WIN_NATT, RE.FRUSTUM_DTYPE)
    for s in range(WIN_NATT):
        cams[s] = RE.camera((0.0, 0.0, 0.0))
        cams["fx"][s], cams["fy"][s] = 500 + 0.25 * s, 510 + 0.25 * s
    kd = [np.zeros((WIN_CAP, 32), np.uint8)] * WIN_NATT
    return dict(kdesc=kd, kps=kps, uright=ur, cams=cams)


def win_scene(M, stereo=True):
    """Live slots 3, 5, 7 (bad), 11 (no points) and 254-258, slot 9 dead; mnId 0 on slot 3.  Good
    points with edges at ids 0-5, 103, 2046-2050 and 4095-4097; 100 is bad, 101 is seen by
    nobody, 102 by the bad slot alone, 103 and 2 by a good and the bad slot.  Rotations of about
    170 degrees about x, y and z on slots 254-256 take Eigen's three diagonal branches."""
    rng = np.random.default_rng(77)
    pos = rng.uniform(-3.0, 3.0, (WIN_POINTS, 3)) + (0.0, 0.0, 30.0)
    first = {}
    for s in sorted(WIN_ROWS):
        for p in WIN_ROWS[s]:
            first.setdefault(p, s)
    ref = [first.get(p, -1) for p in range(WIN_POINTS)]
    bad = [p not in first and p != 101 for p in range(WIN_POINTS)]     # the unused ids are bad
    M.set_points(0, pos, bad, np.zeros((WIN_POINTS, 32), np.uint8), ref)
    M.set_point_bad(100)
    M.set_keyframe(WIN_DEAD_SLOT, [0, 1])
    for s, row in WIN_ROWS.items():
        M.set_keyframe(s, row, octaves=[(7 if i % 2 else 0) for i in range(len(row))], root=(s == 3))
    M.attach(win_attach_data(stereo))
    slots = sorted(WIN_ROWS) + [WIN_DEAD_SLOT]
    Ts = []
    for s in slots:
        Rm = None
        if s in (254, 255, 256):
            axis = np.zeros(3)
            axis[s - 254] = math.radians(170.0) + 0.01 * (s - 254)
            Rm = RL._rot(axis)
        Ts.append(rand_pose(rng, Rm))
    M.set_poses(slots, Ts, [0 if s == 3 else s + 10 for s in slots])
    M.set_keyframe(WIN_BAD_SLOT, WIN_ROWS[WIN_BAD_SLOT], bad=True,
                   octaves=[(7 if i % 2 else 0) for i in range(len(WIN_ROWS[WIN_BAD_SLOT]))])
    M.erase_keyframe(WIN_DEAD_SLOT)


WIN_COUNTS = [8, 15, 26, 2]      # poses, points, edges, left out (101 and 102)


def store_estimates(w, seed=5):
    """estimates chosen by hand: unit quaternions far from identity, translations and positions
    with full mantissas"""
    rng = np.random.default_rng(seed)
    poses = np.array(w["poses"])
    q = rng.normal(size=(len(poses), 4))
    q[:, 3] = np.abs(q[:, 3])
    poses["q"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses["t"] = rng.uniform(-0.5, 0.5, (len(poses), 3))
    points = rng.uniform(-4.0, 4.0, w["points"].shape) + (0.0, 0.0, 25.0)
    return poses, points


# ---------------------------------------------------------------------------
# the update scene: a tree over 330 slots
# ---------------------------------------------------------------------------
TREE_K, TREE_CAP, TREE_POINTS = 330, 4, 24
TREE_ORIGINS = [0, 5]
TREE_BA = [0, 1, 2, 3, 5, 6, 7, 13]             # in the BA; 13 hangs below the non-BA slot 9
TREE_DEAD, TREE_BAD = 15, 100


def tree_parents():
    """0 -> 1 -> 2 -> 3 and 5 -> 6 -> 7 in the BA.  Outside it: 8 below 1 (a run of 1); 9 -> 10
    below 2 with 11 and 12 both below 10 (runs of 3, a branch); 13 (in the BA) below 9 and 14
    below 13; the dead 15 below 2 with 16 and 17 below it; the chain 70 .. 329 below 7 (a run of
    260, 100 flagged bad) with 20 -> 21 -> 22 branching off 136, the 67th of the chain (a run of
    70, its slots lower than their parents')."""
    par = {1: 0, 2: 1, 3: 2, 6: 5, 7: 6, 8: 1, 9: 2, 10: 9, 11: 10, 12: 10, 13: 9, 14: 13,
           15: 2, 16: 15, 17: 16, 70: 7, 20: 136, 21: 20, 22: 21}
    for s in range(71, 330):
        par[s] = s - 1
    return par


def tree_scene(M, loop_kf):
    rng = np.random.default_rng(91)
    par = tree_parents()
    slots = sorted(set(par) | set(TREE_ORIGINS))
    ref = [1, 2, 6, 13, 8, 10, 22, 329, 100, 14, 17, 16, 15, -1, 3, 0]
    npt = len(ref)
    pos = rng.uniform(-2.0, 2.0, (TREE_POINTS, 3)) + (0.0, 0.0, 12.0)
    refs = ref + [0] * (TREE_POINTS - npt)
    M.set_points(0, pos, [False] * TREE_POINTS, np.zeros((TREE_POINTS, 32), np.uint8), refs)
    M.set_point_bad(15)
    for s in slots:
        M.set_keyframe(s, [], root=(s in TREE_ORIGINS))
    for s, p in par.items():
        M.set_parent(s, p)
    small = lambda: np.concatenate([RL._rot(rng.normal(size=3) * 0.3),     # noqa: E731
                                    rng.uniform(-1.0, 1.0, (3, 1))], 1).astype(F)
    M.set_poses(slots, [small() for _ in slots])
    M.set_keyframe(TREE_BAD, [], bad=True)
    M.erase_keyframe(TREE_DEAD)
    tree_ba_state(M, loop_kf, rng, also=(17,))
    return slots


def tree_ba_state(M, loop_kf, rng, also=()):
    """what a global BA with loop_kf leaves: mTcwGBA and the mark on TREE_BA (and `also`), mPosGBA
    and the mark on points 0, 1 and the bad point 15"""
    for s in list(TREE_BA) + list(also):
        T = np.concatenate([RL._rot(rng.normal(size=3) * 0.3), rng.uniform(-1.0, 1.0, (3, 1))], 1)
        M.set_gba_state(s, TcwGBA=[T.astype(F)], kf_gba=[loop_kf])
    for p in (0, 1, 15):
        M.set_gba_state(first_point=p, PosGBA=[rng.uniform(-2.0, 2.0, 3) + (0.0, 0.0, 12.0)],
                        mp_gba=[loop_kf])


# visited: 8 BA + 8, 9 .. 12, 14 + 260 + 3; propagated: all of those outside the BA
TREE_COUNTS = [8 + 6 + 260 + 3, 6 + 260 + 3, 2, 17, 3, 0]


# ---------------------------------------------------------------------------
# a bundle adjustment problem (poses, points, edges in the library's record layouts) as a map
# ---------------------------------------------------------------------------
def build_ba_map(M, poses, points, edges, nkf_cap, extra_bad=0):
    """Keyframe s = pose s (mnId s, so pose 0 is fixed), its features the edges of pose s in edge
    order; the octave is the level whose mvInvLevelSigma2 is nearest the edge's.  Slot s + 1's
    parent is s.  extra_bad: that many further keyframes, flagged bad (outside the BA, inside the
    spanning tree), each with two points of its own."""
    isg = np.array([float(v) for v in RB.inv_level_sigma2()])
    nkf, npt = len(poses), len(points)
    rows = {s: [] for s in range(nkf + extra_bad)}
    kps = {s: [] for s in range(nkf + extra_bad)}
    ur = {s: [] for s in range(nkf + extra_bad)}
    ref = [-1] * (npt + 2 * extra_bad)
    for e in edges:
        s, p = int(e["pose"]), int(e["point"])
        kp = np.zeros((), RE.KP_DTYPE)
        kp["x"], kp["y"] = e["obs"][0], e["obs"][1]
        kp["octave"] = int(np.argmin(np.abs(isg - float(e["inv_sigma2"]))))
        rows[s].append(p)
        kps[s].append(kp)
        ur[s].append(F(e["obs"][2]) if e["stereo"] else F(-1))
        if ref[p] < 0:
            ref[p] = s
    pos = [np.asarray(x, D).astype(F) for x in points]
    rng = np.random.default_rng(3)
    for k in range(extra_bad):
        s = nkf + k
        for j in range(2):
            p = npt + 2 * k + j
            rows[s].append(p)
            kp = np.zeros((), RE.KP_DTYPE)
            kp["x"], kp["y"] = 100.0 + j, 50.0 + k
            kps[s].append(kp)
            ur[s].append(F(-1))
            ref[p] = s
            pos.append((rng.uniform(-1.0, 1.0, 3) + (0.0, 0.0, 20.0)).astype(F))
    M.set_points(0, pos, [False] * len(pos), np.zeros((len(pos), 32), np.uint8), ref)
    cams = np.zeros(nkf_cap, RE.FRUSTUM_DTYPE)
    e0 = edges[0]
    for s in range(nkf_cap):
        cams[s] = RE.camera((0.0, 0.0, 0.0))
        for key in ("fx", "fy", "cx", "cy", "bf"):
            cams[key][s] = e0[key]
    natt = nkf + extra_bad
    Ts = [RB.tcw_of(poses["q"][s], poses["t"][s]) for s in range(nkf)]
    for k in range(extra_bad):
        T = np.array(Ts[nkf - 1])
        T[:, 3] += F(0.25 * (k + 1))
        Ts.append(T)
    for s in range(natt):
        M.set_keyframe(s, rows[s], octaves=[int(k["octave"]) for k in kps[s]], root=(s == 0))
        if s:
            M.set_parent(s, s - 1)
    M.attach(dict(kdesc=[np.zeros((len(rows[s]), 32), np.uint8) for s in range(natt)],
                  kps=[np.array(kps[s], RE.KP_DTYPE).reshape(-1) for s in range(natt)],
                  uright=[np.array(ur[s], F).reshape(-1) for s in range(natt)], cams=cams))
    M.set_poses(list(range(natt)), Ts)
    for k in range(extra_bad):
        s = nkf + k
        M.set_keyframe(s, rows[s], octaves=[int(k_["octave"]) for k_ in kps[s]], bad=True)
    M.apply_normal_and_depth(range(len(pos)))
    return natt, len(pos)
