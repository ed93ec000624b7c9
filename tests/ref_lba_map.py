"""A pure-Python statement of Optimizer::LocalBundleAdjustment's walk over the map
(src/Optimizer.cc:633-851) and of its write-back (:907-978), written from the reference's text,
keyframe by keyframe and point by point in the reference's loop order, over
tests/ref_loop_correct.py's RefLoopMap (poses, rows, observations, _drop, mp_set_bad).  Nothing
here imports the library or oracle/.

Converter::toSE3Quat and Converter::toCvMat(SE3Quat) are float64 NumPy scalars in the operation
order of Eigen's Quaterniond(Matrix3d) / toRotationMatrix, so their results are what an IEEE
implementation of the same order gives, bit for bit.

The scenes are written against the duck-typed interface (lba_window, lba_apply, ...) so one
function drives this class and the GPU adapter.
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

F = np.float32
D = np.float64
HUBER_MONO = float(F(math.sqrt(5.991)))      # const float thHuberMono (Optimizer.cc:758)
HUBER_STEREO = float(F(math.sqrt(7.815)))    # const float thHuberStereo (:759)
CHI2_MONO, CHI2_STEREO = 5.991, 7.815

# the library's record layouts (include/orbg.h), restated so that this file stands alone
POSE_DTYPE = np.dtype([("q", "<f8", 4), ("t", "<f8", 3), ("fixed", "<i4"), ("pad", "<i4")])
EDGE_DTYPE = np.dtype([("point", "<i4"), ("pose", "<i4"), ("stereo", "<i4"), ("robust", "<i4"),
                       ("active", "<i4"), ("pad", "<i4"), ("obs", "<f8", 3),
                       ("inv_sigma2", "<f8"), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"),
                       ("cy", "<f8"), ("bf", "<f8"), ("huber_delta", "<f8")])


def inv_level_sigma2(nlevels=8, factor=1.2):
    """ORBextractor's mvInvLevelSigma2: 1.0f / (mvScaleFactor[i] * mvScaleFactor[i]) in float"""
    return [F(F(1.0) / F(s * s)) for s in R.scale_factors(nlevels, factor)]


def se3quat_of(T):
    """Converter::toSE3Quat of a float32 3x4 pose: (q [4] as x, y, z, w, t [3]) float64 --
    Eigen's Quaterniond(Matrix3d) (the trace branch, else the largest diagonal entry), w >= 0,
    one normalisation"""
    T = np.asarray(T, F).reshape(3, 4)
    Rm = [[D(T[i, j]) for j in range(3)] for i in range(3)]
    q = [D(0)] * 4
    tr = Rm[0][0] + Rm[1][1] + Rm[2][2]
    if tr > 0:
        s = np.sqrt(tr + D(1.0))
        q[3] = D(0.5) * s
        s = D(0.5) / s
        q[0] = (Rm[2][1] - Rm[1][2]) * s
        q[1] = (Rm[0][2] - Rm[2][0]) * s
        q[2] = (Rm[1][0] - Rm[0][1]) * s
    else:
        i = 0
        if Rm[1][1] > Rm[0][0]:
            i = 1
        if Rm[2][2] > Rm[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = np.sqrt(Rm[i][i] - Rm[j][j] - Rm[k][k] + D(1.0))
        q[i] = D(0.5) * s
        s = D(0.5) / s
        q[3] = (Rm[k][j] - Rm[j][k]) * s
        q[j] = (Rm[j][i] + Rm[i][j]) * s
        q[k] = (Rm[k][i] + Rm[i][k]) * s
    if q[3] < 0:
        q = [-v for v in q]
    nq = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([v / nq for v in q], D), T[:, 3].astype(D)


def tcw_of(q, t):
    """Converter::toCvMat(SE3Quat): Eigen's toRotationMatrix in double, every element cast to
    float: float32 [3, 4]"""
    q = [D(v) for v in q]
    tx, ty, tz = D(2) * q[0], D(2) * q[1], D(2) * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    Rm = [[D(1) - (tyy + tzz), txy - twz, txz + twy],
          [txy + twz, D(1) - (txx + tzz), tyz - twx],
          [txz - twy, tyz + twx, D(1) - (txx + tyy)]]
    T = np.zeros((3, 4), F)
    for i in range(3):
        for j in range(3):
            T[i, j] = F(Rm[i][j])
        T[i, 3] = F(D(t[i]))
    return T


class WindowError(ValueError):
    """what the library reports as ORBG_EINVAL: a dead slot, nothing attached, a window keyframe
    without a pose, a feature index past the attached count"""


def lba_window(M, slot, isg=None):
    """Optimizer.cc:635-851 over the map: a dict of kf_slots (local, then fixed), nlocal,
    point_ids, poses POSE_DTYPE, points float64 [n, 3], edges EDGE_DTYPE and edge_feat.  The
    attached keyframe data is M.d (kps, uright, cams: ref_map_edit's datasets)."""
    isg = inv_level_sigma2() if isg is None else isg
    k = M.kf.get(slot)
    if k is None or not k["live"]:
        raise WindowError("dead slot")
    d = getattr(M, "d", None)
    if d is None:
        raise WindowError("nothing attached")
    # lLocalKeyFrames: pKF, then GetVectorCovisibleKeyFrames(); every one is marked local, the
    # bad ones are not listed (:639-648)
    local, marked_local = [slot], {slot}
    for t, _ in M.ordered(slot):
        marked_local.add(t)
        if not M.kf[t]["bad"] and M.kf[t]["live"]:
            local.append(t)
    # lLocalMapPoints (:651-667)
    points, seen = [], set()
    for s in local:
        for p in M.kf[s]["points"]:
            if p >= 0 and not M.mp[p]["bad"] and p not in seen:
                points.append(p)
                seen.add(p)
    # lFixedCameras (:670-686)
    fixed, marked_fixed = [], set()
    for p in points:
        for s, _ in M.observations(p):
            if s not in marked_local and s not in marked_fixed:
                marked_fixed.add(s)
                if not M.kf[s]["bad"]:
                    fixed.append(s)
    kfs = local + fixed
    for s in kfs:
        if s not in M.pose:
            raise WindowError("a window keyframe has no pose")
    poses = np.zeros(len(kfs), POSE_DTYPE)
    for i, s in enumerate(kfs):
        poses["q"][i], poses["t"][i] = se3quat_of(M.pose[s])
        poses["fixed"][i] = 1 if i >= len(local) or M.id_of(s) == 0 else 0
    pose_of = {s: i for i, s in enumerate(kfs)}
    pts = np.array([M.mp[p]["pos"].astype(D) for p in points], D).reshape(-1, 3)
    edges, feat = [], []
    for i, p in enumerate(points):
        for s, idx in M.observations(p):
            if M.kf[s]["bad"]:
                continue
            if idx >= len(d["kps"][s]):
                raise WindowError("feature index past the attached count")
            kp, ur, cam = d["kps"][s][idx], F(d["uright"][s][idx]), d["cams"][s]
            st = 0 if ur < 0 else 1
            e = np.zeros((), EDGE_DTYPE)
            e["point"], e["pose"], e["stereo"], e["robust"], e["active"] = i, pose_of[s], st, 1, 1
            e["obs"] = (D(kp["x"]), D(kp["y"]), D(ur) if st else 0.0)
            e["inv_sigma2"] = D(isg[int(kp["octave"])])
            for key in ("fx", "fy", "cx", "cy", "bf"):
                e[key] = D(cam[key])
            e["huber_delta"] = HUBER_STEREO if st else HUBER_MONO
            edges.append(e)
            feat.append(idx)
    return dict(kf_slots=np.array(kfs, np.int32), nlocal=len(local),
                point_ids=np.array(points, np.int32), poses=poses, points=pts,
                edges=np.array(edges, EDGE_DTYPE).reshape(-1), edge_feat=np.array(feat, np.int32))


def erase_observation(M, p, s):
    """MapPoint::EraseObservation(pKF) (MapPoint.cc:159-193) on the table; True: the point went
    bad"""
    obs = dict(M.observations(p))
    if s not in obs:
        return False
    nobs = M.n_obs(p) - (2 if M.feat(s, obs[s]) & RC.FEAT_STEREO else 1)
    M._drop(s, obs[s])                                  # mObservations.erase(pKF) on the table
    if M.mp[p]["ref"] == s:
        rest = M.observations(p)
        M.mp[p]["ref"] = rest[0][0] if rest else -1     # mObservations.begin()->first
    if nobs <= 2:
        M.mp_set_bad(p)
        return True
    return False


def lba_apply(M, w, poses, points, erase, cams=None):
    """Optimizer.cc:943-978: the erasures (vpEdgesMono first, then vpEdgesStereo, each in edge
    order), SetPose of the local keyframes, SetWorldPos + UpdateNormalAndDepth of the local
    points.  cams: FRUSTUM records per slot whose Tcw follows the local keyframes' poses.
    Returns (observations erased, points gone bad)."""
    nerased = nbad = 0
    for st in (0, 1):
        for e in range(len(w["edges"])):
            if not erase[e] or int(w["edges"]["stereo"][e] != 0) != st:
                continue
            s = int(w["kf_slots"][w["edges"]["pose"][e]])
            p = int(w["point_ids"][w["edges"]["point"][e]])
            if M.mp[p]["bad"] or dict(M.observations(p)).get(s) != int(w["edge_feat"][e]):
                continue                                # gone with the point earlier in the call
            # EraseMapPointMatch(pMP) is EraseObservation's _drop: one table holds both sides
            nerased += 1
            nbad += erase_observation(M, p, s)
    for i in range(w["nlocal"]):
        s = int(w["kf_slots"][i])
        T = tcw_of(poses["q"][i], poses["t"][i])
        M.set_pose(s, T)
        if cams is not None:
            cams["Tcw"][s] = T.reshape(12)
    for i, p in enumerate(w["point_ids"]):
        M.mp[int(p)]["pos"] = np.asarray(points[i], D).astype(F)
    M.apply_normal_and_depth([int(p) for p in w["point_ids"]])
    return nerased, nbad


def erase_flags(poses, points, edges, ba_optimize, ba_system, lba_outlier_pass):
    """Optimizer.cc:856-937 with tests/ref_optim.py's optimiser: (poses, points, erase, the
    smallest |chi2 / threshold - 1| of any decision)"""
    P5, X5, _ = ba_optimize(poses, points, edges, 5)
    active, margin = lba_outlier_pass(P5, X5, edges)
    sy5 = ba_system(P5, X5, edges)
    e2 = np.array(edges)
    e2["active"], e2["robust"] = active, 0
    P10, X10, _ = ba_optimize(P5, X5, e2, 10)
    sy10 = ba_system(P10, X10, e2)
    thr = np.where(edges["stereo"] != 0, CHI2_STEREO, CHI2_MONO)
    chi = np.where(active != 0, sy10["chi2"], sy5["chi2"])
    erase = (chi > thr) | ~sy10["depth_ok"]
    return P10, X10, erase.astype(np.uint8), min(margin, float(np.abs(chi / thr - 1).min()))


class RefLbaMap(RL.RefLoopMap):
    """the duck-typed interface of the scenes below over the reference model"""

    def lba_window(self, slot):
        return lba_window(self, slot)

    def lba_apply(self, w, poses, points, erase, cams=None):
        return lba_apply(self, w, poses, points, erase, cams)


def state(M, nkf, npts):
    """everything discrete the tests compare after a call"""
    return RC.state(M, nkf, npts)


# ---------------------------------------------------------------------------
# hand scenes: tables alone, K <= 8, cap <= 32, at least 15 shared points per connected pair
# ---------------------------------------------------------------------------
HAND_K, HAND_CAP, HAND_POINTS = 8, 32, 48


def hand_attach(M, stereo_slots=()):
    """keypoint idx of slot s at (10 s + idx, 100 + idx), octave idx % 8; in a stereo slot every
    third feature has mvuRight = x - 2; camera s has fx = 500 + s, fy = 510 + s"""
    kps, ur = [], []
    for s in range(HAND_K):
        kp = np.zeros(HAND_CAP, RE.KP_DTYPE)
        kp["x"], kp["y"] = 10 * s + np.arange(HAND_CAP), 100 + np.arange(HAND_CAP)
        kp["octave"] = np.arange(HAND_CAP) % 8
        u = np.full(HAND_CAP, -1, F)
        if s in stereo_slots:
            u[::3] = kp["x"][::3] - 2
        kps.append(kp)
        ur.append(u)
    cams = np.zeros(HAND_K, RE.FRUSTUM_DTYPE)
    for s in range(HAND_K):
        cams[s] = RE.camera((0.5 * s, 0.0, 0.0))
        cams["fx"][s], cams["fy"][s] = 500 + s, 510 + s
    kd = [np.zeros((HAND_CAP, 32), np.uint8)] * HAND_K
    M.attach(dict(kdesc=kd, kps=kps, uright=ur, cams=cams))


def hand_main(M):
    """cur = 2.  Points 0..15 are in rows 2, 3, 1 and 6: slots 3 and 1 tie at weight 16 (the tie
    goes to the higher slot), slot 6 has 17 (point 21 too) and is bad: it heads the ordered list,
    appears in neither part and its edges are dropped.  Row 2 holds the points in descending
    order, then the bad point 30, a hole and point 21.  Point 20 is in rows 3 and 1, not in row
    2: listed at row 3.  Slot 5 sees point 15 (the first listed) and slot 4 point 14 (the
    second): the fixed part is [5, 4].  Slot 0 (bad, not covisible) sees point 13: nowhere.
    Slot 1 has mnId 0: fixed inside the local part.  Slots 1 and 5 are stereo."""
    R._plain_points(M, HAND_POINTS)
    M.set_point_bad(30)
    A = list(range(16))
    M.set_keyframe(0, [13], root=True)
    M.set_keyframe(1, [20] + A)
    M.set_keyframe(2, A[::-1] + [30, -1, 21])
    M.set_keyframe(3, A + [20, 22])
    M.set_keyframe(4, [14, 40])
    M.set_keyframe(5, [15, 22])
    M.set_keyframe(6, A + [21])
    for s in (1, 5):
        M.set_keyframe_features(s, [RC.FEAT_STEREO if i % 3 == 0 else 0 for i in range(17)])
    hand_attach(M, stereo_slots=(1, 5))
    M.set_poses(list(range(7)), [RL.eye_pose((0.5 * s, 0.0, 0.0)) for s in range(7)],
                [10, 0, 12, 13, 14, 15, 16])
    for s in range(7):
        M.update_connections(s)
    M.set_keyframe(6, A + [21], bad=True)
    M.set_keyframe(0, [13], root=True, bad=True)
    return M.ordered(2), window_lists(M.lba_window(2))


def window_lists(w):
    """(kf_slots, nlocal, fixed flags, point_ids, the (point id, slot, feature, stereo) edges)"""
    e = w["edges"]
    return (w["kf_slots"].tolist(), int(w["nlocal"]), w["poses"]["fixed"].tolist(),
            w["point_ids"].tolist(),
            [(int(w["point_ids"][e["point"][k]]), int(w["kf_slots"][e["pose"][k]]),
              int(w["edge_feat"][k]), int(e["stereo"][k])) for k in range(len(e))])


HAND_MAIN = (
    [(6, 17), (3, 16), (1, 16)],
    ([2, 3, 1, 5, 4], 3, [0, 0, 1, 1, 1],
     [15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 21, 20, 22],
     [(15, 1, 16, 0), (15, 2, 0, 0), (15, 3, 15, 0), (15, 5, 0, 1),
      (14, 1, 15, 1), (14, 2, 1, 0), (14, 3, 14, 0), (14, 4, 0, 0),
      (13, 1, 14, 0), (13, 2, 2, 0), (13, 3, 13, 0),
      (12, 1, 13, 0), (12, 2, 3, 0), (12, 3, 12, 0),
      (11, 1, 12, 1), (11, 2, 4, 0), (11, 3, 11, 0),
      (10, 1, 11, 0), (10, 2, 5, 0), (10, 3, 10, 0),
      (9, 1, 10, 0), (9, 2, 6, 0), (9, 3, 9, 0),
      (8, 1, 9, 1), (8, 2, 7, 0), (8, 3, 8, 0),
      (7, 1, 8, 0), (7, 2, 8, 0), (7, 3, 7, 0),
      (6, 1, 7, 0), (6, 2, 9, 0), (6, 3, 6, 0),
      (5, 1, 6, 1), (5, 2, 10, 0), (5, 3, 5, 0),
      (4, 1, 5, 0), (4, 2, 11, 0), (4, 3, 4, 0),
      (3, 1, 4, 0), (3, 2, 12, 0), (3, 3, 3, 0),
      (2, 1, 3, 1), (2, 2, 13, 0), (2, 3, 2, 0),
      (1, 1, 2, 0), (1, 2, 14, 0), (1, 3, 1, 0),
      (0, 1, 1, 0), (0, 2, 15, 0), (0, 3, 0, 0),
      (21, 2, 18, 0),
      (20, 1, 0, 1), (20, 3, 16, 0),
      (22, 3, 17, 0), (22, 5, 1, 0)]))


def hand_no_fixed(M):
    """two keyframes that share 16 points and nothing else: no fixed camera"""
    R._plain_points(M, HAND_POINTS)
    A = list(range(16))
    M.set_keyframe(0, A, root=True)
    M.set_keyframe(1, A[8:] + A[:8] + [17])
    hand_attach(M)
    M.set_poses([0, 1], [RL.eye_pose((0.0, 0.0, 0.0)), RL.eye_pose((0.5, 0.0, 0.0))])
    M.update_connections(0)
    M.update_connections(1)
    return window_lists(M.lba_window(1))


HAND_NO_FIXED = (
    [1, 0], 2, [0, 1], [8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7, 17],
    [(8, 0, 8, 0), (8, 1, 0, 0), (9, 0, 9, 0), (9, 1, 1, 0), (10, 0, 10, 0), (10, 1, 2, 0),
     (11, 0, 11, 0), (11, 1, 3, 0), (12, 0, 12, 0), (12, 1, 4, 0), (13, 0, 13, 0), (13, 1, 5, 0),
     (14, 0, 14, 0), (14, 1, 6, 0), (15, 0, 15, 0), (15, 1, 7, 0), (0, 0, 0, 0), (0, 1, 8, 0),
     (1, 0, 1, 0), (1, 1, 9, 0), (2, 0, 2, 0), (2, 1, 10, 0), (3, 0, 3, 0), (3, 1, 11, 0),
     (4, 0, 4, 0), (4, 1, 12, 0), (5, 0, 5, 0), (5, 1, 13, 0), (6, 0, 6, 0), (6, 1, 14, 0),
     (7, 0, 7, 0), (7, 1, 15, 0), (17, 1, 16, 0)])


def hand_empty_current(M):
    """a current keyframe without points: itself, no points, no edges"""
    R._plain_points(M, HAND_POINTS)
    M.set_keyframe(0, list(range(16)), root=True)
    M.set_keyframe(3, [])
    hand_attach(M)
    M.set_poses([0, 3], [RL.eye_pose((0.0, 0.0, 0.0)), RL.eye_pose((1.5, 0.0, 0.0))])
    M.update_connections(3)
    return window_lists(M.lba_window(3))


HAND_EMPTY_CURRENT = ([3], 1, [0], [], [])

HAND_WINDOWS = [(hand_main, HAND_MAIN), (hand_no_fixed, HAND_NO_FIXED),
                (hand_empty_current, HAND_EMPTY_CURRENT)]
HAND_WINDOW_NAMES = ["main", "no_fixed", "empty_current"]


def hand_apply(M):
    """The write-back with flags chosen by hand, on five keyframes that all share 16 points (one
    local part, cur = 2); features 0, 3, 6, ... of slots 1 and 3 are stereo (Observations()
    counts them twice).  Every point's reference keyframe is slot 0.
      point 0  rows 0, 1 (stereo), 2, 4: Observations() 5; slot 2's mono one is erased: 4, good
      point 1  rows 0, 1, 2: 3; slot 0's is erased: the reference moves to slot 1, 2 are left:
               bad, every row entry cleared
      point 2  rows 0, 1, 2, 4: 4; slot 0's is erased: 3, good, the reference moves to slot 1
      point 3  rows 0, 1 (stereo), 2, 3 (stereo), 4: 7; slot 3's is erased: 5
      point 4  rows 0, 1 (stereo), 2, 3 (stereo), 4: 7; slot 2's (mono) and slot 3's (stereo)
               are erased: 4
      point 5  rows 0, 2, 4: 3; slot 0's erasure (the reference moves to slot 2) sends it bad; the
               flag on slot 4's edge, later in edge order, does nothing
      point 6  rows 1 (stereo), 2, 4: 4; flags on slot 1's and slot 2's edges.  Mono first: slot
               2's goes (3 left), then slot 1's (1 left, bad): two erasures.  In plain edge
               order slot 1's would send it bad at once and slot 2's would do nothing.
    Returns the window, (erased, gone bad), the poses and the points written."""
    R._plain_points(M, HAND_POINTS)
    A = list(range(20, 36))                              # 16 points that link every pair
    rows = {0: [0, 1, 2, 3, 4, 5] + A, 1: [0, 1, 2, 3, -1, -1, 4, -1, -1, 6] + A,
            2: [0, 1, 2, 3, 4, 5, 6] + A, 3: [-1, -1, -1, 3, -1, -1, 4] + A,
            4: [0, -1, 2, 3, 4, 5, 6] + A}
    for s, row in rows.items():
        M.set_keyframe(s, row, root=(s == 0))
        st = s in (1, 3)
        M.set_keyframe_features(s, [RC.FEAT_STEREO if st and i % 3 == 0 else 0
                                    for i in range(len(row))])
    hand_attach(M, stereo_slots=(1, 3))
    M.set_poses(list(rows), [RL.eye_pose((0.5 * s, 0.0, 0.0)) for s in rows])
    for s in rows:
        M.update_connections(s)
    w = M.lba_window(2)
    flagged = {(0, 2, 0), (1, 0, 1), (2, 0, 2), (3, 3, 3), (4, 2, 4), (4, 3, 6), (5, 0, 5), (5, 4, 5),
               (6, 1, 9), (6, 2, 6)}
    e = w["edges"]
    erase = np.array([(int(w["point_ids"][e["point"][k]]), int(w["kf_slots"][e["pose"][k]]),
                       int(w["edge_feat"][k])) in flagged for k in range(len(e))], np.uint8)
    assert int(erase.sum()) == len(flagged)
    poses = np.array(w["poses"])
    poses["t"][:, 1] += 0.015625                         # exact in float: every pose moves
    points = w["points"] + 0.03125
    return w, M.lba_apply(w, poses, points, erase), poses, points


HAND_APPLY = (9, 3)                                      # point 5's second flag erases nothing
HAND_APPLY_STATE = dict(
    bad=[False, True, False, False, False, True, True],
    ref=[0, 1, 1, 0, 0, 2, 0],
    nobs=[4, 0, 3, 5, 4, 0, 0],
    rows={0: [0, -1, -1, 3, 4, -1], 1: [0, -1, 2, 3, -1, -1, 4, -1, -1, -1],
          2: [-1, -1, 2, 3, -1, -1, -1], 3: [-1, -1, -1, -1, -1, -1, -1],
          4: [0, -1, 2, 3, 4, -1, -1]})


# ---------------------------------------------------------------------------
# geometric scenes: cameras on a line looking along +z (ref_loop_correct.loop_dataset's), noisy
# projections, gross outliers planted
# ---------------------------------------------------------------------------
WINDOW = 2.2
SCENES = {                      # nkf, cap, landmarks, P(feature), current keyframe, stereo
    "small": dict(nkf=12, cap=192, nland=520, pfeat=0.8, cur=11, stereo=True, seed=0),
    "wide": dict(nkf=12, cap=512, nland=3600, pfeat=0.31, cur=11, stereo=False, seed=1),
}
MAX_KF = 16
OUTLIER_FRACTION, OUTLIER_PIXELS = 0.03, 40.0


def lba_dataset(name):
    """nkf keyframes on a line at x = 0.5 s; keyframe s sees the landmarks within WINDOW of its
    x.  The stored poses and positions are the true ones slightly perturbed; OUTLIER_FRACTION
    of the keypoints are moved by tens of pixels.  A keyframe has mnId 3 s, so slot 0 is the
    map's first keyframe."""
    c = SCENES[name]
    rng = np.random.default_rng(7300 + c["seed"])
    nkf, cap, nland = c["nkf"], c["cap"], c["nland"]
    centres = [(0.5 * s, float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
               for s in range(nkf)]
    land = np.stack([rng.uniform(-2.0, 8.0, nland), rng.uniform(-3.0, 3.0, nland),
                     rng.uniform(8.0, 12.0, nland)], 1)
    land_oct = rng.integers(0, 6, nland)
    feats = []
    for s in range(nkf):
        f = []
        for l in range(nland):
            if abs(land[l][0] - centres[s][0]) > WINDOW or rng.random() > c["pfeat"]:
                continue
            u, v, _ = RE.project(land[l], centres[s])
            if not (12 < u < RE.W_IMG - 12 and 12 < v < RE.H_IMG - 12):
                continue
            f.append((l, l))
        f += [(-1, -1)] * 6
        order = rng.permutation(len(f))
        feats.append([f[i] for i in order][:cap])
    d = RE.geo_dataset(rng, nkf, nland, centres, land, land_oct, feats, cap, c["stereo"])
    d["cur"], d["cap"] = c["cur"], cap
    # gross outliers: the keypoint (and its right coordinate) moved by tens of pixels
    d["outliers"] = []
    for s in range(nkf):
        for i, p in enumerate(d["rows"][s]):
            if p >= 0 and rng.random() < OUTLIER_FRACTION:
                dx = float(rng.choice([-1.0, 1.0]) * rng.uniform(0.75, 1.5) * OUTLIER_PIXELS)
                dy = float(rng.choice([-1.0, 1.0]) * rng.uniform(0.75, 1.5) * OUTLIER_PIXELS)
                d["kps"][s]["x"][i] += dx
                d["kps"][s]["y"][i] += dy
                if d["uright"][s][i] >= 0:
                    d["uright"][s][i] += F(dx)
                d["outliers"].append((s, i))
    T = np.zeros((nkf, 3, 4), F)
    for s in range(nkf):
        Rm = RL._rot(rng.normal(size=3) * 2e-3)
        t = -Rm @ (np.asarray(centres[s], D) + rng.normal(size=3) * 5e-3)
        T[s] = np.concatenate([Rm, t[:, None]], 1).astype(F)
    d["Tcw"] = T
    d["pos"] = (d["pos"].astype(D) + rng.normal(size=d["pos"].shape) * 2e-2).astype(F)
    d["mnid"] = [3 * s for s in range(nkf)]
    return d


def build_lba_map(M, d):
    RE.build_geo_map(M, d)
    M.set_poses(list(range(d["nkf"])), d["Tcw"], d["mnid"])
    M.apply_normal_and_depth(range(d["npts"]))
