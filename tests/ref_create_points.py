"""A pure-Python statement of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:293-576),
KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:823-853) and the table side of
LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:164-220) over tests/ref_lba_map.py's
RefLbaMap, which it subclasses.  The pair search and the triangulation are not restated here:
`create_new_points` takes them as callables (`search_tri`, `triangulate`), as
ref_map_edit.make_search does for Fuse.  Nothing here imports the library; `make_oracle_pair`
takes oracle/pyoracle.py as an argument.

What the reference text gives, as the model states it:
  * the neighbours are the first nn entries of the ordered list, no bad check;
  * from the second neighbour on a raised abort ends the call;
  * each neighbour's search reads has_mp of both rows as they stand then, so a feature of the
    current keyframe that got a point with neighbour i is out of neighbour i + 1's search;
  * vbMatched2 is declared and read in SearchForTriangulation but never set (ORBmatcher.cc:804,
    856): features of the current keyframe do not compete for a feature of the neighbour, and two
    of them may match the same one.  Both points are created; pKF2->AddMapPoint overwrites, so
    the later point keeps the neighbour's feature.  In the table the row is the observation set,
    so the earlier point then has no observation in the neighbour (the reference leaves it a
    one-sided one);
  * ComputeDistinctiveDescriptors and UpdateNormalAndDepth read only the point's own
    observations, so running them after the last neighbour gives the reference's result.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map_edit as RE  # noqa: E402
import ref_loop_correct as RL  # noqa: E402
import ref_lba_map as RB  # noqa: E402

F = np.float32
TRI_NEW = 1
POINT_RANGE, RECENT_RANGE, DEAD, NO_POSE = 1, 2, 4, 8
KF_CAMERA_DTYPE = np.dtype([("Tcw", "<f4", 12), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                            ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"),
                            ("mbf", "<f4")])


def median_index(n):
    """ComputeSceneMedianDepth(q = 2): vDepths[(vDepths.size() - 1) / q]"""
    return (n - 1) // 2


class RefCreateMap(RB.RefLbaMap):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.P = None            # max_points
        self.intr = None         # KF_CAMERA_DTYPE [K]: the attached intrinsics
        self.search_tri = None   # (M, cur, nb, has1, has2) -> (nmatches, vMatches12)
        self.triangulate = None  # (M, cur, nb, vMatches12) -> (x3d [n1][3], status [n1])

    def attach(self, d):
        super().attach(d)
        self.intr = d.get("intr")

    # ---- KeyFrame.cc:823-853 ----
    def scene_depths(self, s):
        T = self.pose[s]
        out = []
        for p in self.kf[s]["points"]:
            if p < 0 or p not in self.mp:
                continue
            x = self.mp[p]["pos"]
            t = np.float64(T[2, 0]) * np.float64(x[0])        # Mat::dot on CV_32F: double, in order
            t += np.float64(T[2, 1]) * np.float64(x[1])
            t += np.float64(T[2, 2]) * np.float64(x[2])
            out.append(F(t + np.float64(T[2, 3])))
        return out

    def baseline(self, a, b):
        d = [F(self.kf[b]["centre"][k]) - F(self.kf[a]["centre"][k]) for k in range(3)]
        sq = np.float64(0)
        for v in d:
            sq += np.float64(v) * np.float64(v)               # cv::norm on CV_32F
        return F(np.sqrt(sq))

    def neighbour_status(self, slot, nb, monocular):
        k = self.kf.get(nb)
        if k is None or not k["live"] or nb not in self.pose:
            return 3
        b = self.baseline(slot, nb)
        if not monocular:
            return 1 if b < F(self.intr[nb]["mb"]) else 0
        z = sorted(self.scene_depths(nb))
        if not z:
            return 3
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = F(b) / F(z[median_index(len(z))])
        return 1 if float(ratio) < 0.01 else 0

    # ---- LocalMapping.cc:293-576 ----
    def create_new_points(self, slot, current_kf_id, monocular, first_id, recent, abort=None,
                          recent_cap=None, batched=False):
        """(recent, report).  batched = True is NOT the reference: it searches every neighbour
        against the rows as they stood when the call started (what a caller batching the pair
        calls computes); the tests use it to show that a scene tells the two apart."""
        rec = list(recent)
        cap = len(rec) + 10 ** 9 if recent_cap is None else recent_cap
        rep = dict(neigh=[], status=[], nmatches=[], nnew=[], created=0, needed=0, bits=0,
                   tri_status=[])
        k = self.kf.get(slot)
        if k is None or not k["live"]:
            rep["bits"] = DEAD
            return rec, rep
        if slot not in self.pose:
            rep["bits"] = NO_POSE
            return rec, rep
        rec0 = len(rec)
        room_p, room_r = max(self.P - first_id, 0), max(cap - rec0, 0)
        room = min(room_p, room_r)
        start = {s: list(v["points"]) for s, v in self.kf.items() if v["live"]}
        n1 = len(k["points"])
        new, aborted, left_out = [], False, set()
        for i, nb in enumerate(self.neighbours(slot, 20 if monocular else 10)):
            rep["neigh"].append(nb)
            if i > 0 and abort:
                aborted = True
            st = 2 if aborted else self.neighbour_status(slot, nb, monocular)
            rep["status"].append(st)
            if st:
                rep["nmatches"].append(0)
                rep["nnew"].append(0)
                rep["tri_status"].append([0] * n1)
                continue
            rows = start if batched else {slot: k["points"], nb: self.kf[nb]["points"]}
            has1, has2 = [p >= 0 for p in rows[slot]], [p >= 0 for p in rows[nb]]
            for idx1 in left_out:       # a cap left this feature's point out: it stays counted once
                has1[idx1] = True
            nm, m12 = self.search_tri(self, slot, nb, has1, has2)
            x3d, tst = self.triangulate(self, slot, nb, m12)
            n2, made = len(self.kf[nb]["points"]), 0
            for idx1 in range(n1):
                idx2 = int(m12[idx1])
                if int(tst[idx1]) != TRI_NEW or not 0 <= idx2 < n2:
                    continue
                order = rep["needed"]
                rep["needed"] += 1
                if order >= room:
                    left_out.add(idx1)
                    continue
                p = first_id + order
                self.mp[p] = {"pos": np.array(x3d[idx1], F), "normal": np.zeros(3, F),
                              "min": F(0), "max": F(0), "bad": False, "desc": bytes(32),
                              "ref": slot}
                self.stats[p] = [current_kf_id, 1, 1]
                self.replaced.pop(p, None)
                self.corr_by.pop(p, None)
                self.corr_ref.pop(p, None)
                if k["points"][idx1] >= 0:               # only the batched variant gets here
                    self._drop(slot, idx1)
                self._put(slot, idx1, p)
                if self.kf[nb]["points"][idx2] >= 0:     # a second idx1 on the same idx2
                    self._drop(nb, idx2)
                self._put(nb, idx2, p)
                rec.append(p)
                new.append(p)
                made += 1
            rep["nmatches"].append(int(nm))
            rep["nnew"].append(made)
            rep["tri_status"].append([int(v) for v in tst])
        rep["created"] = len(new)
        rep["bits"] = (POINT_RANGE if rep["needed"] > room_p else 0) | \
                      (RECENT_RANGE if rep["needed"] > room_r else 0)
        for p in new:
            self.distinctive(p)
            self.apply_normal_and_depth([p])
        return rec, rep

    # ---- LocalMapping.cc:164-220 ----
    def process_new_keyframe(self, slot, ids, octs, feat, Tcw, mnid, in_keyframe, recent,
                             root=False, recent_cap=None):
        rec = list(recent)
        cap = len(rec) + 10 ** 9 if recent_cap is None else recent_cap
        good = [p if 0 <= p < self.P and p in self.mp and not self.mp[p]["bad"] else -1
                for p in ids]
        self.set_keyframe(slot, good, octs, (0.0, 0.0, 0.0), root=root)
        if feat is not None:
            self.set_keyframe_features(slot, feat)
        self.set_poses([slot], [np.asarray(Tcw, F).reshape(3, 4)], [mnid])
        upd, needed, appended = [], 0, 0
        for i, p in enumerate(good):
            if p < 0:
                continue
            if in_keyframe is not None and in_keyframe[i]:
                needed += 1
                if len(rec) < cap:
                    rec.append(p)
                    appended += 1
            else:
                upd.append(p)
        for p in upd:
            self.apply_normal_and_depth([p])
            self.distinctive(p)
        self.update_connections(slot)
        return rec, dict(appended=appended, updated=len(upd), needed=needed,
                         bits=RECENT_RANGE if needed > appended else 0)


def report_lists(rep):
    """the part of a report both sides give as plain lists"""
    return {k: (rep[k] if isinstance(rep[k], int) else [int(v) for v in rep[k]])
            for k in ("neigh", "status", "nmatches", "nnew", "created", "needed", "bits")}


# ---------------------------------------------------------------------------
# the injected pair functions over oracle/pyoracle.py
# ---------------------------------------------------------------------------
def kf_cam(M, s):
    c = np.array(M.intr[s], KF_CAMERA_DTYPE)
    c["Tcw"] = np.asarray(M.pose[s], F).reshape(12)
    return c


def make_oracle_pair(oracle):
    p = oracle.params(nfeatures=2000, scale_factor=1.2, nlevels=8)
    sf, s2 = np.array(p.scale[:8], F), np.array(p.sigma2[:8], F)

    def side(d, s, has):
        return dict(kps=d["kps"][s], desc=d["kdesc"][s], uright=d["uright"][s],
                    has_mp=np.array(has, np.uint8), fv=d["fv"][s])

    def search(M, cur, nb, has1, has2):
        g = oracle.tri_geometry(kf_cam(M, cur), kf_cam(M, nb))
        n, m = oracle.search_for_triangulation(side(M.d, cur, has1), side(M.d, nb, has2), g, sf, s2,
                                               False, False)
        return n, m.tolist()

    def tri(M, cur, nb, m12):
        d = M.d
        a, b = (dict(kps=d["kps"][s], kps_raw=None, uright=d["uright"][s], depth=d["depth"][s])
                for s in (cur, nb))
        _, x, st = oracle.triangulate(a, b, kf_cam(M, cur), kf_cam(M, nb), np.array(m12, np.int32),
                                      sf, s2, p.scale_factor)
        return x.copy(), st.tolist()
    return search, tri


# ---------------------------------------------------------------------------
# hand scenes on the tables alone: stub search / triangulation
# ---------------------------------------------------------------------------
HAND_K, HAND_CAP, HAND_POINTS = 8, 32, 96
ANCH = 16          # points 0..15 are in every row: every pair of keyframes is connected


def hand_map(M, extra, centres=None, stereo_mb=None, npts=HAND_POINTS):
    """Slots 0..len(extra)-1; row s = points 0..15 (plus s further shared ones so that the weights
    differ: slot s also holds 16 .. 16 + s - 1) then `extra[s]` free entries (-1).  Identity
    rotations; centres default to (s, 0, 0); every point at (0, 0, 8)."""
    n = len(extra)
    M.P = npts
    pos = np.tile(np.array([0.0, 0.0, 8.0], F), (npts, 1))
    M.set_points(0, pos, [False] * npts, np.zeros((npts, 32), np.uint8), [0] * npts)
    intr = np.zeros(HAND_K, KF_CAMERA_DTYPE)
    intr["fx"], intr["fy"], intr["cx"], intr["cy"] = 500, 500, 320, 240
    intr["invfx"], intr["invfy"] = F(1) / F(500), F(1) / F(500)
    intr["mb"], intr["mbf"] = (stereo_mb or 0.0), 40.0
    rows = []
    for s in range(n):
        row = list(range(ANCH)) + list(range(ANCH, ANCH + s)) + [-1] * extra[s]
        rows.append(row)
        M.set_keyframe(s, row, [0] * len(row), (0.0, 0.0, 0.0), root=(s == 0))
    cen = centres or [(float(s), 0.0, 0.0) for s in range(n)]
    M.set_poses(list(range(n)), [RL.eye_pose(c) for c in cen], list(range(n)))
    kd = [np.array([[(7 * s + 3 * i) % 256] * 32 for i in range(HAND_CAP)], np.uint8)
          for s in range(HAND_K)]
    M.attach(dict(kdesc=kd, kps=[np.zeros(HAND_CAP, RE.KP_DTYPE)] * HAND_K,
                  uright=[np.full(HAND_CAP, -1, F)] * HAND_K,
                  cams=np.zeros(HAND_K, RE.FRUSTUM_DTYPE), intr=intr))
    for _ in range(2):
        for s in range(n):
            M.update_connections(s)
    return rows


def stub_pair(table):
    """search / triangulate stubs: table[nb] = [(idx1, idx2, status)]; a pair whose idx1 or idx2
    already holds a point is left out, as the search leaves it out"""
    def search(M, cur, nb, has1, has2):
        m = [-1] * len(has1)
        for i1, i2, _ in table.get(nb, []):
            if not has1[i1] and not has2[i2]:
                m[i1] = i2
        return sum(v >= 0 for v in m), m

    def tri(M, cur, nb, m12):
        st = [0] * len(m12)
        for i1, i2, s in table.get(nb, []):
            if m12[i1] == i2:
                st[i1] = s
        x = np.zeros((len(m12), 3), F)
        x[:, 0], x[:, 2] = np.arange(len(m12)), 8.0 + nb
        return x, st
    return search, tri


def hand_sequential(M, batched=False):
    """cur = 3, neighbours by weight 2, 1, 0.  Feature 19 of cur matches feature 18 of slot 2 and
    feature 17 of slot 1; feature 20 matches only slot 1's 18; feature 21's match with slot 2 fails
    the triangulation (-1) and succeeds with slot 1."""
    hand_map(M, [4, 4, 4, 4])
    M.search_tri, M.triangulate = stub_pair({2: [(19, 18, 1), (21, 19, -1)],
                                             1: [(19, 17, 1), (20, 18, 1), (21, 19, 1)]})
    rec, rep = M.create_new_points(3, 3, True, 60, [5], batched=batched)
    return [rec, report_lists(rep), M.keyframe_points(3)[19:], M.keyframe_points(2)[18:],
            M.keyframe_points(1)[17:], M.point_stats(60, 3), M.point_refs(60, 3)]


HAND_SEQUENTIAL = [[5, 60, 61, 62],
                   dict(neigh=[2, 1, 0], status=[0, 0, 0], nmatches=[2, 2, 0], nnew=[1, 2, 0],
                        created=3, needed=3, bits=0),
                   [60, 61, 62, -1], [60, -1, -1, -1], [-1, 61, 62, -1],
                   [(3, 1, 1, 2), (3, 1, 1, 2), (3, 1, 1, 2)], [3, 3, 3]]


def hand_duplicate_idx2(M):
    """features 19 and 20 of cur both match feature 18 of slot 2: two points, the later keeps it"""
    hand_map(M, [4, 4, 4, 4])
    M.search_tri, M.triangulate = stub_pair({2: [(19, 18, 1), (20, 18, 1)]})
    rec, rep = M.create_new_points(3, 3, True, 60, [])
    return [rec, rep["nnew"], M.keyframe_points(3)[19:], M.keyframe_points(2)[18:],
            M.point_stats(60, 2)]


HAND_DUPLICATE = [[60, 61], [2, 0, 0], [60, 61, -1, -1], [61, -1, -1, -1],
                  [(3, 1, 1, 1), (3, 1, 1, 2)]]


def hand_abort(M, abort):
    hand_map(M, [4, 4, 4, 4])
    M.search_tri, M.triangulate = stub_pair({2: [(19, 18, 1)], 1: [(20, 18, 1)], 0: [(21, 17, 1)]})
    rec, rep = M.create_new_points(3, 3, True, 60, [], abort=abort)
    return [rec, rep["status"], rep["nnew"]]


HAND_ABORT = {None: [[60, 61, 62], [0, 0, 0], [1, 1, 1]], 0: [[60, 61, 62], [0, 0, 0], [1, 1, 1]],
              1: [[60], [0, 2, 2], [1, 0, 0]]}


def hand_range(M, first_id, recent_cap):
    hand_map(M, [4, 4, 4, 4])
    M.search_tri, M.triangulate = stub_pair({2: [(19, 18, 1), (20, 19, 1)], 1: [(21, 18, 1), (22, 19, 1)]})
    rec, rep = M.create_new_points(3, 3, True, first_id, [7], recent_cap=recent_cap)
    return [rec, report_lists(rep), M.keyframe_points(3)[19:], M.keyframe_points(1)[17:]]


# max_points 96 reached after three points; recent_cap 3 holds the old entry and two new ones
HAND_RANGE = {(93, None): [[7, 93, 94, 95], dict(neigh=[2, 1, 0], status=[0, 0, 0], nmatches=[2, 2, 0],
                                                  nnew=[2, 1, 0], created=3, needed=4, bits=POINT_RANGE),
                           [93, 94, 95, -1], [-1, 95, -1, -1]],
              (60, 3): [[7, 60, 61], dict(neigh=[2, 1, 0], status=[0, 0, 0], nmatches=[2, 2, 0],
                                          nnew=[2, 0, 0], created=2, needed=4, bits=RECENT_RANGE),
                        [60, 61, -1, -1], [-1, -1, -1, -1]]}


def hand_baseline(M, monocular, gap, depths=None):
    """cur = 1 at (gap, 0, 0), its only neighbour slot 0 at the origin.  Stereo: mb = 2.
    Monocular: slot 0's row entries get the depths `depths` (small integers, identity rotation:
    exact in any order)."""
    hand_map(M, [2, 2], centres=[(0.0, 0.0, 0.0), (float(gap), 0.0, 0.0)], stereo_mb=2.0)
    if depths is not None:
        row = M.keyframe_points(0)
        ids = [p for p in row if p >= 0][:len(depths)]
        pos = np.zeros((len(ids), 3), F)
        pos[:, 2] = depths
        for p, x in zip(ids, pos):
            M.set_points(p, [x], [False], np.zeros((1, 32), np.uint8), [0])
        M.set_keyframe(0, ids + [-1, -1], [0] * (len(ids) + 2), (0.0, 0.0, 0.0), root=True)
        M.set_poses([0], [RL.eye_pose((0.0, 0.0, 0.0))], [0])
    M.search_tri, M.triangulate = stub_pair({})
    return M.create_new_points(1, 1, monocular, 60, [])[1]["status"]


# stereo: baseline 1 < mb 2, 2 == mb, 3 > mb.  Monocular, baseline 1: depths 1..5 -> sorted index
# 2 = 3 (ratio 1/3); an even count 4: index 1; median 128: 1/128 = 0.0078 < 0.01, median 64:
# 1/64 = 0.0156
HAND_BASELINE = [((False, 1, None), [1]), ((False, 2, None), [0]), ((False, 3, None), [0]),
                 ((True, 1, [5, 1, 4, 2, 3]), [0]), ((True, 1, [128] * 3 + [1] * 2), [1]),
                 ((True, 1, [1, 128, 128, 1]), [0]), ((True, 1, [1, 128, 128, 128]), [1]),
                 ((True, 1, [64] * 5), [0]), ((True, 1, [128] * 5), [1]),
                 # (float)1 / 100 = 0.0099999998 < 0.01 in double; 1 / 99 = 0.0101
                 ((True, 1, [100] * 5), [1]), ((True, 1, [99] * 5), [0])]


def hand_process(M):
    """slot 2 arrives with points 0..15 (2 flagged in_keyframe), a bad id, an id out of range and
    a free feature; then the same row for slot 3 flags the same two again"""
    hand_map(M, [2, 2])
    M.set_point_bad(9)
    row = list(range(ANCH)) + [HAND_POINTS + 5, -1]
    ink = [0] * len(row)
    ink[3] = ink[9] = ink[12] = 1
    out = []
    rec = [40]
    for s in (2, 3):
        rec, rep = M.process_new_keyframe(s, row, [0] * len(row), [0] * len(row),
                                          RL.eye_pose((float(s), 0.0, 0.0)), 10 + s, ink, rec)
        out.append([rec, rep, M.keyframe_points(s), M.ordered(s), M.parent(s)])
    return out


HAND_PROCESS_ROW = list(range(9)) + [-1] + list(range(10, ANCH)) + [-1, -1]
HAND_PROCESS = [[[40, 3, 12], dict(appended=2, updated=13, needed=2, bits=0), HAND_PROCESS_ROW,
                 [(1, 15), (0, 15)], 1],
                [[40, 3, 12, 3, 12], dict(appended=2, updated=13, needed=2, bits=0), HAND_PROCESS_ROW,
                 [(2, 15), (1, 15), (0, 15)], 2]]


# ---------------------------------------------------------------------------
# geometric scenes for the injected oracle functions and the GPU
# ---------------------------------------------------------------------------
def create_dataset(seed, stereo, ncur=257, nkf=8, cap=320, nanchor=40, nfresh=420, spacing=0.3,
                   nfeat=None, anchor_all=False, spare_ids=0):
    """nkf keyframes on a line; cur = nkf - 1 with exactly `ncur` features.  Landmarks 0 ..
    nanchor - 1 own the points of the same id and are seen (as that point) by every keyframe
    (anchor_all) or by all but some, so that the weights differ; the fresh landmarks are
    seen without a point, by cur with probability 0.9 and by the others with 0.55: most are in
    more than one neighbour, the sequential dependence.  Landmark nanchor is seen twice by cur
    (two features, one in the neighbours): the double match of one idx2."""
    rng = np.random.default_rng(9100 + seed)
    cur = nkf - 1
    centres = [(spacing * s, float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
               for s in range(nkf)]
    nland = nanchor + nfresh
    land = np.stack([rng.uniform(-3.0, spacing * nkf + 3.0, nland), rng.uniform(-3.5, 3.5, nland),
                     rng.uniform(8.0, 12.0, nland)], 1)
    land[:nanchor, 0] = rng.uniform(spacing * nkf / 2 - 2.0, spacing * nkf / 2 + 2.0, nanchor)
    land[nanchor] = (spacing * nkf / 2, 0.5, 10.0)
    land_oct = rng.integers(0, 6, nland)
    feats = []
    for s in range(nkf):
        f = []
        for l in range(nland):
            u, v, _ = RE.project(land[l], centres[s])
            if not (12 < u < RE.W_IMG - 12 and 12 < v < RE.H_IMG - 12):
                continue
            if l < nanchor:
                if anchor_all or (l + s) % 8 >= s % 5:
                    f.append((l, l))
            elif l == nanchor or rng.random() < (0.9 if s == cur else 0.55):
                f.append((l, -1))
        if s == cur:
            f.insert(0, (nanchor, -1))
        want = ncur if s == cur else (nfeat or len(f) + 10)
        f = f[:want] + [(-1, -1)] * max(want - len(f), 0)
        order = rng.permutation(len(f))
        feats.append([f[i] for i in order])
        assert len(feats[-1]) <= cap
    npts = nanchor + 24 + ncur + spare_ids
    d = RE.geo_dataset(rng, nkf, npts, centres, land, land_oct, feats, cap, stereo)
    d["cur"], d["first_id"], d["cap"] = cur, nanchor + 24, cap
    d["poses"] = [RL.eye_pose(np.asarray(c, np.float64)) for c in d["centre"]]
    d["depth"], d["fv"] = [], []
    for s in range(nkf):
        kp, ur = d["kps"][s], d["uright"][s]
        with np.errstate(divide="ignore"):
            d["depth"].append(np.where(ur >= 0, F(RE.BF) / (kp["x"] - ur), F(-1)).astype(F))
        node = np.array([l // 3 if l >= 0 else 100000 + i % 4 for i, (l, _) in enumerate(feats[s])])
        nodes, cnt = np.unique(node, return_counts=True)
        fe = np.argsort(node, kind="stable")           # ascending feature index inside a node
        off = np.concatenate([[0], np.cumsum(cnt)])
        d["fv"].append((nodes.astype(np.int32), off.astype(np.int32), fe.astype(np.int32)))
    intr = np.zeros(nkf, KF_CAMERA_DTYPE)
    intr["fx"], intr["fy"], intr["cx"], intr["cy"] = RE.FX, RE.FX, RE.CX, RE.CY
    intr["invfx"], intr["invfy"] = F(1) / F(RE.FX), F(1) / F(RE.FX)
    intr["mb"], intr["mbf"] = F(RE.BF) / F(RE.FX), RE.BF
    d["intr"] = intr
    d["first"] = [0] * npts
    d["visible"], d["found"] = [3] * npts, [2] * npts
    return d


def build_create_map(M, d):
    M.P = d["npts"]
    RE.build_geo_map(M, d)
    M.set_poses(list(range(d["nkf"])), d["poses"], [10 + s for s in range(d["nkf"])])


def records_of(M, npts, dtype):
    recs = np.zeros(npts, dtype)
    for p in range(npts):
        m = M.mp[p]
        recs[p] = (m["pos"][0], m["pos"][1], m["pos"][2], m["normal"][0], m["normal"][1],
                   m["normal"][2], m["min"], m["max"], 0 if m["bad"] else 1)
    return recs
