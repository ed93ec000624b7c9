"""A pure-Python statement of the parts of LoopClosing::CorrectLoop the Map runs
(src/LoopClosing.cc:744-920 and src/Optimizer.cc:1040-1323), written from the
reference's text, keyframe by keyframe and point by point in the reference's loop order, over
tests/ref_map_edit.py's RefEditMap (rows, observations, update_connections with add_connection /
update_best_covisibles, replace_one) and tests/ref_essential.py's sim3_mul / sim3_inv / sim3_map /
quat_of_rot.  Nothing here imports the library or oracle/.

State added to the map: per slot a float32 3x4 pose and mnId (the slot by default), mspLoopEdges,
per point mnCorrectedByKF / mnCorrectedReference (0 by default).  cv::Mat products are stated as
the repository states them: float entries, sums in double in index order, one
rounding to float.

The scenes are written against the duck-typed interface (set_poses, propagate, loop_connections,
...) so one function drives this class and the GPU adapter.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402
import ref_culling as RC  # noqa: E402
import ref_map_edit as RE  # noqa: E402
import ref_essential as E  # noqa: E402

F = np.float32


def cv_centre(T):
    """Ow = -Rwc * tcw of a float32 3x4 pose"""
    O = np.zeros(3, F)
    for i in range(3):
        a = float(T[0, i]) * float(T[0, 3])
        a += float(T[1, i]) * float(T[1, 3])
        a += float(T[2, i]) * float(T[2, 3])
        O[i] = F(-a)
    return O


def cv_mul44(A, B):
    """the float 4x4 product A * B: each entry a double sum over k = 0..3, rounded once"""
    out = np.zeros((4, 4), F)
    for r in range(4):
        for c in range(4):
            a = 0.0
            for k in range(4):
                a += float(A[r, k]) * float(B[k, c])
            out[r, c] = F(a)
    return out


def sim3_of_pose(T):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)"""
    T = np.asarray(T, F)
    return (E.quat_of_rot(T[:3, :3].astype(np.float64)[None]), T[:3, 3].astype(np.float64)[None],
            np.ones(1))


def pose_of_sim3(S):
    """Converter::toCvSE3(R(q), t * (1 / s)): float32 3x4"""
    return E.poses(S)[0]


def sim3_record(S):
    return (tuple(S[0][0].tolist()), tuple(S[1][0].tolist()), float(S[2][0]))


class RefLoopMap(RE.RefEditMap):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pose = {}            # slot -> float32 [3, 4]
        self.mnid = {}            # slot -> mnId (the slot when absent)
        self.loop_edges = {}      # slot -> set of slots
        self.corr_by = {}         # id -> mnCorrectedByKF
        self.corr_ref = {}        # id -> mnCorrectedReference
        self.nd64 = {}            # id -> the float64 normal / depth at the moment of its correction

    # ---- state ----
    def id_of(self, s):
        return self.mnid.get(s, s)

    def set_pose(self, s, T):
        """KeyFrame::SetPose"""
        T = np.array(T, F).reshape(3, 4)
        self.pose[s] = T
        self.kf[s]["centre"] = cv_centre(T)

    def set_poses(self, slots, Tcw=None, mnid=None):
        for k, s in enumerate(slots):
            if Tcw is not None:
                self.set_pose(s, Tcw[k])
            if mnid is not None:
                self.mnid[s] = int(mnid[k])

    def get_poses(self, n):
        """(Tcw [n, 3, 4], has_pose, mnId, centres) as the library reports them"""
        T = np.zeros((n, 3, 4), F)
        c = np.zeros((n, 3), F)
        for s in range(n):
            if s in self.pose:
                T[s] = self.pose[s]
            if s in self.kf:
                c[s] = self.kf[s]["centre"]
        return (T, np.array([s in self.pose for s in range(n)]),
                np.array([self.id_of(s) for s in range(n)], np.int32), c)

    def add_loop_edge(self, a, b):
        self.loop_edges.setdefault(a, set()).add(b)
        self.loop_edges.setdefault(b, set()).add(a)

    def get_loop_edges(self, s):
        return sorted(self.loop_edges.get(s, ()))

    def corrected(self, n):
        return ([self.corr_by.get(p, 0) for p in range(n)],
                [self.corr_ref.get(p, 0) for p in range(n)])

    def set_corrected(self, first, by, ref):
        for k, (a, b) in enumerate(zip(by, ref)):
            self.corr_by[first + k], self.corr_ref[first + k] = int(a), int(b)

    def point_pos(self, p):
        return tuple(float(v) for v in self.mp[p]["pos"])

    def point_normal_depth(self, p):
        m = self.mp[p]
        return tuple(float(v) for v in m["normal"]) + (float(m["max"]),)

    def records(self, npts):
        """the MAPPOINT_DTYPE records of the points"""
        recs = np.zeros(npts, RE.MAPPOINT_DTYPE)
        for p in range(npts):
            m = self.mp[p]
            recs[p] = (m["pos"][0], m["pos"][1], m["pos"][2], m["normal"][0], m["normal"][1],
                       m["normal"][2], m["min"], m["max"], 0 if m["bad"] else R.MP_VALID)
        return recs

    # ---- LoopClosing.cc:744-843 ----
    def propagate(self, cur, Scw):
        """(mvpCurrentConnectedKFs, CorrectedSim3, NonCorrectedSim3): dicts slot -> Sim3 as
        ref_essential's one-element tuples.  Scw: (q, t, s)."""
        Scw = (np.array(Scw[0], np.float64)[None], np.array(Scw[1], np.float64)[None],
               np.array([Scw[2]], np.float64))
        self.update_connections(cur)
        members = [t for t, _ in self.ordered(cur)] + [cur]
        corrected, noncorrected = {cur: Scw}, {}
        Tc = self.pose[cur]
        Twc = np.zeros((4, 4), F)                       # GetPoseInverse()
        Twc[:3, :3] = Tc[:3, :3].T
        Twc[:3, 3] = cv_centre(Tc)
        Twc[3, 3] = 1
        for s in members:
            Tiw = np.concatenate([self.pose[s], np.array([[0, 0, 0, 1]], F)])
            if s != cur:
                Tic = cv_mul44(Tiw, Twc)
                corrected[s] = E.sim3_mul(sim3_of_pose(Tic[:3]), Scw)
            noncorrected[s] = sim3_of_pose(Tiw[:3])
        curid = self.id_of(cur)
        for s in sorted(corrected):                     # a std::map<KeyFrame*, ...>
            Siw_c, Siw = corrected[s], noncorrected[s]
            Swi_c = E.sim3_inv(Siw_c)
            for p in list(self.kf[s]["points"]):
                if p < 0 or self.mp[p]["bad"]:
                    continue
                if self.corr_by.get(p, 0) == curid:
                    continue
                P = self.mp[p]["pos"].astype(np.float64)[None]
                self.mp[p]["pos"] = E.sim3_map(Swi_c, E.sim3_map(Siw, P))[0].astype(F)
                self.corr_by[p] = curid
                self.corr_ref[p] = self.id_of(s)
                self.apply_normal_and_depth([p])
                self.nd64[p] = self.normal_and_depth64(p)
            self.set_pose(s, pose_of_sim3(Siw_c))
            self.update_connections(s)
        return members, corrected, noncorrected

    # ---- LoopClosing.cc:848-863 ----
    def loop_fusion(self, cur, matched):
        """mvpCurrentMatchedPoints as ids in feature order: (replaced, added)"""
        row = self.kf[cur]["points"]                    # the live row
        nrep = nadd = 0
        for i, w in enumerate(list(matched)[:len(row)]):
            if w < 0 or w not in self.mp:
                continue
            if row[i] >= 0:
                nrep += self.replace_one(row[i], w) in (0, 4)      # pCurMP->Replace(pLoopMP)
            elif self.add_observation(cur, i, w) == 0:
                self.distinctive(w)
                nadd += 1
        return nrep, nadd

    # ---- LoopClosing.cc:944-992, ORBmatcher.cc:1230-1250 ----
    def search_and_fuse(self, members, corrected, loop_ids, th=4.0):
        """CorrectedPosesMap in slot order; self.search_sim3(map, slot, Scw, ids, th) is the
        Fuse(pKF, Scw, ...) search on the map's state at that moment: (sum of nFused, replaced)"""
        nfused = nrep = 0
        for s in sorted(members):
            k = self.kf[s]
            if not k["live"] or not len(loop_ids):
                continue
            bi, bd = self.search_sim3(self, s, corrected[s], loop_ids, th)
            replace = [-1] * len(loop_ids)              # vpReplacePoints
            for i, (p, b, d) in enumerate(zip(loop_ids, bi, bd)):
                if p not in self.mp or b < 0 or b >= len(k["points"]) or d > RE.TH_LOW:
                    continue
                q = k["points"][b]
                if q >= 0:
                    if not self.mp[q]["bad"]:
                        replace[i] = q
                else:
                    self.add_observation(s, b, p)
                nfused += 1
            for i, q in enumerate(replace):
                if q >= 0:
                    nrep += self.replace_one(q, loop_ids[i]) in (0, 4)
        return nfused, nrep

    # ---- LoopClosing.cc:882-911 ----
    def loop_connections(self, members):
        """[(i, j)] in the iteration order of the map of sets"""
        lc = {}
        for s in members:
            previous = [t for t, _ in self.ordered(s)]
            self.update_connections(s)
            conn = set(self.weights(s))                 # GetConnectedKeyFrames
            for t in previous:
                conn.discard(t)
            for t in members:
                conn.discard(t)
            lc[s] = conn
        return [(s, t) for s in sorted(lc) for t in sorted(lc[s])]


    # ---- Optimizer.cc:1040-1258 ----
    def essential_graph(self, cur, loop, corrected, noncorrected, members, pairs):
        """(vertex slots, fixed vertex, vScw per vertex, the non-corrected Sim3 per vertex, the
        edges (i, j, kind) in addEdge order, edges left out because an end is no vertex).
        members is what CorrectedSim3 / NonCorrectedSim3 hold (their keys)."""
        MIN_FEAT = 100
        assert sorted(members) == sorted(corrected) == sorted(noncorrected)
        verts = [s for s in sorted(self.kf) if self.kf[s]["live"] and not self.kf[s]["bad"]]
        vmap = {s: v for v, s in enumerate(verts)}
        Scw = {s: corrected[s] if s in corrected else sim3_of_pose(self.pose[s]) for s in verts}
        Snc = {s: noncorrected[s] if s in noncorrected else Scw[s] for s in verts}
        edges, inserted, skipped = [], set(), 0
        idc, idl = self.id_of(cur), self.id_of(loop)
        for i, j in pairs:                              # the map of sets, in its order
            idi, idj = self.id_of(i), self.id_of(j)
            if (idi != idc or idj != idl) and self.weights(i).get(j, 0) < MIN_FEAT:
                continue
            if i not in vmap or j not in vmap:
                skipped += 1                            # the reference: optimizer.vertex() = NULL
                continue
            edges.append((vmap[i], vmap[j], 0))
            inserted.add((min(idi, idj), max(idi, idj)))
        for s in verts:
            ids = self.id_of(s)
            par = self.kf[s]["parent"]
            if par is not None:
                if par in vmap:
                    edges.append((vmap[s], vmap[par], 1))
                else:
                    skipped += 1
            loops = self.get_loop_edges(s)
            for t in loops:
                if self.id_of(t) < ids:
                    if t in vmap:
                        edges.append((vmap[s], vmap[t], 1))
                    else:
                        skipped += 1
            # GetCovisiblesByWeight(minFeat): upper_bound over the descending weights; end() gives
            # the EMPTY vector (KeyFrame.cc:237-241)
            ordl = self.ordered(s)
            n = next((k for k, (_, w) in enumerate(ordl) if w < MIN_FEAT), None)
            for t, _ in ([] if n is None else ordl[:n]):
                if t == par or self.kf[t]["parent"] == s or t in loops:
                    continue
                idt = self.id_of(t)
                if self.is_bad_kf(t) or not idt < ids:
                    continue
                if (min(ids, idt), max(ids, idt)) in inserted:
                    continue
                edges.append((vmap[s], vmap[t], 1))
        return (verts, vmap[loop], [Scw[s] for s in verts], [Snc[s] for s in verts], edges, skipped)

    # ---- Optimizer.cc:1264-1323 ----
    def apply_correction(self, cur, verts, Scw, Siw, Tiw):
        """Scw / Siw: one-element Sim3 tuples per vertex (vScw, the optimised estimates)"""
        vmap = {s: v for v, s in enumerate(verts)}
        for v, s in enumerate(verts):
            self.set_pose(s, Tiw[v])
        slot_of = {self.id_of(s): s for s in sorted(self.kf)}
        curid = self.id_of(cur)
        for p in sorted(self.mp):
            m = self.mp[p]
            if m["bad"]:
                continue
            if self.corr_by.get(p, 0) == curid:
                r = slot_of.get(self.corr_ref.get(p, 0))
            else:
                r = m["ref"]
            if r not in vmap:
                continue
            P = m["pos"].astype(np.float64)[None]
            m["pos"] = E.sim3_map(E.sim3_inv(Siw[vmap[r]]), E.sim3_map(Scw[vmap[r]], P))[0].astype(F)
            self.apply_normal_and_depth([p])


def make_search_sim3(fuse_sim3_search, scale_factors):
    """a search callable over fuse_sim3_search(kf, fcam, mps, mdesc, th, sf) -> (n, bi, bd): the
    inputs from the map's own state (ref_map_edit.search_inputs), the camera's Tcw = the Sim3's
    rows [s R | t] rounded to float (Converter::toCvMat(g2o::Sim3))"""
    def search(M, slot, S, ids, th):
        kf, cam, mps, md = RE.search_inputs(M, M.d, slot, ids)
        cam = np.array(cam)
        T = np.concatenate([S[2][0] * E.rot_of_quat(S[0])[0], S[1][0][:, None]], 1)
        cam["Tcw"] = T.astype(F).reshape(12)
        _, bi, bd = fuse_sim3_search(dict(kps=kf["kps"], desc=kf["desc"]), cam, mps, md, th,
                                     scale_factors)
        return bi.tolist(), bd.tolist()
    return search


def state(M, nkf, npts):
    """everything the tests compare exactly after a stage"""
    s = RE.state(M, nkf, npts)
    s["corr"] = M.corrected(npts)
    s["mnid"] = M.get_poses(nkf)[2].tolist()
    s["has_pose"] = M.get_poses(nkf)[1].tolist()
    s["loop_edges"] = [M.get_loop_edges(k) for k in range(nkf)]
    return s


# ---------------------------------------------------------------------------
# hand cases
# ---------------------------------------------------------------------------
def eye_pose(C):
    return np.concatenate([np.eye(3), -np.asarray(C, np.float64)[:, None]], 1).astype(F)


def hand_points_scene(M):
    """Slots 0 (an outsider), 1 and 2 = cur, cameras at x = 0, 1, 2 looking along +z with
    identity rotation; mnId 10, 11, 12.  cur shares two points with slot 1 and one with slot 0,
    so its ordered list is [1] and the set [1, 2].  Scw moves cur's centre from (2, 0, 0) to
    (3, 0, 0), so every member's centre moves by +1 in x.
    Point 0 (1, 0, 4) is in rows 0, 1, 2: corrected once, by slot 1, to (2, 0, 4); its normal is
    taken while no member has moved yet (the owner is the lowest member):
    ((2, 0, 4) / sqrt 20 + (1, 0, 4) / sqrt 17 + (0, 0, 4) / 4) / 3, and its distance to the
    reference keyframe 1 is sqrt 17.  Point 1 is in rows 1, 2 (owner 1), point 2 in row 2 alone
    (owner 2), point 3 in row 0 alone (untouched)."""
    pos = [(1.0, 0.0, 4.0), (1.5, 0.5, 5.0), (2.0, -0.5, 6.0), (0.0, 0.25, 3.0)] + [(0.0, 0.0, 9.0)] * 4
    M.set_points(0, pos, [False] * 8, [[i] * 32 for i in range(8)], [1, 1, 2, 0, 0, 0, 0, 0])
    M.set_keyframe(0, [0, 3], root=True)
    M.set_keyframe(1, [0, 1])
    M.set_keyframe(2, [0, 1, 2])
    M.set_poses([0, 1, 2], [eye_pose((x, 0, 0)) for x in (0, 1, 2)], [10, 11, 12])
    Scw = ((0.0, 0.0, 0.0, 1.0), (-3.0, 0.0, 0.0), 1.0)
    first = M.propagate(2, Scw)[0]
    after_first = (M.corrected(4), [M.point_pos(p) for p in range(4)], M.get_poses(3)[3].tolist())
    nd0 = M.point_normal_depth(0)
    # already corrected: a second call moves the poses again and leaves every point alone
    second = M.propagate(2, Scw)[0]
    after_second = (M.corrected(4), [M.point_pos(p) for p in range(4)], M.get_poses(3)[3].tolist())
    return [first, after_first, second, after_second], nd0


HAND_POINTS_SCENE = [
    [1, 2],
    (([12, 12, 12, 0], [11, 11, 12, 0]),
     [(2.0, 0.0, 4.0), (2.5, 0.5, 5.0), (3.0, -0.5, 6.0), (0.0, 0.25, 3.0)],
     [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]]),
    [1, 2],
    # Tic = [I | C2 - C1] = [I | (1, 0, 0)] again, so slot 1 lands on (2, 0, 0) once more
    (([12, 12, 12, 0], [11, 11, 12, 0]),
     [(2.0, 0.0, 4.0), (2.5, 0.5, 5.0), (3.0, -0.5, 6.0), (0.0, 0.25, 3.0)],
     [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]]),
]
S20, S17 = 20.0 ** 0.5, 17.0 ** 0.5
HAND_POINT0_ND = ((2 / S20 + 1 / S17) / 3, 0.0, (4 / S20 + 4 / S17 + 1) / 3, S17)   # normal, max_dist


def hand_apply_by_mnid(M):
    """Apply maps mnCorrectedReference from mnId to a keyframe at the moment it runs.  After
    hand_points_scene (points 0, 1 carry reference 11, point 2 carries 12): point 3 is given
    (12, 10) by the caller, and slot 1's mnId becomes 77, so no keyframe carries 11 any more.
    Vertex v's optimised pose lies v + 1 behind its Scw along z, so a point moves by +(v + 1) in
    z: points 0 and 1 stay, point 2 (slot 2) moves by 3, point 3 (slot 0, mnId 10) by 1."""
    hand_points_scene(M)
    M.set_corrected(3, [12], [10])
    M.set_poses([1], None, [77])
    centres = M.get_poses(3)[3].astype(np.float64)
    q = np.array([[0.0, 0.0, 0.0, 1.0]])
    Scw = [(q, -centres[v][None], np.ones(1)) for v in range(3)]
    Siw = [(q, -centres[v][None] - np.array([[0.0, 0.0, v + 1.0]]), np.ones(1)) for v in range(3)]
    Tiw = np.stack([pose_of_sim3(S) for S in Siw])
    M.apply_correction(2, [0, 1, 2], Scw, Siw, Tiw)
    return [M.point_pos(p) for p in range(4)], M.get_poses(3)[3].tolist()


HAND_APPLY_BY_MNID = ([(2.0, 0.0, 4.0), (2.5, 0.5, 5.0), (3.0, -0.5, 9.0), (0.0, 0.25, 4.0)],
                      [[0.0, 0.0, 1.0], [2.0, 0.0, 2.0], [3.0, 0.0, 3.0]])


def hand_loop_connections(M, members):
    """Slots 0 = e, 1 = t, 2 = u (an outsider), 3.  t shares 3 points with u, 20 with slot 3 and
    15 with e; its UpdateConnections ran before e existed, so W[t] = {u: 3, 3: 20} with u below
    the threshold and off its list.  members [e, t]: e's AddConnection(t <- e, 15) re-sorts t's
    list over all its weights, u enters t's snapshot and drops out of LoopConnections[t]:
    [(0, 2)].  members [t, e]: t's snapshot is [3], so u stays: [(0, 2), (1, 2)]."""
    R._plain_points(M, 64)
    ids = R._Ids()
    s12, s13, s01, s02 = ids.take(3), ids.take(20), ids.take(15), ids.take(2)
    M.set_keyframe(1, s12 + s13 + s01)
    M.set_keyframe(2, s12 + s02)
    M.set_keyframe(3, s13)
    M.update_connections(1)
    M.set_keyframe(0, s01 + s02, root=True)
    return [tuple(p) for p in M.loop_connections(members)], M.ordered(1)


HAND_LC_E_FIRST = ([(0, 2)], [(3, 20), (0, 15)])      # t's own update then rebuilds its list
HAND_LC_T_FIRST = ([(0, 2), (1, 2)], [(3, 20), (0, 15)])


def hand_loop_fusion(M):
    """The loop fusion in feature order on cur = 0 with rows 0: [1, -, 2, -, 3, 6], 1: [1, 4],
    2: [5, 6] and point 9 bad, matched = [4, 5, 9, 5, 3, 5, 7]:
      feature 0: 1 -> 4; keyframe 1 holds both, so its entry of 1 is erased
      feature 1: free, 5 is added
      feature 2: 2 -> 9, a bad point: nothing
      feature 3: free, but cur holds 5 by now: nothing
      feature 4: 3 -> 3, the same point: nothing
      feature 5: 6 -> 5; cur and keyframe 2 hold 5, so both entries of 6 are erased
    The seventh entry is past the row."""
    RE._hand_map(M, {0: [1, -1, 2, -1, 3, 6], 1: [1, 4], 2: [5, 6]})
    M.set_point_bad(9)
    counts = tuple(M.loop_fusion(0, [4, 5, 9, 5, 3, 5, 7]))
    return [counts, [M.keyframe_points(s) for s in range(3)], M.point_bad(1, 6),
            M.point_replaced(1, 6)]


HAND_LOOP_FUSION = [(2, 1), [[4, 5, 2, -1, 3, -1], [-1, 4], [5, -1]],
                    [True, False, False, False, False, True], [4, -1, -1, -1, -1, 5]]


def hand_edge_rules(M):
    """16 slots, rows of at most 128 features, so a keyframe has one partner at weight 100.  Slot
    15 is a hub that shares 15 points with slots 2, 4, 6, 8, 9, 10, 12: their ordered lists then
    end below 100 and GetCovisiblesByWeight(100) returns the partner (a list with no weight
    below 100 returns nothing: slots 1, 3, 5, 7, 11).  Slot 14 is bad: no vertex, so the hub is
    vertex 14.  cur = 13 and loop = 0 share 99 points.
      (1, 2)   weight 100, nothing in the way: the covisibility edge 2 -> 1
      (3, 4)   4's parent is 3: the spanning-tree edge alone
      (5, 6)   5's parent is 6, so 5 is 6's child: 5 -> 6 alone
      (7, 8)   a loop edge: 8 -> 7 once, as the loop edge
      (9, 10)  mnId 100 and 50, against the slot order: 9 -> 10, and nothing from 10
      (11, 12) a LoopConnections pair of weight 100: kind 0, then in sInsertedEdges
    The pairs (0, 13) and (13, 0) both have weight 99: only (cur, loop) is kept.  Slot 1's parent
    is the bad slot 14: left out, counted."""
    R._plain_points(M, 1024)
    ids = R._Ids()
    rows = {s: [] for s in range(16)}
    for a, b in ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12)):
        sh = ids.take(100)
        rows[a] += sh
        rows[b] += sh
    sh = ids.take(99)
    rows[0] += sh
    rows[13] += sh
    for s in (2, 4, 6, 8, 9, 10, 12):
        sh = ids.take(15)
        rows[s] += sh
        rows[15] += sh
    for s in range(16):
        M.set_keyframe(s, rows[s], root=(s == 0), bad=(s == 14))
    M.set_poses(list(range(16)), [eye_pose((0.1 * s, 0, 0)) for s in range(16)])
    M.set_poses([9, 10], None, [100, 50])
    for s in range(16):
        M.update_connections(s)
    members, co, nc = M.propagate(13, ((0.0, 0.0, 0.0, 1.0), (-1.4, 0.0, 0.0), 1.0))
    for s in range(1, 16):
        M.set_parent(s, {1: 14, 4: 3, 5: 6}.get(s, 0))
    M.add_loop_edge(7, 8)
    verts, fixed, _, _, edges, skipped = M.essential_graph(13, 0, co, nc, members,
                                                           [(0, 13), (11, 12), (13, 0)])
    return members, list(verts), fixed, [tuple(e) for e in edges], skipped


HAND_EDGE_RULES = (
    [0, 13], list(range(14)) + [15], 0,
    [(11, 12, 0), (13, 0, 0),
     (2, 0, 1), (2, 1, 1), (3, 0, 1), (4, 3, 1), (5, 6, 1), (6, 0, 1), (7, 0, 1), (8, 0, 1), (8, 7, 1),
     (9, 0, 1), (9, 10, 1), (10, 0, 1), (11, 0, 1), (12, 0, 1), (13, 0, 1), (14, 0, 1)],
    1)


# ---------------------------------------------------------------------------
# random scenes: a trajectory that returns to its start
# ---------------------------------------------------------------------------
NKF, KF_CAP, NLAND, MAX_KF = 24, 192, 520, 32
NPTS = 2 * NLAND
CUR, LOOP = 23, 0
HALF = 12
WINDOW = 2.2


def _rot(w):
    return E._rotvec(np.asarray(w, np.float64))


def loop_dataset(seed, stereo):
    """24 keyframes on a line, out (slots 0..11) and back (12..23), looking along +z; keyframe
    s sees the landmarks within WINDOW of its x.  The way back sees every landmark under a
    second id (nland + l): nothing links the two halves until the duplicates are fused.  The
    second half carries a drift D (a small rotation and translation): its poses are Tcw * D^-1
    and its points D(X)."""
    rng = np.random.default_rng(9100 + seed)
    xs = [0.5 * s for s in range(HALF)] + [0.5 * (NKF - 1 - s) + 0.13 for s in range(HALF, NKF)]
    centres = [(x, float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1))) for x in xs]
    land = np.stack([rng.uniform(-2.0, 8.0, NLAND), rng.uniform(-3.0, 3.0, NLAND),
                     rng.uniform(8.0, 12.0, NLAND)], 1)
    land_oct = rng.integers(0, 6, NLAND)
    feats = []
    for s in range(NKF):
        f = []
        for l in range(NLAND):
            u, v, _ = RE.project(land[l], centres[s])
            if abs(land[l][0] - centres[s][0]) > WINDOW or rng.random() > 0.8:
                continue
            if not (12 < u < RE.W_IMG - 12 and 12 < v < RE.H_IMG - 12):
                continue
            f.append((l, -1 if rng.random() < 0.1 else (l if s < HALF else NLAND + l)))
        f += [(-1, -1)] * 6
        order = rng.permutation(len(f))
        feats.append([f[i] for i in order][:KF_CAP])
    d = RE.geo_dataset(rng, NKF, NPTS, centres, land, land_oct, feats, KF_CAP, stereo)
    d["nland"] = NLAND
    Rd, td = _rot(rng.normal(size=3) * 0.02), rng.normal(size=3) * 0.05
    d["drift"] = (Rd, td)
    T = np.zeros((NKF, 3, 4), F)
    for s in range(NKF):
        Tt = np.concatenate([np.eye(3), -np.asarray(centres[s], np.float64)[:, None]], 1)
        if s >= HALF:                                   # Tcw * D^-1
            Tt = np.concatenate([Tt[:, :3] @ Rd.T, (Tt[:, 3] - Tt[:, :3] @ Rd.T @ td)[:, None]], 1)
        T[s] = Tt.astype(F)
    d["Tcw"] = T
    pos = d["pos"].astype(np.float64)
    pos[NLAND:] = pos[NLAND:] @ Rd.T + td
    d["pos"] = pos.astype(F)
    d["mnid"] = [3 * s + 1 for s in range(NKF)]
    # mvpCurrentMatchedPoints: the first half's point of the landmark, for 60 % of cur's features
    d["matched"] = [int(l) if l >= 0 and rng.random() < 0.6 else -1 for l, _ in feats[CUR]]
    # mvpLoopMapPoints: the points of the loop keyframe and of the keyframes after it
    d["loop_ids"] = sorted({p for s in range(LOOP, LOOP + 5) for p in d["rows"][s] if p >= 0})
    # mg2oScw: the true pose of cur with a scale drift
    s_drift = 1.0 if stereo else 1.03
    Ttrue = np.concatenate([np.eye(3), -np.asarray(centres[CUR], np.float64)[:, None]], 1)
    Rt = _rot(rng.normal(size=3) * 0.003) @ Ttrue[:, :3]
    d["Scw"] = (tuple(E.quat_of_rot(Rt[None])[0].tolist()), tuple((s_drift * Ttrue[:, 3]).tolist()),
                s_drift)
    return d


def build_loop_map(M, d):
    RE.build_geo_map(M, d)
    M.set_poses(list(range(d["nkf"])), d["Tcw"], d["mnid"])
    for s in range(1, d["nkf"]):                        # the spanning tree of a trajectory: the
        M.set_parent(s, s - 1)                          # keyframes came one after another
    M.apply_normal_and_depth(range(d["npts"]))


def run_loop_scene(M, d, check=None):
    """Propagate, the loop fusion, SearchAndFuse, LoopConnections, the essential graph,
    AddLoopEdge; check(stage) after each"""
    build_loop_map(M, d)
    if check:
        check("build")
    out = {}
    out["set"], out["corrected"], out["noncorrected"] = M.propagate(CUR, d["Scw"])
    if check:
        check("propagate")
    out["fusion"] = tuple(M.loop_fusion(CUR, d["matched"]))
    if check:
        check("fusion")
    out["saf"] = tuple(M.search_and_fuse(out["set"], out["corrected"], d["loop_ids"]))
    if check:
        check("fuse")
    out["pairs"] = [tuple(p) for p in M.loop_connections(out["set"])]
    if check:
        check("loop_connections")
    (out["verts"], out["fixed"], out["Scw"], out["Snc"], out["edges"],
     out["skipped"]) = M.essential_graph(CUR, LOOP, out["corrected"], out["noncorrected"], out["set"],
                                         out["pairs"])
    out["verts"], out["edges"] = list(out["verts"]), [tuple(e) for e in out["edges"]]
    M.add_loop_edge(LOOP, CUR)
    if check:
        check("loop_edge")
    return out
