"""A pure-Python statement of MapPoint::AddObservation / Replace / ComputeDistinctiveDescriptors
(src/MapPoint.cc:121-142, 253-303, 342-425), the map update of ORBmatcher::Fuse
(src/ORBmatcher.cc:1100-1125) and LocalMapping::SearchInNeighbors (src/LocalMapping.cc:583-683)
over tests/ref_culling.py's RefCullMap, which it subclasses.  Fuse's search is not restated here:
`fuse` takes a search result, and `search_in_neighbors` a callable that produces one.  Nothing
here imports the library or oracle/.

Replace recomputes the survivor's descriptor at once, as the reference does.  The library does it
once per call ("Edits on the Map"), which gives the same descriptor for every point
that is good when the call ends; a survivor replaced later in the same call is bad, and its
descriptor is read by nothing.  The comparisons therefore cover the descriptors of good points.

The scenes are written against RefCullMap's duck-typed interface extended with the calls below,
so one scene function drives this class and the GPU adapter.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402
import ref_culling as RC  # noqa: E402

F = np.float32
TH_LOW = 50
NONE, ADDED, REPLACED_BY_KF, REPLACED_KF, KF_BAD_POINT, STALE = 0, 1, 2, 3, 4, 5

# the library's record layouts (include/orbg.h), restated so that this file stands alone
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MAPPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"),
                           ("ny", "<f4"), ("nz", "<f4"), ("min_dist", "<f4"),
                           ("max_dist", "<f4"), ("flags", "<i4")])
FRUSTUM_DTYPE = np.dtype([("Tcw", "<f4", 12), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                          ("cy", "<f4"), ("bf", "<f4"), ("log_scale_factor", "<f4"),
                          ("nlevels", "<i4"), ("min_x", "<f4"), ("max_x", "<f4"),
                          ("min_y", "<f4"), ("max_y", "<f4")])


class RefEditMap(RC.RefCullMap):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.replaced = {}       # id -> mpReplaced
        self.kfdesc = {}         # slot -> uint8 [N][32]: the attached mDescriptors
        self.search = None       # (map, slot, ids) -> (best_idx, best_dist)
        self.n_desc_changed = 0

    # ---- state ----
    def attach(self, d):
        """the keyframes' descriptors (and, for the search callable, everything else in d)"""
        self.kfdesc = {s: np.asarray(d["kdesc"][s], np.uint8) for s in range(len(d["kdesc"]))}
        self.d = d

    def point_replaced(self, first, n):
        return [self.replaced.get(p, -1) for p in range(first, first + n)]

    def point_desc(self, first, n):
        """mDescriptor of the good points (None for a bad one: see the module docstring)"""
        return [None if self.mp[p]["bad"] else self.mp[p]["desc"] for p in range(first, first + n)]

    def _put(self, s, idx, p):
        self.observations(0)
        self.kf[s]["points"][idx] = p
        self._inv.setdefault(p, {})[s] = idx

    def in_keyframe(self, p, s):
        self.observations(0)
        return s in self._inv.get(p, {})

    def _stats(self, p):
        return self.stats.setdefault(p, [0, 1, 1])

    # ---- MapPoint.cc ----
    def add_observation(self, s, idx, p):
        """AddObservation + AddMapPoint; the status the library reports"""
        k = self.kf.get(s)
        if k is None or not k["live"]:
            return 1
        if idx < 0 or idx >= len(k["points"]):
            return 2
        if p not in self.mp:
            return 3
        if self.mp[p]["bad"]:
            return 4
        if self.in_keyframe(p, s):
            return 5
        if k["points"][idx] >= 0:
            return 6
        self._put(s, idx, p)
        return 0

    def add_observations(self, slots, idx, ids):
        return [self.add_observation(s, i, p) for s, i, p in zip(slots, idx, ids)]

    def distinctive(self, p):
        m = self.mp[p]
        if m["bad"]:
            return
        D = [self.kfdesc[s][i] for s, i in self.observations(p)
             if not self.kf[s]["bad"] and s in self.kfdesc and i < len(self.kfdesc[s])]
        if not D:
            return
        N = len(D)
        A = np.stack(D)
        dist = np.unpackbits(A[:, None, :] ^ A[None, :, :], axis=2).sum(2).tolist()  # all pairs
        best_median, best = 2 ** 31 - 1, 0
        for i in range(N):
            median = sorted(dist[i])[int(0.5 * (N - 1))]
            if median < best_median:
                best_median, best = median, i
        new = bytes(bytearray(D[best]))
        self.n_desc_changed += new != m["desc"]
        m["desc"] = new

    def compute_distinctive(self, ids):
        for p in ids:
            if p in self.mp:
                self.distinctive(p)

    def replace_one(self, o, w):
        """o->Replace(w); the status the library reports"""
        if o == w:
            return 1
        if w not in self.mp or self.mp[w]["bad"]:
            return 2
        if o not in self.mp:
            return 3
        was_bad = self.mp[o]["bad"]
        if not was_bad:
            for s, idx in self.observations(o):
                self._drop(s, idx)
                if not self.in_keyframe(w, s):
                    self._put(s, idx, w)            # ReplaceMapPointMatch + AddObservation
            self.mp[o]["bad"] = True
        self.replaced[o] = w
        so, sw = self._stats(o), self._stats(w)
        sw[2] += so[2]
        sw[1] += so[1]
        self.distinctive(w)
        return 4 if was_bad else 0

    def replace(self, olds, news):
        return [self.replace_one(o, w) for o, w in zip(olds, news)]

    # ---- ORBmatcher.cc:1100-1125 ----
    def fuse(self, slot, ids, best_idx, best_dist):
        """the update given a search result: (nFused, status per point)"""
        k = self.kf.get(slot)
        if k is None or not k["live"]:
            return 0, [NONE] * len(ids)
        nfused, status = 0, []
        for p, b, d in zip(ids, best_idx, best_dist):
            if p not in self.mp or b < 0 or b >= len(k["points"]) or d > TH_LOW:
                status.append(NONE)
                continue
            if self.mp[p]["bad"] or self.in_keyframe(p, slot):
                status.append(STALE)
                continue
            q = k["points"][b]
            if q >= 0:
                if not self.mp[q]["bad"]:
                    if self.n_obs(q) > self.n_obs(p):
                        self.replace_one(p, q)
                        status.append(REPLACED_BY_KF)
                    else:
                        self.replace_one(q, p)
                        status.append(REPLACED_KF)
                else:
                    status.append(KF_BAD_POINT)
            else:
                self.add_observation(slot, b, p)
                status.append(ADDED)
            nfused += 1
        return nfused, status

    def Fuse(self, slot, ids, search=None):
        search = search or self.search
        bi, bd = search(self, slot, ids)
        return self.fuse(slot, ids, bi, bd)

    # ---- LocalMapping.cc:583-683 ----
    def target_keyframes(self, slot, current_kf_id, monocular):
        targets, marked = [], set()
        k = self.kf.get(slot)
        if current_kf_id == 0 or k is None or not k["live"]:
            return targets                          # mnFuseTargetForKF starts at 0
        for t in self.neighbours(slot, 20 if monocular else 10):
            if self.is_bad_kf(t) or t in marked:
                continue
            targets.append(t)
            marked.add(t)
            for t2 in self.neighbours(t, 5):
                if self.is_bad_kf(t2) or t2 in marked or t2 == slot:
                    continue
                targets.append(t2)                  # not marked when pushed
        return targets

    def search_in_neighbors(self, slot, current_kf_id, monocular, search=None):
        """(vpTargetKFs, the return value of each entry's Fuse, the second pass's)"""
        targets = self.target_keyframes(slot, current_kf_id, monocular)
        snap = self.keyframe_points(slot)
        nfused = [self.Fuse(t, snap, search)[0] for t in targets]
        cands, seen = [], set()
        for t in targets:
            for p in self.keyframe_points(t):
                if p < 0 or self.mp[p]["bad"] or p in seen:
                    continue
                seen.add(p)
                cands.append(p)
        second = self.Fuse(slot, cands, search)[0] if current_kf_id != 0 else 0
        for p in self.keyframe_points(slot):
            if p >= 0 and not self.mp[p]["bad"]:
                self.distinctive(p)
                self.apply_normal_and_depth([p])
        self.update_connections(slot)
        return targets, nfused, second


def state(M, nkf, npts):
    """everything the tests compare after a call"""
    s = RC.state(M, nkf, npts)
    s["replaced"] = M.point_replaced(0, npts)
    s["desc"] = M.point_desc(0, npts)
    return s


# ---------------------------------------------------------------------------
# the search inputs from a map's state, for a search callable
# ---------------------------------------------------------------------------
def search_inputs(M, d, slot, ids):
    """(kf dict, camera, MAPPOINT records, descriptors) of Fuse(slot, ids) as the reference
    reads them when the call starts: VALID = pMP && !isBad() && !IsInKeyFrame(pKF)"""
    mps = np.zeros(len(ids), MAPPOINT_DTYPE)
    md = np.zeros((len(ids), 32), np.uint8)
    for i, p in enumerate(ids):
        m = M.mp.get(p)
        if m is None:
            continue
        mps[i] = (m["pos"][0], m["pos"][1], m["pos"][2], m["normal"][0], m["normal"][1],
                  m["normal"][2], m["min"], m["max"],
                  0 if m["bad"] or M.in_keyframe(p, slot) else R.MP_VALID)
        md[i] = np.frombuffer(m["desc"], np.uint8)
    kf = dict(kps=d["kps"][slot], desc=d["kdesc"][slot], uright=d["uright"][slot])
    return kf, d["cams"][slot], mps, md


def make_search(fuse_search, scale_factors, inv_sigma2, th=3.0):
    """a search callable over fuse_search(kf, fcam, mps, mdesc, th, sf, isg) -> (n, bi, bd) and
    the data attached to the map"""
    def search(M, slot, ids):
        if not len(ids):
            return [], []
        kf, cam, mps, md = search_inputs(M, M.d, slot, ids)
        _, bi, bd = fuse_search(kf, cam, mps, md, th, scale_factors, inv_sigma2)
        return bi.tolist(), bd.tolist()
    return search


# ---------------------------------------------------------------------------
# hand cases on the tables alone (no geometry): each returns what it reads
# ---------------------------------------------------------------------------
HAND_POINTS = 64
STEREO = RC.FEAT_STEREO


def _hand_map(M, rows, feats=None, npts=HAND_POINTS):
    R._plain_points(M, npts)
    for s, row in sorted(rows.items()):
        M.set_keyframe(s, row, root=(s == 0))
        if feats and s in feats:
            M.set_keyframe_features(s, feats[s])
    kd = [np.array([[(7 * s + 3 * i) % 256] * 32 for i in range(8)], np.uint8) for s in range(8)]
    M.attach(dict(kdesc=kd, kps=[np.zeros(8, KP_DTYPE)] * 8, uright=[np.full(8, -1, F)] * 8,
                  cams=np.zeros(8, FRUSTUM_DTYPE)))


def hand_replace_moves_and_erases(M):
    """old 1 is in keyframes 0, 1 (a STEREO feature), 2; new 2 is in keyframe 0 and 3: the entry
    of keyframe 0 is erased, those of 1 and 2 move (Observations 1 + 2 + 1 + 1 = 5), found and
    visible add up, mpRefKF stays"""
    _hand_map(M, {0: [1, 2, -1], 1: [-1, 1], 2: [1], 3: [5, 2]}, {1: [0, STEREO]})
    M.set_point_stats(1, visible=[10, 3], found=[7, 2])
    before = M.point_stats(2, 1)
    st = M.replace([1, 2, 9], [2, 2, 1])
    return [before, st, [M.keyframe_points(s) for s in range(4)], M.point_bad(1, 2),
            M.point_replaced(1, 2), M.point_stats(1, 2), M.point_refs(1, 2)]


HAND_REPLACE = [[(0, 3, 2, 2)], [0, 1, 2], [[-1, 2, -1], [-1, 2], [2], [5, 2]], [True, False],
                [2, -1], [(0, 10, 7, 0), (0, 13, 9, 5)], [0, 0]]


def hand_replace_bad_old(M):
    """an already-bad old point still sits in a row: only mpReplaced and the transfer happen"""
    _hand_map(M, {0: [1, 2], 1: [1]})
    M.set_point_stats(1, visible=[4, 5], found=[2, 3])
    M.set_point_bad(1)
    st = M.replace([1, 1], [2, 40])
    return [st, M.keyframe_points(0), M.keyframe_points(1), M.point_replaced(1, 1),
            M.point_stats(2, 1)[0][1:3]]


HAND_REPLACE_BAD_OLD = [[4, 4], [1, 2], [1], [40], (9, 5)]


def hand_add_observations(M):
    _hand_map(M, {0: [1, -1, -1], 1: [-1]})
    M.set_point_bad(7)
    st = M.add_observations([0, 0, 0, 0, 0, 5, 1, 0, 0], [1, 2, 3, 2, 0, 0, 0, 2, 2],
                            [3, 3, 4, HAND_POINTS, 4, 4, 4, 7, 1])
    return [st, M.keyframe_points(0), M.keyframe_points(1), M.point_stats(3, 2)]


# added; already in the slot; idx past N; id out of range; the feature holds 1; dead slot; added;
# bad point; already in the slot
HAND_ADD = [[0, 5, 2, 3, 6, 1, 0, 4, 5], [1, 3, -1], [4], [(0, 1, 1, 1), (0, 1, 1, 1)]]

HAND_CASES = [(hand_replace_moves_and_erases, HAND_REPLACE),
              (hand_replace_bad_old, HAND_REPLACE_BAD_OLD),
              (hand_add_observations, HAND_ADD)]
HAND_NAMES = ["replace_moves_and_erases", "replace_bad_old", "add_observations"]


# ---------------------------------------------------------------------------
# geometric scenes: cameras on a line looking along +z, landmarks in front of them, a feature
# where a keyframe sees a landmark.  A landmark may own several map point ids (the duplicates
# Fuse merges).
# ---------------------------------------------------------------------------
W_IMG, H_IMG, FX, CX, CY, BF = 640.0, 480.0, 500.0, 320.0, 240.0, 40.0
NLEVELS = 8


def project(X, C):
    z = X[2] - C[2]
    return FX * (X[0] - C[0]) / z + CX, FX * (X[1] - C[1]) / z + CY, z


def camera(C):
    cam = np.zeros((), FRUSTUM_DTYPE)
    T = np.concatenate([np.eye(3), -np.asarray(C, np.float64)[:, None]], 1).astype(F)
    cam["Tcw"] = T.reshape(12)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"] = FX, FX, CX, CY, BF
    cam["log_scale_factor"] = F(np.log(np.float64(F(1.2))))
    cam["nlevels"] = NLEVELS
    cam["min_x"], cam["max_x"], cam["min_y"], cam["max_y"] = 0.0, W_IMG, 0.0, H_IMG
    return cam


def geo_dataset(rng, nkf, npts, centres, land_pos, land_oct, feats, kf_cap, stereo):
    """feats[s] = [(landmark or -1 for a decoy, point id or -1)] in feature order.  A landmark's
    features carry its base descriptor a few bits apart and its octave everywhere; a decoy is a
    random keypoint with a random descriptor."""
    base = rng.integers(0, 256, (len(land_pos), 32), dtype=np.uint8)

    def noisy(l):
        flips = np.zeros(256, np.uint8)
        flips[rng.choice(256, int(rng.integers(0, 7)), replace=False)] = 1
        return base[l] ^ np.packbits(flips)

    d = {"nkf": nkf, "npts": npts, "stereo": stereo, "centre": np.asarray(centres, F)}
    d["rows"], d["octs"], d["featfl"], d["kps"], d["kdesc"], d["uright"] = [], [], [], [], [], []
    d["cams"] = np.zeros(nkf, FRUSTUM_DTYPE)
    owner = {}
    for s in range(nkf):
        d["cams"][s] = camera(d["centre"][s].astype(np.float64))
        n = len(feats[s])
        assert n <= kf_cap
        kp = np.zeros(n, KP_DTYPE)
        kd = np.zeros((n, 32), np.uint8)
        ur = np.full(n, -1.0, F)
        row, octs, fl = [], [], []
        for i, (l, p) in enumerate(feats[s]):
            if l < 0:
                kp["x"][i], kp["y"][i] = rng.uniform(5, W_IMG - 5), rng.uniform(5, H_IMG - 5)
                kp["octave"][i] = rng.integers(0, 6)
                kd[i] = rng.integers(0, 256, 32, dtype=np.uint8)
                z = 10.0
            else:
                u, v, z = project(land_pos[l], d["centre"][s].astype(np.float64))
                kp["x"][i], kp["y"][i] = u + rng.normal(0, 0.25), v + rng.normal(0, 0.25)
                kp["octave"][i] = land_oct[l]
                kd[i] = noisy(l)
            st = stereo and rng.random() < 0.5
            if st:
                ur[i] = kp["x"][i] - BF / z
            kp["size"][i], kp["response"][i], kp["angle"][i] = 31, 20, rng.uniform(0, 360)
            row.append(int(p))
            octs.append(int(kp["octave"][i]))
            fl.append((RC.FEAT_STEREO if st else 0) | (RC.FEAT_CLOSE if rng.random() < 0.8 else 0))
            if p >= 0:
                owner[p] = l
        d["rows"].append(row)
        d["octs"].append(octs)
        d["featfl"].append(fl)
        d["kps"].append(kp)
        d["kdesc"].append(kd)
        d["uright"].append(ur)
    pos = np.zeros((npts, 3), F)
    desc = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    ref = [0] * npts
    seen = {}
    for s in range(nkf):
        for p in d["rows"][s]:
            if p >= 0:
                seen.setdefault(p, []).append(s)
    for p, l in owner.items():
        pos[p] = land_pos[l]
        desc[p] = noisy(l)
        ref[p] = int(seen[p][rng.integers(len(seen[p]))])
    d["pos"], d["desc"], d["ref"] = pos, desc, ref
    d["bad"] = np.array([p not in owner for p in range(npts)])
    return d


def build_geo_map(M, d):
    M.set_points(0, d["pos"], d["bad"], d["desc"], d["ref"])
    if "first" in d:
        M.set_point_stats(0, d["first"], d["visible"], d["found"])
    for s in range(d["nkf"]):
        M.set_keyframe(s, d["rows"][s], d["octs"][s], d["centre"][s], root=(s == 0))
        M.set_keyframe_features(s, d["featfl"][s])
    M.attach(d)
    for _ in range(2):
        for s in range(d["nkf"]):
            M.update_connections(s)
    M.apply_normal_and_depth(range(d["npts"]))


def chain_dataset():
    """The chain inside one Fuse call.  One landmark, seen by keyframes 0..7; keyframe 0 is the
    target and holds S at its feature; S is also in keyframe 1 (Observations 2).  Point i is in
    keyframe 2 (1 < 2: i is replaced by S, which then has 3).  Point j is in keyframes 3..6 (4 > 3:
    S, carrying i's observation, is replaced by j).  Keyframe 7's feature is free.
    Ids: S = 0, i = 1, j = 2."""
    rng = np.random.default_rng(42)
    centres = [(0.2 * s, 0.0, 0.0) for s in range(8)]
    ids = [0, 0, 1, 2, 2, 2, 2, -1]
    feats = [[(0, ids[s]), (-1, -1)] for s in range(8)]
    return geo_dataset(rng, 8, 8, centres, [(0.5, 0.3, 10.0)], [2], feats, 8, False)


def hand_chain(M):
    d = chain_dataset()
    build_geo_map(M, d)
    M.set_point_stats(0, visible=[2, 3, 5], found=[1, 2, 4])
    out = [M.Fuse(0, [1, 2, 1])]
    out += [[M.keyframe_points(s)[0] for s in range(8)], M.point_bad(0, 3), M.point_replaced(0, 3),
            M.point_stats(0, 3)]
    return out


# i -> S (status 2), S -> j (status 3), the second i is bad by its turn (status 5, not counted);
# every row entry of the landmark ends at j, with i's observation in keyframe 2
HAND_CHAIN = [(2, [2, 3, 5]), [2, 2, 2, 2, 2, 2, 2, -1], [True, True, False], [2, 0, -1],
              [(0, 5, 3, 0), (0, 3, 2, 0), (0, 10, 7, 7)]]


# ---------------------------------------------------------------------------
# random scenes
# ---------------------------------------------------------------------------
NKF, KF_CAP, NPTS, MAX_KF = RC.NKF, RC.KF_CAP, RC.NPTS, RC.MAX_KF
NLAND = 420
SIN_SLOTS = (24, 9)
FUSE_SLOT, FUSE_FROM = 30, (33, 27)     # points from both sides of the slot: statuses 2 and 3
CURRENT_KF_ID = 50


WIDE = dict(nland=640, npts=1200, cap=320, pfeat=0.8)   # rows of more than 256 features


def edit_dataset(seed, stereo, nland=NLAND, npts=NPTS, cap=KF_CAP, pfeat=0.55):
    rng = np.random.default_rng(7000 + seed)
    centres = [(0.25 * s, float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
               for s in range(NKF)]
    land = np.stack([rng.uniform(-5.0, 16.5, nland), rng.uniform(-4.0, 4.0, nland),
                     rng.uniform(8.0, 12.0, nland)], 1)
    land_oct = rng.integers(0, 6, nland)
    # ids: every landmark owns id l; the first npts - nland - 48 also own a second one
    second = {l: nland + l for l in range(npts - nland - 48)}
    feats = []
    for s in range(NKF):
        f = []
        for l in range(nland):
            u, v, _ = project(land[l], centres[s])
            if not (12 < u < W_IMG - 12 and 12 < v < H_IMG - 12) or rng.random() > pfeat:
                continue
            r = rng.random()
            if r < 0.22:
                p = -1
            elif l in second and s >= 8 + (l * 7) % 32:
                p = second[l]
            else:
                p = l
            f.append((l, p))
        f += [(-1, -1)] * 10
        order = rng.permutation(len(f))
        feats.append([f[i] for i in order][:cap])
    d = geo_dataset(rng, NKF, npts, centres, land, land_oct, feats, cap, stereo)
    d["nland"] = nland
    d["first"] = rng.integers(44, 51, npts).tolist()
    d["visible"] = rng.integers(1, 20, npts).tolist()
    d["found"] = rng.integers(1, 12, npts).tolist()
    return d


def run_edit_scene(M, d, check=None):
    """a Fuse call with a repeated list (the only way to status 5), explicit Replace and
    AddObservations calls, two SearchInNeighbors; check(stage) after each.  Returns every
    result."""
    build_geo_map(M, d)
    mono = not d["stereo"]
    npts, nland = d["npts"], d["nland"]
    out = []
    ids = [p for p in d["rows"][FUSE_FROM[0]] if p >= 0]
    ids += [p for p in d["rows"][FUSE_FROM[1]] if p >= 0 and p not in ids]
    out.append(M.Fuse(FUSE_SLOT, ids + [-1] + ids[::3]))
    if check:
        check("fuse")
    # pairs between the two ids of a landmark, where both are still good, then a chain a->b->c
    olds, news = [], []
    bad = M.point_bad(0, npts)
    for l in range(0, npts - nland - 48, 9):
        if not bad[l] and not bad[nland + l]:
            olds.append(l)
            news.append(nland + l)
    chain = [p for p in range(300, 330) if not bad[p] and p not in olds][:3]
    olds += [chain[0], chain[1], chain[0], 5, npts]
    news += [chain[1], chain[2], chain[2], 5, chain[2]]
    out.append(M.replace(olds, news))
    if check:
        check("replace")
    free = [(s, i) for s in (12, 13) for i, p in enumerate(M.keyframe_points(s)) if p < 0][:12]
    fresh = list(range(npts - 40, npts - 28))
    M.set_points(npts - 40, d["pos"][:12] + F(0.5), [False] * 12, d["desc"][:12], [12] * 12)
    out.append(M.add_observations([s for s, _ in free] + [12, 12], [i for _, i in free] + [free[0][1], 0],
                                  fresh + [fresh[1], fresh[0]]))
    if check:
        check("add")
    for k, s in enumerate(SIN_SLOTS):
        out.append(M.search_in_neighbors(s, CURRENT_KF_ID, mono))
        if check:
            check("sin%d" % k)
    out.append(M.search_in_neighbors(SIN_SLOTS[0], 0, mono))
    if check:
        check("sin_id0")
    return out
