"""A pure-Python statement of the reference's covisibility graph and local map, after the text of
KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection
(src/KeyFrame.cc:160-205, 375-515), Tracking::UpdateLocalKeyFrames / UpdateLocalPoints
(src/Tracking.cc:1731-1925) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:457-518).

Dicts keyed by slot, sorted() where the reference iterates a std::map<KeyFrame*, ...> or a
std::set<KeyFrame*>: pointer order is ascending slot order (include/orbg.h).  Observations are
the inverse of the keyframe rows: point p is observed by (slot, idx) iff the slot is live and
its row holds p at idx.  Nothing here imports the library or oracle/.

The scenes (hand cases, random maps, the wide map) are written against a small duck-typed
interface (set_points, set_keyframe, update_connections, ...) that RefMap implements; the GPU
test drives the library through an adapter with the same methods.
"""
import math

import numpy as np

TH = 15
MP_VALID, MP_HAS_OBS = 1, 2
F = np.float32


def scale_factors(nlevels=8, factor=1.2):
    """ORBextractor's mvScaleFactor: float products of the float scaleFactor"""
    s = [F(1.0)]
    for _ in range(1, nlevels):
        s.append(F(s[-1] * F(factor)))
    return s


class RefMap:
    def __init__(self, nlevels=8, factor=1.2):
        self.kf = {}    # slot -> dict
        self.mp = {}    # id -> dict
        self.scale = scale_factors(nlevels, factor)
        self._obs = None

    # ---- mutations ----
    def set_points(self, first, pos, bad, desc, ref):
        for i in range(len(pos)):
            self.mp[first + i] = {"pos": np.array(pos[i], F), "normal": np.zeros(3, F),
                                  "min": F(0), "max": F(0), "bad": bool(bad[i]),
                                  "desc": bytes(bytearray(desc[i])), "ref": int(ref[i])}

    def set_keyframe(self, slot, points, octaves=None, centre=(0.0, 0.0, 0.0), root=False,
                     bad=False):
        octaves = [0] * len(points) if octaves is None else list(octaves)
        k = self.kf.get(slot)
        if k is None or not k["live"]:
            k = {"parent": None, "first": True, "W": {}, "ord": []}
            self.kf[slot] = k
        k.update(live=True, points=[int(p) for p in points], oct=[int(o) for o in octaves],
                 centre=np.array(centre, F), root=bool(root), bad=bool(bad))
        self._obs = None

    def set_point_bad(self, p):
        self.mp[p]["bad"] = True

    def set_parent(self, slot, parent):
        self.kf[slot]["parent"] = parent

    def erase_keyframe(self, s):
        """SetBadFlag's table side as include/orbg.h states it: every row t with W[t][s] > 0"""
        k = self.kf[s]
        k.update(live=False, bad=True, points=[], oct=[], W={}, ord=[])
        for t in sorted(self.kf):
            if self.kf[t]["W"].get(s, 0) > 0:   # EraseConnection
                del self.kf[t]["W"][s]
                self.update_best_covisibles(t)
        self._obs = None

    # ---- the observation table ----
    def observations(self, p):
        """mObservations of point p: [(slot, idx)] in ascending slot order"""
        if self._obs is None:
            self._obs = {}
            for s in sorted(self.kf):
                k = self.kf[s]
                if not k["live"]:
                    continue
                for idx, q in enumerate(k["points"]):
                    if q >= 0:
                        self._obs.setdefault(q, []).append((s, idx))
        return self._obs.get(p, [])

    def is_bad_kf(self, s):
        k = self.kf.get(s)
        return k is None or k["bad"] or not k["live"]

    # ---- KeyFrame.cc ----
    def update_best_covisibles(self, t):
        k = self.kf[t]
        pairs = sorted((w, s) for s, w in k["W"].items())
        k["ord"] = [(s, w) for w, s in reversed(pairs)]      # push_front

    def add_connection(self, t, s, w):
        W = self.kf[t]["W"]
        if s not in W:
            W[s] = w
        elif W[s] != w:
            W[s] = w
        else:
            return
        self.update_best_covisibles(t)

    def update_connections(self, s):
        k = self.kf[s]
        if not k["live"]:
            return
        counter = {}
        for p in k["points"]:
            if p < 0 or self.mp[p]["bad"]:
                continue
            for t, _ in self.observations(p):
                if t == s:
                    continue
                counter[t] = counter.get(t, 0) + 1
        if not counter:
            return
        nmax, kmax, pairs = 0, None, []
        for t in sorted(counter):
            if counter[t] > nmax:
                nmax, kmax = counter[t], t
            if counter[t] >= TH:
                pairs.append((counter[t], t))
                self.add_connection(t, s, counter[t])
        if not pairs:
            pairs.append((nmax, kmax))
            self.add_connection(kmax, s, nmax)
        pairs.sort()
        k["W"] = dict(counter)
        k["ord"] = [(t, w) for w, t in reversed(pairs)]
        if k["first"] and not k["root"]:
            k["parent"] = k["ord"][0][0]
            k["first"] = False

    # ---- readers ----
    def ordered(self, s):
        return list(self.kf[s]["ord"]) if s in self.kf else []

    def weights(self, s):
        return dict(self.kf[s]["W"]) if s in self.kf else {}

    def parent(self, s):
        return self.kf[s]["parent"] if s in self.kf else None

    def neighbours(self, s, n=10):
        return [t for t, _ in self.ordered(s)[:n]]

    # ---- Tracking.cc ----
    def local_keyframes(self, frame_points):
        """(mvpLocalKeyFrames or None, pKFmax or None, frame_points after the nulling)"""
        fp = list(frame_points)
        counter = {}
        for i, p in enumerate(fp):
            if p < 0:
                continue
            if self.mp[p]["bad"]:
                fp[i] = -1
                continue
            for t, _ in self.observations(p):
                counter[t] = counter.get(t, 0) + 1
        if not counter:
            return None, None, fp
        best, kmax, local, marked = 0, None, [], set()
        for t in sorted(counter):
            if self.is_bad_kf(t):
                continue
            if counter[t] > best:
                best, kmax = counter[t], t
            local.append(t)
            marked.add(t)
        for kf in list(local):                 # the end iterator is fixed before the appends
            if len(local) > 80:
                break
            for nb in self.neighbours(kf, 10):
                if not self.is_bad_kf(nb) and nb not in marked:
                    local.append(nb)
                    marked.add(nb)
                    break
            for ch in sorted(c for c in self.kf if self.kf[c]["parent"] == kf):
                if not self.is_bad_kf(ch) and ch not in marked:
                    local.append(ch)
                    marked.add(ch)
                    break
            par = self.kf[kf]["parent"]
            if par is not None and par not in marked:
                local.append(par)
                marked.add(par)
                break                          # Tracking.cc:1912
        return local, kmax, fp

    def local_points(self, local_kfs, frame_points):
        """[(id, flags)] of mvpLocalMapPoints in order; flags as SearchLocalPoints reads them"""
        own = set(p for p in frame_points if p >= 0)
        out, seen = [], set()
        for kf in local_kfs:
            k = self.kf.get(kf)
            if k is None or not k["live"]:
                continue
            for p in k["points"]:
                if p < 0 or p in seen:
                    continue
                if not self.mp[p]["bad"]:
                    seen.add(p)
                    fl = (0 if p in own else MP_VALID) | (MP_HAS_OBS if self.observations(p) else 0)
                    out.append((p, fl))
        return out

    # ---- MapPoint.cc ----
    def normal_and_depth(self, p):
        """The float statement (include/orbg.h): (normal[3], min, max) as float32, or None when
        the point is left untouched."""
        m = self.mp[p]
        obs = self.observations(p)
        if m["bad"] or not obs:
            return None
        ridx = [i for s, i in obs if s == m["ref"]]
        if not ridx:
            return None
        normal = [F(0), F(0), F(0)]
        dist = None
        for s, _ in obs:
            O = self.kf[s]["centre"]
            d = [m["pos"][i] - O[i] for i in range(3)]                  # float
            sq = float(d[0]) * float(d[0])                                # cv::norm: double
            sq += float(d[1]) * float(d[1])
            sq += float(d[2]) * float(d[2])
            nrm = math.sqrt(sq)
            a = F(1.0 / nrm)                                              # the float alpha
            normal = [F(normal[i] + F(d[i] * a)) for i in range(3)]
            if s == m["ref"]:
                dist = F(nrm)
        level = self.kf[m["ref"]]["oct"][ridx[0]]
        maxd = F(dist * self.scale[level])
        mind = F(maxd / self.scale[-1])
        inv = F(1.0 / len(obs))
        return np.array([F(v * inv) for v in normal], F), mind, maxd

    def normal_and_depth64(self, p):
        """The same in float64 from the float32 inputs (scale factors included)"""
        m = self.mp[p]
        obs = self.observations(p)
        if m["bad"] or not obs or not [i for s, i in obs if s == m["ref"]]:
            return None
        pos = m["pos"].astype(np.float64)
        normal = np.zeros(3)
        for s, _ in obs:
            d = pos - self.kf[s]["centre"].astype(np.float64)
            normal += d / np.linalg.norm(d)
        ref = self.kf[m["ref"]]
        dist = np.linalg.norm(pos - ref["centre"].astype(np.float64))
        level = ref["oct"][[i for s, i in obs if s == m["ref"]][0]]
        maxd = dist * float(self.scale[level])
        return normal / len(obs), maxd / float(self.scale[-1]), maxd

    def apply_normal_and_depth(self, ids):
        for p in ids:
            r = self.normal_and_depth(p)
            if r is not None:
                self.mp[p]["normal"], self.mp[p]["min"], self.mp[p]["max"] = r


def check_normal_depth_bounds(M, ids):
    """The float statement against the float64 one, within the bounds the rounding count gives:
    each normal component within (n + 4) * 2^-24 (n float additions of terms <= 1 plus the
    products' and the final scaling's roundings), the distances within 8 * 2^-24 relative
    (three to four roundings each), on scenes where |Pos - O| >= max(|Pos|, |O|) / 4 so the
    subtraction's cancellation stays inside the bound.  Returns the number of points checked."""
    eps, n_checked = 2.0 ** -24, 0
    for p in ids:
        a, b = M.normal_and_depth(p), M.normal_and_depth64(p)
        assert (a is None) == (b is None)
        if a is None:
            continue
        m = M.mp[p]
        obs = M.observations(p)
        for s, _ in obs:
            O = M.kf[s]["centre"].astype(np.float64)
            P = m["pos"].astype(np.float64)
            assert np.linalg.norm(P - O) >= 0.25 * max(np.linalg.norm(P), np.linalg.norm(O))
        assert np.all(np.abs(a[0].astype(np.float64) - b[0]) <= (len(obs) + 4) * eps), p
        assert abs(float(a[1]) - b[1]) <= 8 * eps * b[1], p
        assert abs(float(a[2]) - b[2]) <= 8 * eps * b[2], p
        n_checked += 1
    return n_checked


def snapshot(M, slots):
    """every W row, ordered list with weights, neighbours and parent of the listed slots"""
    return {s: {"W": M.weights(s), "ord": M.ordered(s), "neigh": M.neighbours(s),
                "parent": M.parent(s)} for s in slots}


# ---------------------------------------------------------------------------
# hand cases: each builds a map on M (duck-typed) and returns what it reads
# ---------------------------------------------------------------------------
class _Ids:
    def __init__(self):
        self.n = 0

    def take(self, k):
        r = list(range(self.n, self.n + k))
        self.n += k
        return r


def _plain_points(M, n):
    pos = [(0.01 * i, 0.0, 5.0) for i in range(n)]
    M.set_points(0, pos, [False] * n, [[i % 251] * 32 for i in range(n)], [0] * n)


HAND_POINTS = 256


def hand_threshold(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    a, b = ids.take(15), ids.take(14)
    M.set_keyframe(0, a + b, root=True)
    M.set_keyframe(1, a)
    M.set_keyframe(2, b)
    M.update_connections(0)
    return snapshot(M, [0, 1, 2])


HAND_THRESHOLD = {
    0: {"W": {1: 15, 2: 14}, "ord": [(1, 15)], "neigh": [1], "parent": None},
    1: {"W": {0: 15}, "ord": [(0, 15)], "neigh": [0], "parent": None},
    2: {"W": {}, "ord": [], "neigh": [], "parent": None},
}


def hand_fallback_tie(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    a, b = ids.take(5), ids.take(5)
    M.set_keyframe(0, a + b, root=True)
    M.set_keyframe(1, a)
    M.set_keyframe(2, b)
    M.update_connections(0)
    return snapshot(M, [0, 1, 2])


HAND_FALLBACK_TIE = {
    0: {"W": {1: 5, 2: 5}, "ord": [(1, 5)], "neigh": [1], "parent": None},
    1: {"W": {0: 5}, "ord": [(0, 5)], "neigh": [0], "parent": None},
    2: {"W": {}, "ord": [], "neigh": [], "parent": None},
}


def hand_equal_weights(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    a, b, c = ids.take(16), ids.take(16), ids.take(16)
    M.set_keyframe(0, a + b + c, root=True)
    M.set_keyframe(1, a)
    M.set_keyframe(2, b)
    M.set_keyframe(3, c)
    M.update_connections(0)
    return snapshot(M, [0])


HAND_EQUAL_WEIGHTS = {
    0: {"W": {1: 16, 2: 16, 3: 16}, "ord": [(3, 16), (2, 16), (1, 16)], "neigh": [3, 2, 1],
        "parent": None},
}


def hand_stale_and_unchanged(M):
    """A stale sub-threshold weight enters a neighbour's list through AddConnection; an
    unchanged weight does not re-sort."""
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    s12, s13, s01, s02 = ids.take(3), ids.take(20), ids.take(15), ids.take(2)
    M.set_keyframe(1, s12 + s13 + s01)
    M.set_keyframe(2, s12 + s02)
    M.set_keyframe(3, s13)
    M.update_connections(1)             # kf 0 is not there yet
    first = snapshot(M, [1, 3])
    M.set_keyframe(0, s01 + s02)
    M.update_connections(0)             # AddConnection(1 <- 0, 15) re-sorts all of row 1
    second = snapshot(M, [0, 1])
    M.update_connections(1)             # AddConnection(0 <- 1, 15): unchanged, row 0 stays
    third = snapshot(M, [0, 1, 3])
    return [first, second, third]


HAND_STALE_AND_UNCHANGED = [
    {1: {"W": {2: 3, 3: 20}, "ord": [(3, 20)], "neigh": [3], "parent": 3},
     3: {"W": {1: 20}, "ord": [(1, 20)], "neigh": [1], "parent": None}},
    {0: {"W": {1: 15, 2: 2}, "ord": [(1, 15)], "neigh": [1], "parent": 1},
     1: {"W": {0: 15, 2: 3, 3: 20}, "ord": [(3, 20), (0, 15), (2, 3)], "neigh": [3, 0, 2],
         "parent": 3}},
    {0: {"W": {1: 15, 2: 2}, "ord": [(1, 15)], "neigh": [1], "parent": 1},
     1: {"W": {0: 15, 2: 3, 3: 20}, "ord": [(3, 20), (0, 15)], "neigh": [3, 0], "parent": 3},
     3: {"W": {1: 20}, "ord": [(1, 20)], "neigh": [1], "parent": None}},
]


def hand_parent_once(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    s01, s12, s02 = ids.take(20), ids.take(30), ids.take(16)
    M.set_keyframe(0, s01 + s02, root=True)
    M.set_keyframe(1, s01 + s12)
    M.update_connections(1)
    M.update_connections(0)             # root: never a parent
    a = (M.parent(0), M.parent(1))
    M.set_keyframe(2, s12 + s02)
    M.update_connections(2)
    M.update_connections(1)             # its best is now 2, its parent stays 0
    return [a, (M.parent(0), M.parent(1), M.parent(2)), M.ordered(1)]


HAND_PARENT_ONCE = [(None, 0), (None, 0, 1), [(2, 30), (0, 20)]]


def hand_local_80_81(M, ninit):
    """ninit keyframes with one vote each; keyframe 100 is keyframe 0's neighbour and child."""
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    own = ids.take(ninit)
    sh = ids.take(15)
    M.set_keyframe(0, [own[0]] + sh, root=True)
    for i in range(1, ninit):
        M.set_keyframe(i, [own[i]])
    M.set_keyframe(100, sh)
    M.update_connections(100)
    return M.local_keyframes(own)[:2]


HAND_LOCAL_80 = (list(range(80)) + [100], 0)
HAND_LOCAL_81 = (list(range(81)), 0)


def hand_parent_break(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    own, sh = ids.take(4), ids.take(15)
    M.set_keyframe(0, [own[0]], root=True)
    M.set_keyframe(1, [own[1], own[3]] + sh)        # two votes: pKFmax
    M.set_keyframe(2, [own[2]])
    M.set_keyframe(5, [])
    M.set_keyframe(6, sh)
    M.update_connections(6)             # 6 becomes keyframe 1's neighbour and child
    M.set_parent(0, 5)
    return M.local_keyframes(own)[:2]


HAND_PARENT_BREAK = ([0, 1, 2, 5], 1)


def hand_bad_skipped(M):
    _plain_points(M, HAND_POINTS)
    ids = _Ids()
    own, s03, s04, s02 = ids.take(1), ids.take(20), ids.take(16), ids.take(15)
    M.set_keyframe(0, own + s03 + s04 + s02, root=True)
    M.set_keyframe(2, s02)
    M.set_keyframe(3, s03)
    M.set_keyframe(4, s04)
    M.set_keyframe(7, [])
    for s in (2, 3, 4):
        M.update_connections(s)         # each becomes a child of 0; 0's list: 3, 4, 2
    M.set_parent(7, 0)
    M.erase_keyframe(2)                 # an erased child keeps its parent until the caller's repair
    M.set_keyframe(3, s03, bad=True)    # SetBadFlag under way: bad, row still standing
    return [M.ordered(0), M.local_keyframes(own)[:2]]


HAND_BAD_SKIPPED = [[(3, 20), (4, 16)], ([0, 4, 7], 0)]


def hand_empty(M):
    _plain_points(M, HAND_POINTS)
    M.set_keyframe(0, [0, 1, 2], root=True)
    M.set_keyframe(1, [3, 4])
    M.set_point_bad(1)
    M.update_connections(1)             # KFcounter empty: nothing changes
    return [snapshot(M, [0, 1]), M.local_keyframes([-1, 1, 9, -1]), M.local_keyframes([])]


HAND_EMPTY = [
    {0: {"W": {}, "ord": [], "neigh": [], "parent": None},
     1: {"W": {}, "ord": [], "neigh": [], "parent": None}},
    (None, None, [-1, -1, 9, -1]),
    (None, None, []),
]

HAND_CASES = [
    (hand_threshold, HAND_THRESHOLD),
    (hand_fallback_tie, HAND_FALLBACK_TIE),
    (hand_equal_weights, HAND_EQUAL_WEIGHTS),
    (hand_stale_and_unchanged, HAND_STALE_AND_UNCHANGED),
    (hand_parent_once, HAND_PARENT_ONCE),
    (lambda M: hand_local_80_81(M, 80), HAND_LOCAL_80),
    (lambda M: hand_local_80_81(M, 81), HAND_LOCAL_81),
    (hand_parent_break, HAND_PARENT_BREAK),
    (hand_bad_skipped, HAND_BAD_SKIPPED),
    (hand_empty, HAND_EMPTY),
]
HAND_NAMES = ["threshold", "fallback_tie", "equal_weights", "stale_and_unchanged", "parent_once",
              "local_80", "local_81", "parent_break", "bad_skipped", "empty"]


# ---------------------------------------------------------------------------
# random maps
# ---------------------------------------------------------------------------
NKF, KF_CAP, NPTS, NFRAMES, FRAME_CAP = 64, 128, 2048, 6, 160
LKF_CAP, LP_CAP = 64, 2048


def map_dataset(seed, nkf=NKF, cap=KF_CAP, npts=NPTS, nframes=NFRAMES):
    """Points at distance >= 4 of the origin, camera centres within 1 of it (so |Pos - O| >=
    max(|Pos|, |O|) / 4); keyframe s sees a random part of a window of points that moves with
    s (covisibility weights on both sides of 15 a few slots apart) plus a few far ones."""
    rng = np.random.default_rng(1000 + seed)
    d = {"nkf": nkf, "cap": cap, "npts": npts}
    dirs = rng.normal(size=(npts, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    d["pos"] = (dirs * rng.uniform(4.0, 20.0, (npts, 1))).astype(F)
    d["bad"] = rng.random(npts) < 0.05
    d["desc"] = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    d["centre"] = rng.uniform(-0.55, 0.55, (nkf, 3)).astype(F)
    step, width = npts // nkf, 5 * (npts // nkf)
    rows, octs = [], []
    for s in range(nkf):
        lo = min(s * step, npts - width)
        near = lo + rng.choice(width, int(rng.integers(70, 100)), replace=False)
        far = rng.choice(npts, int(rng.integers(0, 8)), replace=False)
        ids = list(dict.fromkeys(near.tolist() + far.tolist()))
        row = np.full(int(rng.integers(len(ids), cap + 1)), -1, np.int64)
        row[rng.choice(len(row), len(ids), replace=False)] = ids
        rows.append(row.tolist())
        octs.append(rng.integers(0, 8, len(row)).tolist())
    d["rows"], d["octs"] = rows, octs
    # mpRefKF: one of the observers (the lowest or a random one)
    seen = {}
    for s, row in enumerate(rows):
        for p in row:
            if p >= 0:
                seen.setdefault(p, []).append(s)
    d["ref"] = [int(seen[p][0 if rng.random() < 0.5 else rng.integers(len(seen[p]))])
                if p in seen else 0 for p in range(npts)]
    # a second row for the overwritten keyframes
    d["rows2"], d["octs2"] = {}, {}
    for s in rng.choice(np.arange(1, nkf), 3, replace=False).tolist():
        lo = min(s * step, npts - width)
        ids = (lo + rng.choice(width, 60, replace=False)).tolist()
        d["rows2"][s], d["octs2"][s] = ids, rng.integers(0, 8, len(ids)).tolist()
    d["erase"] = sorted(rng.choice(np.arange(1, nkf), 3, replace=False).tolist())
    d["flag_bad"] = int(rng.choice([s for s in range(1, nkf) if s not in d["erase"]]))
    d["late_bad"] = rng.choice(npts, 40, replace=False).tolist()
    frames = []
    for f in range(nframes):
        s = int(rng.integers(nkf))
        lo = min(s * step, npts - width)
        ids = (lo + rng.choice(width, int(rng.integers(40, 120)), replace=False)).tolist()
        fp = np.full(int(rng.integers(len(ids), FRAME_CAP + 1)), -1, np.int64)
        fp[rng.choice(len(fp), len(ids), replace=False)] = ids
        frames.append(fp.tolist())
    frames[-1] = [-1] * 7                 # an empty counter
    d["frames"] = frames
    return d


def build_map(M, d):
    """ProcessNewKeyFrame's order: every keyframe is added, then its UpdateConnections runs"""
    M.set_points(0, d["pos"], d["bad"], d["desc"], d["ref"])
    for s in range(d["nkf"]):
        M.set_keyframe(s, d["rows"][s], d["octs"][s], d["centre"][s], root=(s == 0))
        M.update_connections(s)


def mutate_map(M, d):
    """points going bad, set_keyframe overwrites, erased keyframes, a keyframe flagged bad, then
    the UpdateConnections a local BA would run"""
    for p in d["late_bad"]:
        M.set_point_bad(p)
    for s in sorted(d["rows2"]):
        M.set_keyframe(s, d["rows2"][s], d["octs2"][s], d["centre"][s])
        M.update_connections(s)
    for s in d["erase"]:
        M.erase_keyframe(s)
    s = d["flag_bad"]
    row = d["rows2"].get(s, d["rows"][s])
    octv = d["octs2"].get(s, d["octs"][s])
    M.set_keyframe(s, row, octv, d["centre"][s], bad=True)
    for s in range(0, d["nkf"], 5):
        M.update_connections(s)


# ---------------------------------------------------------------------------
# the wide map: one keyframe connected to more than 300 others, a frame voting for more than 256
# ---------------------------------------------------------------------------
WIDE_K, WIDE_CAP, WIDE_PTS, WIDE_N, WIDE_HUB = 1024, 128, 2048, 320, 700


def wide_slots():
    return [3 * j + 1 for j in range(WIDE_N) if 3 * j + 1 != WIDE_HUB]


def wide_dataset():
    rng = np.random.default_rng(77)
    d = {"pos": [(0.01 * i, 0.3, 6.0) for i in range(WIDE_PTS)], "bad": [False] * WIDE_PTS,
         "desc": rng.integers(0, 256, (WIDE_PTS, 32), dtype=np.uint8), "ref": [WIDE_HUB] * WIDE_PTS}
    popular = list(range(60))
    rows = {WIDE_HUB: popular + list(range(1000, 1030))}
    for j, s in enumerate(wide_slots()):
        rows[s] = popular[:15 + j % 40] + [100 + 5 * j + k for k in range(5)]
    d["rows"] = rows
    d["frame"] = popular + [-1, 1001]
    return d


def build_wide(M, d):
    M.set_points(0, d["pos"], d["bad"], d["desc"], d["ref"])
    for s in sorted(d["rows"]):
        M.set_keyframe(s, d["rows"][s], root=(s == 1))
    M.update_connections(WIDE_HUB)
