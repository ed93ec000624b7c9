"""A pure-Python statement of LocalMapping::KeyFrameCulling / MapPointCulling
(src/LocalMapping.cc:227-270, 804-877), KeyFrame::SetBadFlag with SetNotErase / SetErase
(src/KeyFrame.cc:560-720) and MapPoint::EraseObservation / SetBadFlag / GetFoundRatio
(src/MapPoint.cc:159-232, 325-329) over tests/ref_map.py's RefMap, which it subclasses.

Observations() is the sum over the point's observations of 2 for a STEREO feature and 1
otherwise; pointer order is ascending slot order, as everywhere in the Map.  Nothing here imports
the library or oracle/.  The scenes are written against RefMap's duck-typed interface extended
with the calls below, so one scene function drives this class and the GPU adapter.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402

FEAT_STEREO, FEAT_CLOSE = 1, 2
KEPT, ERASED, MARKED, SKIPPED = 0, 1, 2, 3
F = np.float32


class RefCullMap(R.RefMap):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.stats = {}          # id -> [mnFirstKFid, mnVisible, mnFound]
        self._inv = {}           # id -> {slot: idx}, current whenever _obs is not None
        self.n_promoted = self.n_fallback = 0

    # ---- the observation table, kept current under this class's own edits ----
    def observations(self, p):
        if self._obs is None:
            self._inv = {}
            for s in sorted(self.kf):
                k = self.kf[s]
                if k["live"]:
                    for idx, q in enumerate(k["points"]):
                        if q >= 0:
                            self._inv.setdefault(q, {})[s] = idx
            self._obs = {}
        return sorted(self._inv.get(p, {}).items())

    def _drop(self, s, idx):
        """mvpMapPoints[idx] of s becomes NULL"""
        self.observations(0)
        p = self.kf[s]["points"][idx]
        self.kf[s]["points"][idx] = -1
        if p >= 0:
            self._inv.get(p, {}).pop(s, None)

    def n_obs(self, p):
        return sum(2 if self.feat(s, i) & FEAT_STEREO else 1 for s, i in self.observations(p))

    # ---- new state ----
    def set_keyframe(self, slot, points, octaves=None, centre=(0.0, 0.0, 0.0), root=False,
                     bad=False):
        k = self.kf.get(slot)
        fresh = k is None or not k["live"]
        super().set_keyframe(slot, points, octaves, centre, root, bad)
        if fresh:
            self.kf[slot].update(feat=[], not_erase=False, to_be_erased=False)

    def feat(self, s, idx):
        f = self.kf[s].get("feat", [])
        return f[idx] if idx < len(f) else 0

    def set_keyframe_features(self, slot, flags):
        if slot in self.kf and self.kf[slot]["live"]:
            self.kf[slot]["feat"] = [int(f) for f in flags]

    def set_point_stats(self, first, first_kf=None, visible=None, found=None):
        for k, arr in enumerate((first_kf, visible, found)):
            if arr is not None:
                for i, v in enumerate(arr):
                    self.stats.setdefault(first + i, [0, 1, 1])[k] = int(v)

    def point_stats(self, first, n):
        """[(mnFirstKFid, mnVisible, mnFound, Observations())]"""
        return [tuple(self.stats.get(p, [0, 1, 1])) + (self.n_obs(p),)
                for p in range(first, first + n)]

    def increase_visible(self, ids, amount=1, mask=None):
        for i, p in enumerate(ids):
            if p >= 0 and (mask is None or mask[i]):
                self.stats.setdefault(p, [0, 1, 1])[1] += amount

    def increase_found(self, ids, amount=1):
        for p in ids:
            if p >= 0:
                self.stats.setdefault(p, [0, 1, 1])[2] += amount

    def keyframe_points(self, slot):
        k = self.kf.get(slot)
        return list(k["points"]) if k is not None and k["live"] else []

    def point_refs(self, first, n):
        return [self.mp[p]["ref"] for p in range(first, first + n)]

    def point_bad(self, first, n):
        return [self.mp[p]["bad"] for p in range(first, first + n)]

    # ---- MapPoint.cc ----
    def mp_set_bad(self, p):
        self.mp[p]["bad"] = True
        for s, idx in self.observations(p):
            self._drop(s, idx)                      # EraseMapPointMatch

    # ---- KeyFrame.cc ----
    def set_not_erase(self, slot, on):
        """SetNotErase (on) / SetErase once mspLoopEdges is empty; returns erased"""
        k = self.kf.get(slot)
        if k is None or not k["live"]:
            return False
        if on:
            k["not_erase"] = True
            return False
        k["not_erase"] = False
        return k["to_be_erased"] and self.set_bad_flag(slot) == ERASED

    def set_bad_flag(self, s):
        k = self.kf.get(s)
        if k is None or not k["live"] or k["root"]:
            return 0
        if k["not_erase"]:
            k["to_be_erased"] = True
            return MARKED
        for t in sorted(self.kf):
            if self.kf[t]["W"].get(s, 0) > 0:       # EraseConnection
                del self.kf[t]["W"][s]
                self.update_best_covisibles(t)
        for idx in range(len(k["points"])):
            p = k["points"][idx]
            if p < 0:
                continue
            self._drop(s, idx)
            m = self.mp[p]
            if m["bad"]:
                continue                            # no observations: EraseObservation finds none
            obs = self.observations(p)
            if m["ref"] == s:
                m["ref"] = obs[0][0] if obs else -1
            if self.n_obs(p) <= 2:
                self.mp_set_bad(p)
        par = k["parent"]
        k.update(live=False, bad=True, points=[], oct=[], W={}, ord=[], feat=[], not_erase=False,
                 to_be_erased=False)
        # the spanning tree
        children = sorted(c for c in self.kf if self.kf[c]["parent"] == s and self.kf[c]["live"])
        cands = [] if par is None else [par]
        while children:
            best, pc, pp = -1, None, None
            for c in children:
                if self.kf[c]["bad"]:
                    continue
                for t, _ in self.kf[c]["ord"]:
                    for cand in sorted(cands):
                        if t == cand:
                            w = self.kf[c]["W"].get(t, 0)       # GetWeight
                            if w > best:
                                best, pc, pp = w, c, t
            if pc is None:
                break
            self.kf[pc]["parent"] = pp
            self.n_promoted += pp != par
            cands.append(pc)
            children.remove(pc)
        for c in children:
            self.kf[c]["parent"] = par
            self.n_fallback += 1
        return ERASED

    # ---- LocalMapping.cc ----
    def cull_score(self, t, monocular):
        """(nMPs, nRedundantObservations) of keyframe t as the map stands"""
        k = self.kf[t]
        nmps = nred = 0
        for idx, p in enumerate(k["points"]):
            if p < 0 or self.mp[p]["bad"]:
                continue
            if not monocular and not self.feat(t, idx) & FEAT_CLOSE:
                continue
            nmps += 1
            if self.n_obs(p) > 3:
                lvl = k["oct"][idx]
                n = sum(1 for u, j in self.observations(p)
                        if u != t and self.kf[u]["oct"][j] <= lvl + 1)
                nred += n >= 3
        return nmps, nred

    def cullable(self, t):
        k = self.kf.get(t)
        return not (k is None or k["root"] or not k["live"] or k["bad"])

    def keyframe_culling(self, slot, monocular):
        """[(slot, status, nMPs, nRedundant)] per entry of slot's ordered list"""
        out = []
        for t in [t for t, _ in self.ordered(slot)]:
            if not self.cullable(t):
                out.append((t, SKIPPED, 0, 0))
                continue
            nmps, nred = self.cull_score(t, monocular)
            st = KEPT
            if float(nred) > 0.9 * float(nmps):
                st = self.set_bad_flag(t)
            out.append((t, st, nmps, nred))
        return out

    def point_culling(self, recent, current_kf_id, monocular):
        """(mlpRecentAddedMapPoints after the call, status per input position)"""
        th = 2 if monocular else 3
        keep, status = [], []
        for p in recent:
            first, vis, found = self.stats.get(p, [0, 1, 1])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = F(found) / F(vis)
            if self.mp[p]["bad"]:
                st = 1
            elif ratio < F(0.25):
                self.mp_set_bad(p)
                st = 2
            elif current_kf_id - first >= 2 and self.n_obs(p) <= th:
                self.mp_set_bad(p)
                st = 3
            elif current_kf_id - first >= 3:
                st = 4
            else:
                st = 0
                keep.append(p)
            status.append(st)
        return keep, status


def state(M, nkf, npts):
    """everything the tests compare: rows, point flags, mpRefKF, stats, W, ordered lists, neigh,
    parents"""
    return {"rows": [M.keyframe_points(s) for s in range(nkf)],
            "bad": M.point_bad(0, npts), "ref": M.point_refs(0, npts),
            "stats": M.point_stats(0, npts), "graph": R.snapshot(M, range(nkf))}


# ---------------------------------------------------------------------------
# hand cases: each builds a map on M (duck-typed) and returns what it reads
# ---------------------------------------------------------------------------
HAND_POINTS = 256
LINK = 200          # link points: shared with the culling slot, then set bad


def _target_scene(M, targets, helpers, links=None):
    """Slot 0 (root) is the culling slot.  targets / helpers: {slot: (points, octaves or None,
    feature flags or None)}.  Target t shares links[t] link points (default 1) with slot 0,
    which put it on slot 0's ordered list and are then set bad, so they count nowhere."""
    R._plain_points(M, HAND_POINTS)
    links = links or {}
    nxt, own, link_rows = LINK, [], {}
    for t in sorted(targets):
        n = links.get(t, 1)
        link_rows[t] = list(range(nxt, nxt + n))
        own += link_rows[t]
        nxt += n
    M.set_keyframe(0, own, root=True)
    for t, (pts, octs, fl) in sorted(targets.items()):
        n = len(link_rows[t])
        M.set_keyframe(t, list(pts) + link_rows[t], (list(octs) if octs else [0] * len(pts)) + [0] * n)
        M.set_keyframe_features(t, (list(fl) if fl else [0] * len(pts)) + [0] * n)
        M.set_parent(t, 0)
    for h, (pts, octs, fl) in sorted(helpers.items()):
        M.set_keyframe(h, list(pts), list(octs) if octs else None)
        if fl:
            M.set_keyframe_features(h, fl)
    M.update_connections(0)
    for p in own:
        M.set_point_bad(p)


def hand_cull_threshold(M, nred):
    """a target of 10 points, nred of them seen by three helpers; nred None: no good point"""
    pts = list(range(10))
    if nred is None:
        _target_scene(M, {1: ([], None, None)}, {})
    else:
        _target_scene(M, {1: (pts, None, None)}, {h: (pts[:nred], None, None) for h in (5, 6, 7)})
    rec = M.keyframe_culling(0, True)
    return [rec, M.keyframe_points(1), M.point_stats(0, 2)]


HAND_THRESHOLD_9 = [[(1, 0, 10, 9)], list(range(10)) + [LINK], [(0, 1, 1, 4), (0, 1, 1, 4)]]
HAND_THRESHOLD_10 = [[(1, 1, 10, 10)], [], [(0, 1, 1, 3), (0, 1, 1, 3)]]
HAND_THRESHOLD_0 = [[(1, 0, 0, 0)], [LINK], [(0, 1, 1, 0), (0, 1, 1, 0)]]


def hand_cull_octave_gate(M):
    """point 0 at level 2 seen at levels 3, 3, 3: redundant; point 1 at 3, 3, 4: not"""
    _target_scene(M, {1: ([0, 1], [2, 2], None)},
                  {5: ([0, 1], [3, 3], None), 6: ([0, 1], [3, 3], None), 7: ([0, 1], [3, 4], None)})
    return M.keyframe_culling(0, True)


HAND_OCTAVE_GATE = [(1, 0, 2, 1)]


def hand_cull_observation_count(M):
    """point 0: target + 2 mono observers (Observations 3); point 1: target + a STEREO and a
    mono observer (Observations 4, two others); point 2: target + 3 mono observers (4, three
    others): only point 2 is redundant"""
    _target_scene(M, {1: ([0, 1, 2], None, None)},
                  {5: ([0, 1, 2], None, [0, FEAT_STEREO, 0]), 6: ([0, 1, 2], None, None),
                   7: ([2], None, None)})
    return [M.point_stats(0, 3), M.keyframe_culling(0, True)]


HAND_OBSERVATION_COUNT = [[(0, 1, 1, 3), (0, 1, 1, 4), (0, 1, 1, 4)], [(1, 0, 3, 1)]]


def hand_cull_close_filter(M, monocular):
    """four points, all redundant, two of them CLOSE"""
    pts = [0, 1, 2, 3]
    _target_scene(M, {1: (pts, None, [FEAT_CLOSE, 0, FEAT_CLOSE | FEAT_STEREO, FEAT_STEREO])},
                  {h: (pts, None, None) for h in (5, 6, 7, 8)})
    return M.keyframe_culling(0, monocular)


HAND_CLOSE_MONO = [(1, 1, 4, 4)]
HAND_CLOSE_STEREO = [(1, 1, 2, 2)]


def hand_cull_order_first_saves_second(M):
    """ten points seen by targets 1 and 2 and helpers 5 and 6: either target alone is
    redundant, and erasing 1 (first on the list) leaves 2 with two other observers"""
    pts = list(range(10))
    _target_scene(M, {1: (pts, None, None), 2: (pts, None, None)},
                  {5: (pts, None, None), 6: (pts, None, None)}, links={1: 16, 2: 15})
    return [M.ordered(0), M.keyframe_culling(0, True), M.point_stats(0, 1)]


HAND_ORDER_SAVES = [[(1, 16), (2, 15)], [(1, 1, 10, 10), (2, 0, 10, 0)], [(0, 1, 1, 3)]]


def hand_cull_order_first_dooms_second(M):
    """target 2: eight redundant points and two seen only by 1, 2 and 5 (8 > 9 is false: kept
    at the start).  Erasing 1 leaves those two with Observations 2: they go bad, leave row 2,
    and 2 is now 8 of 8."""
    a, b, c = list(range(0, 8)), [8, 9], list(range(10, 29))
    _target_scene(M, {1: (b + c, None, None), 2: (a + b, None, None)},
                  {5: (a + b + c, None, None), 6: (a + c, None, None), 7: (a + c, None, None)},
                  links={1: 16, 2: 15})
    start = M.point_bad(8, 2)
    return [start, M.keyframe_culling(0, True), M.point_bad(8, 2), M.keyframe_points(5)[8:10]]


HAND_ORDER_DOOMS = [[False, False], [(1, 1, 21, 19), (2, 1, 8, 8)], [True, True], [-1, -1]]


def hand_ref_handover(M):
    """mpRefKF of the erased keyframe's points: to the lowest remaining slot, to -1 when none
    remains, untouched when it was another keyframe"""
    R._plain_points(M, HAND_POINTS)
    M.set_points(0, [(0.0, 0.0, 5.0)] * 3, [False] * 3, [[7] * 32] * 3, [2, 2, 5])
    M.set_keyframe(0, [], root=True)
    M.set_keyframe(2, [0, 1, 2])
    M.set_parent(2, 0)
    for s in (3, 5, 7):
        M.set_keyframe(s, [0, 2])
    st = M.set_bad_flag(2)
    return [st, M.point_refs(0, 3), M.point_bad(0, 3), M.point_stats(0, 3)]


HAND_REF_HANDOVER = [1, [3, -1, 5], [False, True, False],
                     [(0, 1, 1, 3), (0, 1, 1, 0), (0, 1, 1, 3)]]


def hand_not_erase(M):
    pts = list(range(10))
    _target_scene(M, {1: (pts, None, None)}, {h: (pts, None, None) for h in (5, 6, 7)})
    none_pending = M.set_not_erase(5, False)         # SetErase with no pending mark
    M.set_not_erase(1, True)
    rec = M.keyframe_culling(0, True)
    row, direct = M.keyframe_points(1), M.set_bad_flag(1)
    erased = M.set_not_erase(1, False)
    return [none_pending, M.keyframe_points(5), rec, row, direct, erased, M.keyframe_points(1),
            M.ordered(0), M.point_stats(0, 1)]


HAND_NOT_ERASE = [False, list(range(10)), [(1, 2, 10, 10)], list(range(10)) + [LINK], 2, True, [],
                  [], [(0, 1, 1, 3)]]


def hand_tree_repair(M):
    """Erased: 2, parent 1.  Children: 3 (16 with 1), 4 (18 with 3), 5 (3 with 3, below the
    threshold: on 5's list only through the re-sort), 6 (bad, 30 with 1), 7 (16 with 1 and with
    3: 3 comes first on its list), 8 (no link)."""
    R._plain_points(M, 400)
    ids = R._Ids()
    share = {}
    for a, b, n in ((2, 3, 20), (2, 4, 20), (2, 5, 20), (2, 6, 20), (2, 7, 20), (2, 8, 20),
                    (1, 3, 16), (3, 4, 18), (3, 5, 3), (1, 6, 30), (1, 7, 16), (3, 7, 16),
                    (0, 1, 15)):
        share[(a, b)] = ids.take(n)
    rows = {s: [] for s in range(9)}
    for (a, b), pts in share.items():
        rows[a] += pts
        rows[b] += pts
    for s in range(9):
        M.set_keyframe(s, rows[s], root=(s == 0))
    for s in range(9):
        M.update_connections(s)
    M.set_parent(1, 0)
    M.set_parent(2, 1)
    for c in (3, 4, 5, 6, 7, 8):
        M.set_parent(c, 2)
    M.set_keyframe(6, rows[6], bad=True)
    before = M.ordered(5)
    st = M.set_bad_flag(2)
    return [before, st, M.ordered(5), M.ordered(7), [M.parent(s) for s in range(9)],
            M.weights(1), M.keyframe_points(3)[:20]]


HAND_TREE_REPAIR = [[(2, 20)], 1, [(3, 3)], [(3, 16), (1, 16)],
                    [None, 0, 1, 1, 3, 3, 1, 3, 1], {0: 15, 3: 16, 6: 30, 7: 16}, [-1] * 20]


def hand_root(M):
    """the root on the list is skipped; SetBadFlag of the root does nothing"""
    R._plain_points(M, HAND_POINTS)
    pts = list(range(16))
    M.set_keyframe(0, pts, root=True)
    M.set_keyframe(1, pts)
    for h in (5, 6, 7):
        M.set_keyframe(h, pts)
    M.update_connections(1)
    M.set_parent(5, 0)
    return [M.keyframe_culling(1, True), M.set_bad_flag(0), M.keyframe_points(0) == pts,
            M.keyframe_points(7)]


# 7 goes (others 0, 1, 5, 6), then 6 (others 0, 1, 5); 5 is left with 0 and 1 only
HAND_ROOT = [[(7, 1, 16, 16), (6, 1, 16, 16), (5, 0, 16, 0), (0, 3, 0, 0)], 0, True, []]


def hand_point_culling(M):
    """ids 0..11, current keyframe id 10, every branch of the chain"""
    R._plain_points(M, HAND_POINTS)
    M.set_keyframe(0, list(range(12)), root=True)
    M.set_keyframe(1, list(range(12)))
    M.set_keyframe(2, [6, 7, 8, 9, 10, 11])
    M.set_keyframe(3, [7, 9, 11])
    M.set_keyframe_features(3, [0, FEAT_STEREO, 0])
    #                 0   1   2   3   4   5   6   7   8   9  10  11
    first = [10, 10, 10, 10, 9, 8, 8, 8, 7, 7, 7, 9]
    visible = [1, 4, 0, 0, 8, 1, 1, 1, 1, 1, 1, 100]
    found = [1, 1, 5, 0, 1, 1, 1, 1, 1, 1, 1, 25]
    M.set_point_stats(0, first, visible, found)
    M.set_point_bad(0)
    recent = [11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    mono = M.point_culling(recent, 10, True)
    return [mono, M.keyframe_points(1), M.keyframe_points(2), M.point_bad(0, 12)]


# 11: 25/100 = 0.25 exactly, diff 1: kept.  0: bad.  1: 1/4 kept (diff 0).  2: 5/0 = inf kept.
# 3: 0/0 = nan kept.  4: 1/8 -> bad.  5: diff 2, Observations 2 -> bad.  6: diff 2, 3 obs: kept
# (2 < 3).  7: diff 2, 4 obs: kept.  8: diff 3, 3 obs: dropped good.  9: diff 3, Observations 5
# (a STEREO feature): dropped good.  10: diff 3, 3 obs: dropped good.
HAND_POINT_CULLING_MONO = [([11, 1, 2, 3, 6, 7], [0, 1, 0, 0, 0, 2, 3, 0, 0, 4, 4, 4]),
                           [0, 1, 2, 3, -1, -1, 6, 7, 8, 9, 10, 11], [6, 7, 8, 9, 10, 11],
                           [True, False, False, False, True, True] + [False] * 6]


def hand_point_culling_stereo(M):
    """the same map with the stereo threshold (Observations <= 3 goes bad)"""
    R._plain_points(M, HAND_POINTS)
    M.set_keyframe(0, list(range(12)), root=True)
    M.set_keyframe(1, list(range(12)))
    M.set_keyframe(2, [6, 7, 8, 9, 10, 11])
    M.set_keyframe(3, [7, 9, 11])
    M.set_keyframe_features(3, [0, FEAT_STEREO, 0])
    M.set_point_stats(0, [8] * 12)
    return [M.point_culling([6, 7, 9, 5], 10, False), M.keyframe_points(2), M.keyframe_points(3)]


# 6: 3 obs -> bad.  7: 4 obs: kept.  9: Observations 5: kept.  5: 2 obs -> bad.
HAND_POINT_CULLING_STEREO = [([7, 9], [3, 0, 0, 3]), [-1, 7, 8, 9, 10, 11], [7, 9, 11]]

def hand_state_defaults(M):
    """defaults, a NULL array leaving its field, the feature byte kept by an overwrite and
    cleared (with mbNotErase) when the slot becomes live again, a dead slot left alone"""
    R._plain_points(M, HAND_POINTS)
    out = [M.point_stats(0, 2)]
    M.set_keyframe(0, [], root=True)
    M.set_keyframe(3, [0, 1, 2])
    M.set_parent(3, 0)
    M.set_keyframe_features(3, [FEAT_STEREO, FEAT_CLOSE, FEAT_STEREO | FEAT_CLOSE])
    M.set_not_erase(3, True)
    M.set_keyframe(3, [0, 1, 5])
    out.append(M.point_stats(0, 3) + M.point_stats(5, 1))
    M.set_point_stats(1, visible=[7, 8])
    M.set_point_stats(2, first_kf=[4], found=[5])
    M.increase_visible([1, -1, 1, 2], 2, mask=[1, 1, 0, 1])
    M.increase_found([2, 2], 3)
    out.append(M.point_stats(1, 2))
    M.erase_keyframe(3)
    M.set_keyframe(3, [4])
    M.set_parent(3, 0)
    M.set_keyframe_features(9, [FEAT_STEREO])
    out += [M.point_stats(4, 1), M.set_bad_flag(9), M.set_not_erase(9, False), M.set_bad_flag(3),
            M.keyframe_points(3), M.keyframe_points(9), M.point_bad(4, 1)]
    return out


HAND_STATE_DEFAULTS = [[(0, 1, 1, 0), (0, 1, 1, 0)],
                       [(0, 1, 1, 2), (0, 1, 1, 1), (0, 1, 1, 0), (0, 1, 1, 2)],
                       [(0, 9, 1, 1), (4, 10, 11, 0)],
                       [(0, 1, 1, 1)], 0, False, 1, [], [], [True]]

HAND_CASES = [
    (hand_state_defaults, HAND_STATE_DEFAULTS),
    (lambda M: hand_cull_threshold(M, 9), HAND_THRESHOLD_9),
    (lambda M: hand_cull_threshold(M, 10), HAND_THRESHOLD_10),
    (lambda M: hand_cull_threshold(M, None), HAND_THRESHOLD_0),
    (hand_cull_octave_gate, HAND_OCTAVE_GATE),
    (hand_cull_observation_count, HAND_OBSERVATION_COUNT),
    (lambda M: hand_cull_close_filter(M, True), HAND_CLOSE_MONO),
    (lambda M: hand_cull_close_filter(M, False), HAND_CLOSE_STEREO),
    (hand_cull_order_first_saves_second, HAND_ORDER_SAVES),
    (hand_cull_order_first_dooms_second, HAND_ORDER_DOOMS),
    (hand_ref_handover, HAND_REF_HANDOVER),
    (hand_not_erase, HAND_NOT_ERASE),
    (hand_tree_repair, HAND_TREE_REPAIR),
    (hand_root, HAND_ROOT),
    (hand_point_culling, HAND_POINT_CULLING_MONO),
    (hand_point_culling_stereo, HAND_POINT_CULLING_STEREO),
]
HAND_NAMES = ["state_defaults", "threshold_9", "threshold_10", "threshold_0", "octave_gate", "observation_count",
              "close_mono", "close_stereo", "order_saves", "order_dooms", "ref_handover",
              "not_erase", "tree_repair", "root", "point_culling_mono", "point_culling_stereo"]


# ---------------------------------------------------------------------------
# random scenes
# ---------------------------------------------------------------------------
NKF, KF_CAP, NPTS, MAX_KF = 48, 160, 768, 64
CULL_SLOTS = (20, 40, 5)
CURRENT_KF_ID = 50


def cull_dataset(seed, stereo):
    rng = np.random.default_rng(5000 + seed)
    d = {"nkf": NKF, "npts": NPTS, "stereo": stereo}
    dirs = rng.normal(size=(NPTS, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    d["pos"] = (dirs * rng.uniform(4.0, 20.0, (NPTS, 1))).astype(F)
    d["bad"] = rng.random(NPTS) < 0.03
    d["desc"] = rng.integers(0, 256, (NPTS, 32), dtype=np.uint8)
    d["centre"] = rng.uniform(-0.55, 0.55, (NKF, 3)).astype(F)
    base = rng.integers(0, 8, NPTS)
    step, width = NPTS // NKF, 8 * (NPTS // NKF)
    rows, octs, feats, seen = [], [], [], {}
    for s in range(NKF):
        prob = 0.5 if s % 4 == 3 else 0.9
        ids = [p for p in range(s * step, min(s * step + width, NPTS)) if rng.random() < prob]
        row = np.full(int(rng.integers(len(ids), KF_CAP + 1)), -1, np.int64)
        row[np.sort(rng.choice(len(row), len(ids), replace=False))] = ids
        jit = rng.choice([-1, 0, 0, 0, 1, 2], len(row))
        rows.append(row.tolist())
        octs.append([int(np.clip(base[p] + j, 0, 7)) if p >= 0 else 0 for p, j in zip(row, jit)])
        fl = np.where(rng.random(len(row)) < 0.8, FEAT_CLOSE, 0)
        if stereo:
            fl = fl | np.where(rng.random(len(row)) < 0.5, FEAT_STEREO, 0)
        feats.append(fl.tolist())
        for p in ids:
            seen.setdefault(p, []).append(s)
    d["rows"], d["octs"], d["feats"] = rows, octs, feats
    d["ref"] = [int(seen[p][rng.integers(len(seen[p]))]) if p in seen else 0 for p in range(NPTS)]
    d["first"] = rng.integers(44, 51, NPTS).tolist()
    d["visible"] = rng.integers(0, 20, NPTS).tolist()
    d["found"] = rng.integers(0, 12, NPTS).tolist()
    d["recent"] = rng.permutation(NPTS)[:300].tolist()
    d["update"] = [3, 19, 21, 30, 41]
    # children far from their parent (ChangeParent after a loop closure): when the parent goes
    # they have no link to a candidate and fall back.  Parents are lower slots: still a tree.
    near = [e for e in range(1, 27) if e < 10 or e > 13]
    d["adopt"] = [(int(c), int(rng.choice(near))) for c in rng.choice(np.arange(37, NKF), 10,
                                                                      replace=False)]
    return d


def build_cull_map(M, d):
    M.set_points(0, d["pos"], d["bad"], d["desc"], d["ref"])
    M.set_point_stats(0, d["first"], d["visible"], d["found"])
    for s in range(d["nkf"]):
        M.set_keyframe(s, d["rows"][s], d["octs"][s], d["centre"][s], root=(s == 0))
        M.set_keyframe_features(s, d["feats"][s])
        M.update_connections(s)
    for s in range(d["nkf"]):
        M.update_connections(s)
    for c, e in d["adopt"]:
        M.set_parent(c, e)


def run_cull_scene(M, d, not_erase=None, check=None):
    """three KeyFrameCulling calls, a MapPointCulling, then UpdateConnections of a few slots and
    UpdateNormalAndDepth; check(stage) is called after each step.  Returns every record."""
    build_cull_map(M, d)
    if not_erase is not None:
        M.set_not_erase(not_erase, True)
    out = []
    for i, s in enumerate(CULL_SLOTS):
        out.append(M.keyframe_culling(s, not d["stereo"]))
        if check:
            check("kfc%d" % i)
    out.append(M.point_culling(d["recent"], CURRENT_KF_ID, not d["stereo"]))
    if check:
        check("mpc")
    for s in d["update"]:
        M.update_connections(s)
    if check:
        check("update")
    return out


# ---------------------------------------------------------------------------
# the wide map: a culling slot that lists more than 256 keyframes, rows of more than 256
# features, points with more than 64 observers
# ---------------------------------------------------------------------------
WIDE_K, WIDE_CAP, WIDE_PTS, WIDE_N, WIDE_HUB = 1024, 320, 4096, 300, 700


def wide_slots():
    return [3 * j + 1 for j in range(WIDE_N) if 3 * j + 1 != WIDE_HUB]


def build_wide_cull(M):
    """The hub shares 15 + j % 9 of 64 popular points with keyframe j; every third keyframe holds
    only popular points at coarse levels (redundant), the others mostly own points (kept); a
    few fat keyframes have rows of 300 features."""
    rng = np.random.default_rng(78)
    M.set_points(0, [(0.01 * i, 0.3, 6.0) for i in range(WIDE_PTS)], [False] * WIDE_PTS,
                 rng.integers(0, 256, (WIDE_PTS, 32), dtype=np.uint8), [WIDE_HUB] * WIDE_PTS)
    popular = list(range(64))
    M.set_keyframe(WIDE_HUB, popular + list(range(4000, 4030)), [0] * 94)
    M.set_keyframe(1, [], root=True)
    nxt = 100
    for j, s in enumerate(wide_slots()):
        if s == 1:
            continue
        pop = popular[:15 + j % 9]
        if j % 3 == 0:
            row, octs = pop, [5] * len(pop)
        elif j % 50 == 7:
            own = list(range(nxt, nxt + 300 - len(pop)))
            nxt += len(own)
            row, octs = pop + own, [1] * 300
        else:
            own = list(range(nxt, nxt + 6))
            nxt += 6
            row, octs = pop + own, [j % 3] * len(pop) + [0] * 6
        M.set_keyframe(s, row, octs)
        M.set_parent(s, WIDE_HUB if j % 2 else 1)
    assert nxt <= 4000
    M.update_connections(WIDE_HUB)
    M.set_parent(WIDE_HUB, 1)
