"""KeyFrameDatabase -- ORB-SLAM2's place recognition database (include/KeyFrameDatabase.h,
src/KeyFrameDatabase.cc): add / erase / clear, DetectRelocalizationCandidates(Frame*)
(:291-419, Tracking::Relocalization) and DetectLoopCandidates(KeyFrame*, minScore) (:106-274,
LoopClosing::DetectLoop), device-resident behind liborbg's orbg_kfdb_* entry points.

A KeyFrame is a slot in [0, max_keyframes): the caller's handle.  What the reference reads
from the KeyFrame objects is passed in: the BowVector at add, each slot's
GetBestCovisibilityKeyFrames(10) (`neighbours`, [max_keyframes][10] slots, -1 = unused) and,
for loop detection, the query's GetConnectedKeyFrames() (`connected`).  Candidates come out
as slots in the reference's order.

    db = KeyFrameDatabase(voc, max_keyframes=2048)
    db.add(slot, bow)                                         # KeyFrameDatabase::add(pKF)
    cands = db.DetectRelocalizationCandidates(bow, neighbours)
    cands = db.DetectLoopCandidates(bow, connected, min_score, neighbours)

mRelocScore, which the reference leaves uninitialised at KeyFrame construction, is 0 from add
on.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .orbmatcher import _ctx

NEIGHBOURS = 10   # GetBestCovisibilityKeyFrames(10)


def _bow_arrays(bow):
    if isinstance(bow, dict):
        k = sorted(bow)
        return (np.array(k, np.int32), np.array([bow[i] for i in k], np.float64))
    w, x = bow
    w = np.ascontiguousarray(w, np.int32)
    x = np.ascontiguousarray(x, np.float64)
    if len(w) != len(x):
        raise ValueError("word and weight arrays differ in length")
    return w, x


class KeyFrameDatabase:
    def __init__(self, voc, max_keyframes, cap=2048, device=None):
        """`cap`: the largest BowVector (entries) a slot can hold, <= 8192."""
        self.device = voc.device if device is None else device
        self._voc = voc     # the database reads the vocabulary's size only; keep it alive
        self._h = None
        h = C.c_void_p()
        L.check(L.lib().orbg_kfdb_create(_ctx(self.device).handle, voc.handle, int(max_keyframes),
                                         int(cap), C.byref(h)), "orbg_kfdb_create")
        self._h = h
        self.max_keyframes, self.cap = int(max_keyframes), int(cap)

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                L.lib().orbg_kfdb_destroy(self._h)
            self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _c(self, ctx=None):
        return (ctx if ctx is not None else _ctx(self.device)).handle

    def info(self):
        """(live slots, max_keyframes, cap, largest max_keyframes supported)"""
        v = [C.c_int32() for _ in range(4)]
        L.check(L.lib().orbg_kfdb_info(self._h, *[C.byref(x) for x in v]), "orbg_kfdb_info")
        return tuple(x.value for x in v)

    def __len__(self):
        return self.info()[0]

    # ---- maintenance ----
    def add(self, slot, bow):
        """KeyFrameDatabase::add(pKF): `bow` a BowVector (dict) or (words, weights) arrays."""
        w, x = _bow_arrays(bow)
        L.check(L.lib().orbg_kfdb_add(self._c(), self._h, int(slot), L.ptr(w), L.ptr(x), len(w)),
                "orbg_kfdb_add")

    def add_batch_device(self, d_slots, vectors, vcap, d_index, n, ctx=None):
        """orbg_kfdb_add_batch_device: `vectors` maps words / weights / nbow (or
        transform_batch_device's bow_words / bow_weights / nbow) to device pointers (ints)."""
        v = self._vectors(vectors)
        L.check(L.lib().orbg_kfdb_add_batch_device(self._c(ctx), self._h, d_slots, C.byref(v),
                                                   int(vcap), d_index, int(n)),
                "orbg_kfdb_add_batch_device")

    def erase(self, slot):
        L.check(L.lib().orbg_kfdb_erase(self._c(), self._h, int(slot)), "orbg_kfdb_erase")

    def clear(self):
        L.check(L.lib().orbg_kfdb_clear(self._c(), self._h), "orbg_kfdb_clear")

    def rebuild(self, ctx=None):
        """Rebuild the inverted file now (the first query after a change does it otherwise)."""
        L.check(L.lib().orbg_kfdb_rebuild(self._c(ctx), self._h), "orbg_kfdb_rebuild")

    def reloc_scores(self):
        """mRelocScore of every slot (float32 [max_keyframes]; dead slots unspecified)."""
        out = np.zeros(self.max_keyframes, np.float32)
        L.check(L.lib().orbg_kfdb_reloc_scores(self._c(), self._h, L.ptr(out)),
                "orbg_kfdb_reloc_scores")
        return out

    # ---- queries ----
    _vectors = staticmethod(L.bow_vectors)

    def _neigh(self, neighbours):
        if neighbours is None:
            return np.full((self.max_keyframes, NEIGHBOURS), -1, np.int32)
        n = np.ascontiguousarray(neighbours, np.int32)
        if n.shape != (self.max_keyframes, NEIGHBOURS):
            raise ValueError("neighbours must be [max_keyframes][%d]" % NEIGHBOURS)
        return n

    def detect_reloc(self, bow, neighbours=None, cand_cap=None):
        """(candidates, ncand, maxCommonWords, nscores); ncand counts past cand_cap too."""
        w, x = _bow_arrays(bow)
        ng = self._neigh(neighbours)
        cap = self.max_keyframes if cand_cap is None else int(cand_cap)
        cand = np.full(max(cap, 1), -1, np.int32)
        nc, mc, ns = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(L.lib().orbg_kfdb_detect_reloc(self._c(), self._h, L.ptr(w), L.ptr(x), len(w),
                                               L.ptr(ng), L.ptr(cand), cap, C.byref(nc),
                                               C.byref(mc), C.byref(ns)),
                "orbg_kfdb_detect_reloc")
        return cand[:min(nc.value, cap)].tolist(), nc.value, mc.value, ns.value

    def detect_loop(self, bow, connected, min_score, neighbours=None, cand_cap=None):
        w, x = _bow_arrays(bow)
        ng = self._neigh(neighbours)
        cn = np.ascontiguousarray(sorted(connected) if isinstance(connected, (set, frozenset))
                                  else connected, np.int32).reshape(-1)
        cap = self.max_keyframes if cand_cap is None else int(cand_cap)
        cand = np.full(max(cap, 1), -1, np.int32)
        nc, mc, ns = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(L.lib().orbg_kfdb_detect_loop(self._c(), self._h, L.ptr(w), L.ptr(x), len(w),
                                              L.ptr(cn), len(cn), float(np.float32(min_score)),
                                              L.ptr(ng), L.ptr(cand), cap, C.byref(nc),
                                              C.byref(mc), C.byref(ns)),
                "orbg_kfdb_detect_loop")
        return cand[:min(nc.value, cap)].tolist(), nc.value, mc.value, ns.value

    def DetectRelocalizationCandidates(self, bow, neighbours=None):
        """vector<KeyFrame*> DetectRelocalizationCandidates(Frame *F) as a list of slots."""
        return self.detect_reloc(bow, neighbours)[0]

    def DetectLoopCandidates(self, bow, connected, min_score, neighbours=None):
        """vector<KeyFrame*> DetectLoopCandidates(KeyFrame *pKF, float minScore)."""
        return self.detect_loop(bow, connected, min_score, neighbours)[0]

    def detect_reloc_batch_device(self, queries, qcap, d_qindex, nq, d_neigh, d_cand, cand_cap,
                                  d_ncand, d_max_common=None, d_nscored=None, ctx=None):
        """orbg_kfdb_detect_reloc_batch_device; device pointers as ints."""
        v = self._vectors(queries)
        L.check(L.lib().orbg_kfdb_detect_reloc_batch_device(
            self._c(ctx), self._h, C.byref(v), int(qcap), d_qindex, int(nq), d_neigh, d_cand,
            int(cand_cap), d_ncand, d_max_common, d_nscored),
            "orbg_kfdb_detect_reloc_batch_device")

    def detect_loop_batch_device(self, queries, qcap, d_qindex, nq, d_conn, conn_cap, d_nconn,
                                 d_min_score, d_neigh, d_cand, cand_cap, d_ncand,
                                 d_max_common=None, d_nscored=None, ctx=None):
        """orbg_kfdb_detect_loop_batch_device; device pointers as ints."""
        v = self._vectors(queries)
        L.check(L.lib().orbg_kfdb_detect_loop_batch_device(
            self._c(ctx), self._h, C.byref(v), int(qcap), d_qindex, int(nq), d_conn,
            int(conn_cap), d_nconn, d_min_score, d_neigh, d_cand, int(cand_cap), d_ncand,
            d_max_common, d_nscored),
            "orbg_kfdb_detect_loop_batch_device")
