"""Map -- ORB-SLAM2's covisibility graph and local map over one device-resident table, "which
keyframe slot observes which map point" (liborbg's orbg_map_* entry points):
KeyFrame::UpdateConnections (src/KeyFrame.cc:375-515), Tracking::UpdateLocalKeyFrames /
UpdateLocalPoints (src/Tracking.cc:1731-1925), MapPoint::UpdateNormalAndDepth
(src/MapPoint.cc:457-518), KeyFrame::SetBadFlag (src/KeyFrame.cc:622-720) and
LocalMapping::KeyFrameCulling / MapPointCulling (src/LocalMapping.cc:227-270, 804-877), and of
LoopClosing::CorrectLoop (src/LoopClosing.cc:744-843, 882-911, src/Optimizer.cc:1040-1323) the
Sim3 propagation, LoopConnections, the essential-graph walk and the application of the optimised
poses, over keyframe poses, mnId, loop edges and the mnCorrected fields the Map holds.

A KeyFrame is a slot in [0, max_keyframes), as in KeyFrameDatabase; a MapPoint is an id in
[0, max_points).  Wherever the reference orders by KeyFrame pointer, the order here is the
ascending slot (include/orbg.h).

    m = Map(max_keyframes=2048, kf_cap=2000, max_points=200000)
    m.SetPoints(0, records, descriptors, ref_kf)              # MAPPOINT_DTYPE records
    m.AddKeyFrame(slot, point_ids, octaves, camera_centre)    # after ProcessNewKeyFrame
    m.UpdateConnections(slot)
    kfs, ref = m.UpdateLocalKeyFrames(frame_points)           # frame_points nulled in place
    ids, mps, desc = m.UpdateLocalPoints(kfs, frame_points)
    db.DetectRelocalizationCandidates(bow, m.neighbours())    # the device table, unchanged
    recent, status = m.MapPointCulling(recent, current_kf_id, monocular)
    for r in m.KeyFrameCulling(slot, monocular):              # CULL_RECORD_DTYPE records
        if r["status"] == 1: db.erase(r["slot"])
    m.SetPoses(slots, Tcw, mnId)                              # KeyFrame::SetPose, once per pose
    members, corrected, noncorrected = m.Propagate(cur, Scw)  # CorrectLoop, LoopClosing.cc:744-843
    m.LoopFusion(cur, matched); m.SearchAndFuse(members, corrected, loop_points)
    pairs = m.LoopConnections(members)
    vs, fixed, Scw_v, Snc_v, edges, _ = m.EssentialGraph(cur, loop, corrected, noncorrected, members, pairs)
    Siw, Tiw, _ = OptimizeEssentialGraph(Scw_v, Snc_v, edges, fixed, bFixScale)
    m.ApplyCorrection(cur, vs, Scw_v, Siw, Tiw); m.AddLoopEdge(loop, cur)
    report, counts = m.CorrectLoop(cur, loop, Scw, matched, loop_points, bFixScale)  # all of it
    report = m.LocalBundleAdjustment(slot, stop_flag)         # Optimizer.cc:633-979 on the table
    recent, _ = m.ProcessNewKeyFrame(slot, ids, octs, feats, Tcw, mnId, in_keyframe, recent)
    recent, report = m.CreateNewMapPoints(slot, mnId, monocular, first_id, recent)
    w = m.LbaWindow(slot); m.LbaApply(w, poses, points, erase)  # its two ends, one at a time
    report = m.GlobalBundleAdjustment(20)                     # CreateInitialMapMonocular's call
    report = m.RunGlobalBundleAdjustment(loop_kf, stop_flag=flag)   # LoopClosing.cc:1024-1128
    w = m.GbaWindow(robust); m.GbaStore(w, poses, points, loop_kf); m.GbaUpdate(loop_kf)
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .orbmatcher import _ctx

NEIGHBOURS = 10
SIN_MAX_TARGETS = 120     # SearchInNeighbors: 20 first-level + 20 * 5 second-level entries
KF_ROOT, KF_BAD = 1, 2
MAX_LOOP_EDGES = 16        # mspLoopEdges entries per slot (ORBG_ERANGE past it)
MAX_LOOP_SET = 256         # members of mvpCurrentConnectedKFs a Propagate / LoopConnections call takes
LOOP_NO_POSE, LOOP_SET_RANGE, LOOP_DEAD = 1, 2, 4   # propagate_device's status bits
FEAT_STEREO, FEAT_CLOSE = L.MAP_FEAT_STEREO, L.MAP_FEAT_CLOSE


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


class Map:
    def __init__(self, max_keyframes, kf_cap, max_points, device=0):
        self.device = device
        self._h = None
        h = C.c_void_p()
        L.check(L.lib().orbg_map_create(_ctx(device).handle, int(max_keyframes), int(kf_cap),
                                        int(max_points), C.byref(h)), "orbg_map_create")
        self._h = h
        self.max_keyframes, self.kf_cap, self.max_points = (int(max_keyframes), int(kf_cap),
                                                            int(max_points))

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                L.lib().orbg_map_destroy(self._h)
            self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _c(self, ctx=None):
        return (ctx if ctx is not None else _ctx(self.device)).handle

    def info(self):
        """(live slots, max_keyframes, kf_cap, max_points)"""
        v = [C.c_int32() for _ in range(4)]
        L.check(L.lib().orbg_map_info(self._h, *[C.byref(x) for x in v]), "orbg_map_info")
        return tuple(x.value for x in v)

    def __len__(self):
        return self.info()[0]

    # ---- mutations ----
    def AddKeyFrame(self, slot, point_ids, octaves, centre, root=False, bad=False):
        """Adds or overwrites a slot: mvpMapPoints as ids (-1 = NULL), mvKeysUn[i].octave,
        GetCameraCenter(); root = (mnId == 0)."""
        p = _i32(point_ids)
        o = np.ascontiguousarray(octaves, np.uint8).reshape(-1)
        if len(p) != len(o):
            raise ValueError("point ids and octaves differ in length")
        c = np.ascontiguousarray(centre, np.float32).reshape(3)
        L.check(L.lib().orbg_map_set_keyframe(self._c(), self._h, int(slot), L.ptr(p), L.ptr(o),
                                              len(p), L.ptr(c),
                                              (KF_ROOT if root else 0) | (KF_BAD if bad else 0)),
                "orbg_map_set_keyframe")

    set_keyframe = AddKeyFrame

    def set_keyframes_device(self, d_slots, n, d_point_ids, d_octaves, row_cap, d_counts,
                             d_centres, d_flags, ctx=None):
        """orbg_map_set_keyframes_device; device pointers as ints."""
        L.check(L.lib().orbg_map_set_keyframes_device(self._c(ctx), self._h, d_slots, int(n),
                                                      d_point_ids, d_octaves, int(row_cap),
                                                      d_counts, d_centres, d_flags),
                "orbg_map_set_keyframes_device")

    def SetPoints(self, first, records, descriptors, ref_kf):
        """MAPPOINT_DTYPE records (flags: MP_VALID = !isBad()), mDescriptor [n][32], mpRefKF
        slots of the points first .. first + n - 1."""
        r = np.ascontiguousarray(records, L.MAPPOINT_DTYPE).reshape(-1)
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        k = _i32(ref_kf)
        if not (len(r) == len(d) == len(k)):
            raise ValueError("records, descriptors and reference keyframes differ in length")
        L.check(L.lib().orbg_map_set_points(self._c(), self._h, int(first), len(r), L.ptr(r),
                                            L.ptr(d), L.ptr(k)), "orbg_map_set_points")

    set_points = SetPoints

    def set_points_device(self, d_ids, first, n, d_mps, d_desc, d_ref_kf, ctx=None):
        L.check(L.lib().orbg_map_set_points_device(self._c(ctx), self._h, d_ids, int(first), int(n),
                                                   d_mps, d_desc, d_ref_kf),
                "orbg_map_set_points_device")

    def points(self, first=0, n=None):
        """the stored MAPPOINT_DTYPE records"""
        n = self.max_points - first if n is None else int(n)
        out = np.zeros(n, L.MAPPOINT_DTYPE)
        L.check(L.lib().orbg_map_get_points(self._c(), self._h, int(first), n, L.ptr(out)),
                "orbg_map_get_points")
        return out

    def SetPointBad(self, point_id):
        L.check(L.lib().orbg_map_set_point_bad(self._c(), self._h, int(point_id)),
                "orbg_map_set_point_bad")

    def ChangeParent(self, slot, parent):
        L.check(L.lib().orbg_map_set_parent(self._c(), self._h, int(slot),
                                            -1 if parent is None else int(parent)),
                "orbg_map_set_parent")

    def EraseKeyFrame(self, slot):
        """The table side of KeyFrame::SetBadFlag; the spanning-tree repair stays with the
        caller (ChangeParent)."""
        L.check(L.lib().orbg_map_erase_keyframe(self._c(), self._h, int(slot)),
                "orbg_map_erase_keyframe")

    def clear(self):
        L.check(L.lib().orbg_map_clear(self._c(), self._h), "orbg_map_clear")

    def rebuild(self, ctx=None):
        L.check(L.lib().orbg_map_rebuild(self._c(ctx), self._h), "orbg_map_rebuild")

    # ---- readers ----
    def neighbours(self):
        """Device pointer (int) of neigh[max_keyframes][10]: KeyFrameDatabase's d_neigh."""
        p = C.c_void_p()
        L.check(L.lib().orbg_map_neighbours(self._h, C.byref(p)), "orbg_map_neighbours")
        return p.value

    def neighbours_host(self):
        """a host copy of neigh[max_keyframes][10] (-1 = unused)"""
        out = np.zeros((self.max_keyframes, NEIGHBOURS), np.int32)
        L.check(L.lib().orbg_map_get_neighbours(self._c(), self._h, L.ptr(out)),
                "orbg_map_get_neighbours")
        return out

    def connected_device(self,d_slots, n, d_conn, conn_cap, d_nconn, ctx=None):
        L.check(L.lib().orbg_map_connected_device(self._c(ctx), self._h, d_slots, int(n), d_conn,
                                                  int(conn_cap), d_nconn),
                "orbg_map_connected_device")

    def connections(self, slot):
        """(ordered slots, ordered weights, parent or None): mvpOrderedConnectedKeyFrames,
        mvOrderedWeights, mpParent."""
        cap = self.max_keyframes
        s, w = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n, par = C.c_int32(), C.c_int32()
        L.check(L.lib().orbg_map_get_connections(self._c(), self._h, int(slot), L.ptr(s), L.ptr(w),
                                                 cap, C.byref(n), C.byref(par)),
                "orbg_map_get_connections")
        return s[:n.value].tolist(), w[:n.value].tolist(), None if par.value < 0 else par.value

    def GetVectorCovisibleKeyFrames(self, slot):
        return self.connections(slot)[0]

    def GetBestCovisibilityKeyFrames(self, slot, N=NEIGHBOURS):
        return self.connections(slot)[0][:N]

    def GetCovisiblesByWeight(self, slot, w):
        s, ws, _ = self.connections(slot)
        return [k for k, x in zip(s, ws) if x >= w]

    def GetParent(self, slot):
        return self.connections(slot)[2]

    def weights(self, slot):
        """row `slot` of mConnectedKeyFrameWeights as uint16 [max_keyframes] (0 = none)"""
        out = np.zeros(self.max_keyframes, np.uint16)
        L.check(L.lib().orbg_map_get_weights(self._c(), self._h, int(slot), L.ptr(out)),
                "orbg_map_get_weights")
        return out

    def GetWeight(self, slot, other):
        return int(self.weights(slot)[other])

    def GetConnectedKeyFrames(self, slot):
        return np.nonzero(self.weights(slot))[0].tolist()

    # ---- the reference functions ----
    def UpdateConnections(self, slot):
        L.check(L.lib().orbg_map_update_connections(self._c(), self._h, int(slot)),
                "orbg_map_update_connections")

    def update_connections_batch_device(self, d_slots, n, ctx=None):
        L.check(L.lib().orbg_map_update_connections_batch_device(self._c(ctx), self._h, d_slots,
                                                                 int(n)),
                "orbg_map_update_connections_batch_device")

    def UpdateLocalKeyFrames(self, frame_points, lkf_cap=None):
        """(mvpLocalKeyFrames as slots or None when the vote counter is empty, mpReferenceKF or
        None); frame_points (int32 array) has its bad points set to -1 in place."""
        if not (isinstance(frame_points, np.ndarray) and frame_points.dtype == np.int32
                and frame_points.flags.c_contiguous):
            raise ValueError("frame_points must be a contiguous int32 array (updated in place)")
        cap = self.max_keyframes if lkf_cap is None else int(lkf_cap)
        out = np.full(max(cap, 1), -1, np.int32)
        n, ref = C.c_int32(), C.c_int32()
        L.check(L.lib().orbg_map_local_keyframes(self._c(), self._h, L.ptr(frame_points),
                                                 frame_points.size, L.ptr(out), cap, C.byref(n),
                                                 C.byref(ref)), "orbg_map_local_keyframes")
        if n.value < 0:
            return None, None
        return out[:n.value].tolist(), None if ref.value < 0 else ref.value

    def UpdateLocalPoints(self, local_kfs, frame_points, lp_cap=None):
        """(ids, MAPPOINT_DTYPE records, descriptors [n][32]) of mvpLocalMapPoints in the
        reference's order; flags as Tracking::SearchLocalPoints reads them."""
        lk, fp = _i32(local_kfs), _i32(frame_points)
        cap = len(lk) * self.kf_cap if lp_cap is None else int(lp_cap)
        ids = np.full(max(cap, 1), -1, np.int32)
        mps = np.zeros(max(cap, 1), L.MAPPOINT_DTYPE)
        desc = np.zeros((max(cap, 1), 32), np.uint8)
        n = C.c_int32()
        L.check(L.lib().orbg_map_local_points(self._c(), self._h, L.ptr(lk), len(lk), L.ptr(fp),
                                              len(fp), L.ptr(ids), L.ptr(mps), L.ptr(desc), cap,
                                              C.byref(n)), "orbg_map_local_points")
        return ids[:n.value], mps[:n.value], desc[:n.value]

    def local_keyframes_batch_device(self, d_frame_points, frame_cap, d_counts, nframes,
                                     d_local_kfs, lkf_cap, d_nlocal, d_ref_kf, ctx=None):
        L.check(L.lib().orbg_map_local_keyframes_batch_device(
            self._c(ctx), self._h, d_frame_points, int(frame_cap), d_counts, int(nframes),
            d_local_kfs, int(lkf_cap), d_nlocal, d_ref_kf),
            "orbg_map_local_keyframes_batch_device")

    def local_points_batch_device(self, d_local_kfs, lkf_cap, d_nlocal, d_frame_points, frame_cap,
                                  d_counts, nframes, d_local_ids, d_mps, d_qdesc, lp_cap,
                                  d_nlocal_points, ctx=None):
        L.check(L.lib().orbg_map_local_points_batch_device(
            self._c(ctx), self._h, d_local_kfs, int(lkf_cap), d_nlocal, d_frame_points,
            int(frame_cap), d_counts, int(nframes), d_local_ids, d_mps, d_qdesc, int(lp_cap),
            d_nlocal_points), "orbg_map_local_points_batch_device")

    def update_normal_and_depth_batch_device(self, d_point_ids, n, ctx=None):
        L.check(L.lib().orbg_map_update_normal_and_depth_batch_device(self._c(ctx), self._h,
                                                                      d_point_ids, int(n)),
                "orbg_map_update_normal_and_depth_batch_device")

    def UpdateNormalAndDepth(self, point_ids=None):
        """MapPoint::UpdateNormalAndDepth of the listed points (None: all) into the stored
        records (read them with points())."""
        ctx = _ctx(self.device)
        if point_ids is None:
            self.update_normal_and_depth_batch_device(None, self.max_points)
        else:
            import torch
            ids = torch.from_numpy(_i32(point_ids)).to("cuda:%d" % self.device)
            torch.cuda.synchronize()
            self.update_normal_and_depth_batch_device(ids.data_ptr(), ids.numel())
        ctx.sync()

    # ---- KeyFrame::SetBadFlag, LocalMapping::KeyFrameCulling / MapPointCulling ----
    def SetKeyFrameFeatures(self, slot, flags):
        """per feature: FEAT_STEREO (mvuRight[i] >= 0) | FEAT_CLOSE (depth within mThDepth)"""
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        L.check(L.lib().orbg_map_set_keyframe_features(self._c(), self._h, int(slot), L.ptr(f),
                                                       len(f)), "orbg_map_set_keyframe_features")

    def set_keyframe_features_device(self, d_slots, n, d_flags, row_cap, d_counts, ctx=None):
        L.check(L.lib().orbg_map_set_keyframe_features_device(self._c(ctx), self._h, d_slots,
                                                              int(n), d_flags, int(row_cap),
                                                              d_counts),
                "orbg_map_set_keyframe_features_device")

    def _not_erase(self, slot, on):
        erased = C.c_int32()
        L.check(L.lib().orbg_map_set_not_erase(self._c(), self._h, int(slot), on,
                                               C.byref(erased)), "orbg_map_set_not_erase")
        return bool(erased.value)

    def SetNotErase(self, slot):
        self._not_erase(slot, 1)

    def SetErase(self, slot):
        """once mspLoopEdges is empty; True if the pending SetBadFlag ran"""
        return self._not_erase(slot, 0)

    def SetBadFlag(self, slot):
        """KeyFrame::SetBadFlag in full; 0 nothing (root / dead), 1 erased, 2 marked"""
        st = C.c_int32()
        L.check(L.lib().orbg_map_set_bad_flag(self._c(), self._h, int(slot), C.byref(st)),
                "orbg_map_set_bad_flag")
        return st.value

    def KeyFrameCulling(self, slot, monocular):
        """CULL_RECORD_DTYPE records, one per entry of slot's ordered list"""
        rec = np.zeros(self.max_keyframes, L.CULL_RECORD_DTYPE)
        n = C.c_int32()
        L.check(L.lib().orbg_map_keyframe_culling(self._c(), self._h, int(slot), int(bool(monocular)),
                                                  L.ptr(rec), len(rec), C.byref(n)),
                "orbg_map_keyframe_culling")
        return rec[:n.value]

    def keyframe_culling_device(self, slot, monocular, d_records, rec_cap, d_nrec, ctx=None):
        L.check(L.lib().orbg_map_keyframe_culling_device(self._c(ctx), self._h, int(slot),
                                                         int(bool(monocular)), d_records,
                                                         int(rec_cap), d_nrec),
                "orbg_map_keyframe_culling_device")

    def MapPointCulling(self, recent, current_kf_id, monocular):
        """(mlpRecentAddedMapPoints after the call, status per input position)"""
        r = _i32(recent).copy()
        st = np.zeros(len(r), np.int32)
        n = C.c_int32()
        L.check(L.lib().orbg_map_point_culling(self._c(), self._h, L.ptr(r), len(r),
                                               int(current_kf_id), int(bool(monocular)),
                                               C.byref(n), L.ptr(st)), "orbg_map_point_culling")
        return r[:n.value], st

    def point_culling_device(self, d_recent, n, current_kf_id, monocular, d_nout, d_status,
                             ctx=None):
        L.check(L.lib().orbg_map_point_culling_device(self._c(ctx), self._h, d_recent, int(n),
                                                      int(current_kf_id), int(bool(monocular)),
                                                      d_nout, d_status),
                "orbg_map_point_culling_device")

    def SetPointStats(self, first, first_kf_id=None, visible=None, found=None):
        a = [None if x is None else _i32(x) for x in (first_kf_id, visible, found)]
        n = {len(x) for x in a if x is not None}
        if len(n) != 1:
            raise ValueError("the given arrays differ in length (or none is given)")
        L.check(L.lib().orbg_map_set_point_stats(self._c(), self._h, int(first), n.pop(),
                                                 *[None if x is None else L.ptr(x) for x in a]),
                "orbg_map_set_point_stats")

    def set_point_stats_device(self, d_ids, first, n, d_first_kf_id, d_visible, d_found, ctx=None):
        L.check(L.lib().orbg_map_set_point_stats_device(self._c(ctx), self._h, d_ids, int(first),
                                                        int(n), d_first_kf_id, d_visible, d_found),
                "orbg_map_set_point_stats_device")

    def point_stats(self, first=0, n=None):
        """(mnFirstKFid, mnVisible, mnFound, Observations()) as int32 arrays"""
        n = self.max_points - first if n is None else int(n)
        out = [np.zeros(n, np.int32) for _ in range(4)]
        L.check(L.lib().orbg_map_get_point_stats(self._c(), self._h, int(first), n,
                                                 *[L.ptr(x) for x in out]),
                "orbg_map_get_point_stats")
        return tuple(out)

    def increase_visible_device(self, d_ids, d_proj, n, amount=1, ctx=None):
        L.check(L.lib().orbg_map_increase_visible_device(self._c(ctx), self._h, d_ids, d_proj,
                                                         int(n), int(amount)),
                "orbg_map_increase_visible_device")

    def increase_found_device(self, d_ids, n, amount=1, ctx=None):
        L.check(L.lib().orbg_map_increase_found_device(self._c(ctx), self._h, d_ids, int(n),
                                                       int(amount)),
                "orbg_map_increase_found_device")

    def _increase(self, fn, point_ids, amount):
        import torch
        ids = torch.from_numpy(_i32(point_ids)).to("cuda:%d" % self.device)
        torch.cuda.synchronize()
        fn(ids.data_ptr(), ids.numel(), amount)
        _ctx(self.device).sync()

    def IncreaseVisible(self, point_ids, amount=1):
        self._increase(lambda p, n, a: self.increase_visible_device(p, None, n, a), point_ids,
                       amount)

    def IncreaseFound(self, point_ids, amount=1):
        self._increase(self.increase_found_device, point_ids, amount)

    def keyframe_points(self, slot):
        """mvpMapPoints of a slot as ids (-1 = NULL); empty for a dead slot"""
        out = np.full(self.kf_cap, -1, np.int32)
        n = C.c_int32()
        L.check(L.lib().orbg_map_get_keyframe_points(self._c(), self._h, int(slot), L.ptr(out),
                                                     len(out), C.byref(n)),
                "orbg_map_get_keyframe_points")
        return out[:n.value]

    # ---- MapPoint::Replace, ORBmatcher::Fuse, LocalMapping::SearchInNeighbors ----
    def AttachKeyFrames(self, d_desc, d_kps, d_uright, d_counts, cap, d_cams, d_fv_nodes=None,
                        d_fv_off=None, d_fv_feats=None, d_nfv=None):
        """The keyframes' data the search and ComputeDistinctiveDescriptors read, as device
        pointers (ints) indexed by slot: mDescriptors [K][cap][32], mvKeysUn [K][cap]
        (KEYPOINT records), mvuRight [K][cap] (None: monocular), N [K], FRUSTUM_DTYPE cameras
        [K]; d_fv_*: mFeatVec in orbg_bow_transform_batch_device's layout, read by
        CreateNewMapPoints only.  Not owned: the arrays must outlive the attachment.  d_desc
        None detaches."""
        if d_desc is None:
            L.check(L.lib().orbg_map_attach_keyframes(self._c(), self._h, None, 0, None),
                    "orbg_map_attach_keyframes")
            return
        k = L.KeyFrames(d_desc, d_kps, d_uright, None, d_counts, d_fv_nodes, d_fv_off, d_fv_feats,
                        d_nfv)
        L.check(L.lib().orbg_map_attach_keyframes(self._c(), self._h, C.byref(k), int(cap), d_cams),
                "orbg_map_attach_keyframes")

    def AddObservations(self, slots, idx, point_ids):
        """AddObservation + AddMapPoint, entries in order; the status per entry (0 = added)"""
        s, i, p = _i32(slots), _i32(idx), _i32(point_ids)
        if not (len(s) == len(i) == len(p)):
            raise ValueError("slots, feature indices and point ids differ in length")
        st = np.zeros(len(s), np.int32)
        L.check(L.lib().orbg_map_add_observations(self._c(), self._h, L.ptr(s), L.ptr(i), L.ptr(p),
                                                  len(s), L.ptr(st)), "orbg_map_add_observations")
        return st

    def add_observations_device(self, d_slots, d_idx, d_point_ids, n, d_status, ctx=None):
        L.check(L.lib().orbg_map_add_observations_device(self._c(ctx), self._h, d_slots, d_idx,
                                                         d_point_ids, int(n), d_status),
                "orbg_map_add_observations_device")

    def Replace(self, old_ids, new_ids):
        """old->Replace(new) pair by pair, then the survivors' descriptors; the status per pair
        (0 replaced, 1 same point, 2 new bad, 3 old out of range, 4 old already bad)"""
        o, w = _i32(old_ids), _i32(new_ids)
        if len(o) != len(w):
            raise ValueError("old and new ids differ in length")
        st = np.zeros(len(o), np.int32)
        L.check(L.lib().orbg_map_replace(self._c(), self._h, L.ptr(o), L.ptr(w), len(o), L.ptr(st)),
                "orbg_map_replace")
        return st

    def replace_device(self, d_old, d_new, n, d_status, ctx=None):
        L.check(L.lib().orbg_map_replace_device(self._c(ctx), self._h, d_old, d_new, int(n),
                                                d_status), "orbg_map_replace_device")

    def distinctive_descriptors_device(self, d_point_ids, n, ctx=None):
        L.check(L.lib().orbg_map_distinctive_descriptors_device(self._c(ctx), self._h, d_point_ids,
                                                                int(n)),
                "orbg_map_distinctive_descriptors_device")

    def ComputeDistinctiveDescriptors(self, point_ids):
        """MapPoint::ComputeDistinctiveDescriptors of the listed points into the map"""
        import torch
        ids = torch.from_numpy(_i32(point_ids)).to("cuda:%d" % self.device)
        torch.cuda.synchronize()
        self.distinctive_descriptors_device(ids.data_ptr(), ids.numel())
        _ctx(self.device).sync()

    def Fuse(self, slot, point_ids, th=3.0):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) on the map: (nFused, status, best_idx,
        best_dist), status per point as include/orbg.h lists it"""
        p = _i32(point_ids)
        bi, bd, st = (np.zeros(len(p), np.int32) for _ in range(3))
        n = C.c_int32()
        L.check(L.lib().orbg_map_fuse(self._c(), self._h, int(slot), L.ptr(p), len(p), float(th),
                                      L.ptr(bi), L.ptr(bd), L.ptr(st), C.byref(n)), "orbg_map_fuse")
        return n.value, st, bi, bd

    def fuse_device(self, slot, d_point_ids, n, th, d_best_idx, d_best_dist, d_status, d_nfused,
                    ctx=None):
        L.check(L.lib().orbg_map_fuse_device(self._c(ctx), self._h, int(slot), d_point_ids, int(n),
                                             float(th), d_best_idx, d_best_dist, d_status,
                                             d_nfused), "orbg_map_fuse_device")

    def SearchInNeighbors(self, slot, current_kf_id, monocular, th=3.0):
        """LocalMapping::SearchInNeighbors: (vpTargetKFs as slots, duplicates included, the
        return value of each entry's Fuse, the second pass's)"""
        t = np.full(SIN_MAX_TARGETS, -1, np.int32)
        nf = np.zeros(SIN_MAX_TARGETS + 1, np.int32)
        n = C.c_int32()
        L.check(L.lib().orbg_map_search_in_neighbors(self._c(), self._h, int(slot),
                                                     int(current_kf_id), int(bool(monocular)),
                                                     float(th), L.ptr(t), len(t), C.byref(n),
                                                     L.ptr(nf)), "orbg_map_search_in_neighbors")
        return t[:n.value].tolist(), nf[:n.value].tolist(), int(nf[n.value])

    def search_in_neighbors_device(self, slot, current_kf_id, monocular, th, d_targets, target_cap,
                                   d_ntargets, d_nfused, ctx=None):
        L.check(L.lib().orbg_map_search_in_neighbors_device(
            self._c(ctx), self._h, int(slot), int(current_kf_id), int(bool(monocular)), float(th),
            d_targets, int(target_cap), d_ntargets, d_nfused),
            "orbg_map_search_in_neighbors_device")

    def replaced(self, first=0, n=None):
        """mpReplaced as ids (-1: none)"""
        n = self.max_points - first if n is None else int(n)
        out = np.zeros(n, np.int32)
        L.check(L.lib().orbg_map_get_point_replaced(self._c(), self._h, int(first), n, L.ptr(out)),
                "orbg_map_get_point_replaced")
        return out

    def descriptors(self, first=0, n=None):
        """mDescriptor of the points, uint8 [n][32]"""
        n = self.max_points - first if n is None else int(n)
        out = np.zeros((n, 32), np.uint8)
        L.check(L.lib().orbg_map_get_point_descriptors(self._c(), self._h, int(first), n,
                                                       L.ptr(out)),
                "orbg_map_get_point_descriptors")
        return out

    def point_refs(self, first=0, n=None):
        """mpRefKF as slots (-1: none)"""
        n = self.max_points - first if n is None else int(n)
        out = np.zeros(n, np.int32)
        L.check(L.lib().orbg_map_get_point_refs(self._c(), self._h, int(first), n, L.ptr(out)),
                "orbg_map_get_point_refs")
        return out

    # ---- LoopClosing::CorrectLoop: poses, loop edges, Propagate, LoopConnections ----
    def SetPoses(self, slots, Tcw=None, mnid=None):
        """KeyFrame::SetPose of the listed slots (Tcw [n, 3, 4] float32; the stored camera
        centre becomes -Rcw^T tcw) and / or their mnId; None leaves that half as it is."""
        s = _i32(slots)
        T = None if Tcw is None else np.ascontiguousarray(Tcw, np.float32).reshape(-1, 12)
        i = None if mnid is None else _i32(mnid)
        if (T is not None and len(T) != len(s)) or (i is not None and len(i) != len(s)):
            raise ValueError("slots, poses and ids differ in length")
        L.check(L.lib().orbg_map_set_keyframe_poses(self._c(), self._h, L.ptr(s), len(s), L.ptr(T),
                                                    L.ptr(i)), "orbg_map_set_keyframe_poses")

    def set_poses_device(self, d_slots, n, d_Tcw, d_mnid, ctx=None):
        L.check(L.lib().orbg_map_set_keyframe_poses_device(self._c(ctx), self._h, d_slots, int(n),
                                                           d_Tcw, d_mnid),
                "orbg_map_set_keyframe_poses_device")

    def poses(self, first=0, n=None):
        """(Tcw float32 [n, 3, 4], has_pose bool [n], mnId int32 [n], camera centres [n, 3])"""
        n = self.max_keyframes - first if n is None else int(n)
        T, h = np.zeros((n, 3, 4), np.float32), np.zeros(n, np.int32)
        i, c = np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        L.check(L.lib().orbg_map_get_keyframe_poses(self._c(), self._h, int(first), n, L.ptr(T),
                                                    L.ptr(h), L.ptr(i), L.ptr(c)),
                "orbg_map_get_keyframe_poses")
        return T, h != 0, i, c

    def AddLoopEdge(self, a, b):
        """KeyFrame::AddLoopEdge on both sides, as CorrectLoop calls it"""
        L.check(L.lib().orbg_map_add_loop_edge(self._c(), self._h, int(a), int(b)),
                "orbg_map_add_loop_edge")

    def GetLoopEdges(self, slot):
        """mspLoopEdges of a slot, ascending"""
        out, n = np.zeros(MAX_LOOP_EDGES, np.int32), C.c_int32()
        L.check(L.lib().orbg_map_get_loop_edges(self._c(), self._h, int(slot), L.ptr(out), len(out),
                                                C.byref(n)), "orbg_map_get_loop_edges")
        return out[:n.value].tolist()

    def corrected(self, first=0, n=None):
        """(mnCorrectedByKF, mnCorrectedReference) of the points"""
        n = self.max_points - first if n is None else int(n)
        a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
        L.check(L.lib().orbg_map_get_point_corrected(self._c(), self._h, int(first), n, L.ptr(a),
                                                     L.ptr(b)), "orbg_map_get_point_corrected")
        return a, b

    def Propagate(self, cur, Scw, set_cap=MAX_LOOP_SET):
        """CorrectLoop's Sim3 propagation (LoopClosing.cc:744-843 without the loop fusion) with
        mpCurrentKF = cur and mg2oScw = Scw (a SIM3D_DTYPE record or (q, t, s), q = x, y, z, w):
        (mvpCurrentConnectedKFs as slots, CorrectedSim3, NonCorrectedSim3), the tables
        SIM3D_DTYPE [max_keyframes] indexed by slot."""
        from .optimizer import sim3d_records
        S = sim3d_records(Scw if isinstance(Scw, np.ndarray) else [Scw])
        st = np.zeros(int(set_cap), np.int32)
        n = C.c_int32()
        co, nc = (np.zeros(self.max_keyframes, L.SIM3D_DTYPE) for _ in range(2))
        L.check(L.lib().orbg_map_propagate(self._c(), self._h, int(cur), L.ptr(S), L.ptr(st),
                                           len(st), C.byref(n), L.ptr(co), L.ptr(nc)),
                "orbg_map_propagate")
        return st[:n.value].tolist(), co, nc

    def propagate_device(self, cur, d_Scw, d_set, set_cap, d_nset, d_corrected, d_noncorrected,
                         d_status, ctx=None):
        L.check(L.lib().orbg_map_propagate_device(self._c(ctx), self._h, int(cur), d_Scw, d_set,
                                                  int(set_cap), d_nset, d_corrected,
                                                  d_noncorrected, d_status),
                "orbg_map_propagate_device")

    def LoopConnections(self, members):
        """CorrectLoop's LoopConnections (LoopClosing.cc:882-911) over the members in the given
        (vector) order: int32 [n, 2] slot pairs (i, j), by i then j ascending"""
        s = _i32(members)
        cap = max(len(s) * self.max_keyframes, 1)
        out, n = np.zeros((cap, 2), np.int32), C.c_int32()
        L.check(L.lib().orbg_map_loop_connections(self._c(), self._h, L.ptr(s), len(s), L.ptr(out),
                                                  cap, C.byref(n)), "orbg_map_loop_connections")
        return out[:n.value]

    def loop_connections_device(self, d_set, set_cap, d_nset, d_pairs, pair_cap, d_npairs,
                                ctx=None):
        L.check(L.lib().orbg_map_loop_connections_device(self._c(ctx), self._h, d_set, int(set_cap),
                                                         d_nset, d_pairs, int(pair_cap), d_npairs),
                "orbg_map_loop_connections_device")

    def EssentialGraph(self, cur, loop, corrected, noncorrected, members, pairs, edge_cap=None):
        """The walk of Optimizer::OptimizeEssentialGraph over the map (Optimizer.cc:1040-1258):
        (vert_slot int32 [nvert], fixed vertex, Scw, Snc SIM3D_DTYPE [nvert], edges EG_EDGE_DTYPE
        in the reference's order, edges left out because an end is no vertex) -- the inputs of
        OptimizeEssentialGraph / EssentialGraph.  corrected / noncorrected: Propagate's tables."""
        co = np.ascontiguousarray(corrected, L.SIM3D_DTYPE).reshape(-1)
        nc = np.ascontiguousarray(noncorrected, L.SIM3D_DTYPE).reshape(-1)
        if len(co) != self.max_keyframes or len(nc) != self.max_keyframes:
            raise ValueError("the Sim3 tables have max_keyframes entries")
        s = _i32(members)
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        K = self.max_keyframes
        cap = int(edge_cap) if edge_cap is not None else len(p) + K * (1 + MAX_LOOP_EDGES) + K * 32
        vs = np.zeros(K, np.int32)
        Scw, Snc = np.zeros(K, L.SIM3D_DTYPE), np.zeros(K, L.SIM3D_DTYPE)
        ed = np.zeros(cap, L.EG_EDGE_DTYPE)
        nv, fx, ne, sk = (C.c_int32() for _ in range(4))
        L.check(L.lib().orbg_map_essential_graph(self._c(), self._h, int(cur), int(loop), L.ptr(co),
                                                 L.ptr(nc), L.ptr(s), len(s), L.ptr(p), len(p),
                                                 L.ptr(vs), C.byref(nv), C.byref(fx), L.ptr(Scw),
                                                 L.ptr(Snc), L.ptr(ed), cap, C.byref(ne),
                                                 C.byref(sk)), "orbg_map_essential_graph")
        n = nv.value
        return vs[:n], fx.value, Scw[:n], Snc[:n], ed[:ne.value], sk.value

    def essential_graph_device(self, cur, loop, d_corrected, d_noncorrected, d_set, set_cap, d_nset,
                               d_pairs, pair_cap, d_npairs, d_vert_slot, d_nvert, d_fixed, d_Scw,
                               d_Snc, d_edges, edge_cap, d_nedge, d_status, ctx=None):
        L.check(L.lib().orbg_map_essential_graph_device(
            self._c(ctx), self._h, int(cur), int(loop), d_corrected, d_noncorrected, d_set,
            int(set_cap), d_nset, d_pairs, int(pair_cap), d_npairs, d_vert_slot, d_nvert, d_fixed,
            d_Scw, d_Snc, d_edges, int(edge_cap), d_nedge, d_status),
            "orbg_map_essential_graph_device")

    def ApplyCorrection(self, cur, vert_slot, Scw, Siw, Tiw):
        """Optimizer.cc:1264-1323: SetPose(Tiw[v]) per vertex, the map points' correction with
        Srw = Scw[r] and the optimised Siw[r], UpdateNormalAndDepth of all points."""
        v = _i32(vert_slot)
        a = np.ascontiguousarray(Scw, L.SIM3D_DTYPE).reshape(-1)
        b = np.ascontiguousarray(Siw, L.SIM3D_DTYPE).reshape(-1)
        T = np.ascontiguousarray(Tiw, np.float32).reshape(-1, 12)
        if not (len(v) == len(a) == len(b) == len(T)):
            raise ValueError("vert_slot, Scw, Siw and Tiw differ in length")
        L.check(L.lib().orbg_map_apply_correction(self._c(), self._h, int(cur), L.ptr(v), len(v),
                                                  L.ptr(a), L.ptr(b), L.ptr(T)),
                "orbg_map_apply_correction")

    def apply_correction_device(self, cur, d_vert_slot, d_nvert, d_Scw, d_Siw, d_Tiw, ctx=None):
        L.check(L.lib().orbg_map_apply_correction_device(self._c(ctx), self._h, int(cur),
                                                         d_vert_slot, d_nvert, d_Scw, d_Siw, d_Tiw),
                "orbg_map_apply_correction_device")

    def SetCorrected(self, first, corrected_by_kf, corrected_reference):
        """mnCorrectedByKF / mnCorrectedReference of the points first .. (a map uploaded from host
        state)"""
        a, b = _i32(corrected_by_kf), _i32(corrected_reference)
        if len(a) != len(b):
            raise ValueError("the two arrays differ in length")
        L.check(L.lib().orbg_map_set_point_corrected(self._c(), self._h, int(first), len(a), L.ptr(a),
                                                     L.ptr(b)), "orbg_map_set_point_corrected")

    def LoopFusion(self, cur, matched):
        """CorrectLoop's loop fusion (LoopClosing.cc:848-863) with mvpCurrentMatchedPoints as ids
        (-1 = none) in feature order: (replaced, added)"""
        p = _i32(matched)
        out = np.zeros(2, np.int32)
        L.check(L.lib().orbg_map_loop_fusion(self._c(), self._h, int(cur), L.ptr(p), len(p),
                                             L.ptr(out)), "orbg_map_loop_fusion")
        return int(out[0]), int(out[1])

    def loop_fusion_device(self, cur, d_matched, n, d_counts, ctx=None):
        L.check(L.lib().orbg_map_loop_fusion_device(self._c(ctx), self._h, int(cur), d_matched,
                                                    int(n), d_counts), "orbg_map_loop_fusion_device")

    def SearchAndFuse(self, members, corrected, loop_points, th=4.0):
        """LoopClosing::SearchAndFuse over the members in slot order with Propagate's
        CorrectedSim3 table and mvpLoopMapPoints as ids: (sum of nFused, replacements)"""
        s, p = _i32(members), _i32(loop_points)
        co = np.ascontiguousarray(corrected, L.SIM3D_DTYPE).reshape(-1)
        if len(co) != self.max_keyframes:
            raise ValueError("the Sim3 table has max_keyframes entries")
        out = np.zeros(2, np.int32)
        L.check(L.lib().orbg_map_search_and_fuse(self._c(), self._h, L.ptr(s), len(s), L.ptr(co),
                                                 L.ptr(p), len(p), float(th), L.ptr(out)),
                "orbg_map_search_and_fuse")
        return int(out[0]), int(out[1])

    def search_and_fuse_device(self, d_set, set_cap, d_nset, d_corrected, d_loop_points, n, th,
                               d_counts, ctx=None):
        L.check(L.lib().orbg_map_search_and_fuse_device(self._c(ctx), self._h, d_set, int(set_cap),
                                                        d_nset, d_corrected, d_loop_points, int(n),
                                                        float(th), d_counts),
                "orbg_map_search_and_fuse_device")

    def CorrectLoop(self, cur, loop, Scw, matched, loop_points, bFixScale):
        """LoopClosing::CorrectLoop in one call: (LM report dict, counts dict)"""
        from .optimizer import sim3d_records, _lm_report
        S = sim3d_records(Scw if isinstance(Scw, np.ndarray) else [Scw])
        a, b = _i32(matched), _i32(loop_points)
        rep, cnt = L.LmReport(), np.zeros(8, np.int32)
        L.check(L.lib().orbg_map_correct_loop(self._c(), self._h, int(cur), int(loop), L.ptr(S),
                                              L.ptr(a), len(a), L.ptr(b), len(b),
                                              1 if bFixScale else 0, C.byref(rep), L.ptr(cnt)),
                "orbg_map_correct_loop")
        keys = ("members", "fusion_replaced", "fusion_added", "fused", "replaced", "pairs",
                "vertices", "edges")
        return _lm_report(rep), dict(zip(keys, cnt.tolist()))

    # ---- Optimizer::LocalBundleAdjustment: the window, the write-back, all of it ----
    def LbaWindow(self, slot, pose_cap=None, point_cap=None, edge_cap=None):
        """The window of Optimizer::LocalBundleAdjustment(slot) (Optimizer.cc:635-851) as a dict:
        kf_slots (nlocal local keyframes, then the fixed cameras), nlocal, poses POSE_DTYPE,
        point_ids, points float64 [n, 3], edges EDGE_DTYPE, edge_feat (the keypoint index of each
        edge).  The keyframe data must be attached (AttachKeyFrames) and the poses set."""
        K = self.max_keyframes
        pc = K if pose_cap is None else int(pose_cap)
        qc = min(self.max_points, K * self.kf_cap, 524286) if point_cap is None else int(point_cap)
        ec = K * self.kf_cap if edge_cap is None else int(edge_cap)
        ks, po = np.zeros(pc, np.int32), np.zeros(pc, L.POSE_DTYPE)
        ids, pts = np.zeros(qc, np.int32), np.zeros((qc, 3), np.float64)
        ed, ef = np.zeros(ec, L.EDGE_DTYPE), np.zeros(ec, np.int32)
        cnt = np.zeros(4, np.int32)
        rc = L.lib().orbg_map_lba_window(self._c(), self._h, int(slot), L.ptr(ks), L.ptr(po), pc,
                                         L.ptr(ids), L.ptr(pts), qc, L.ptr(ed), L.ptr(ef), ec,
                                         L.ptr(cnt))
        self.lba_counts = cnt.tolist()      # the full counts, also after ORBG_ERANGE
        L.check(rc, "orbg_map_lba_window")
        nl, npo, nq, ne = cnt.tolist()
        return dict(kf_slots=ks[:npo], nlocal=nl, poses=po[:npo], point_ids=ids[:nq],
                    points=pts[:nq], edges=ed[:ne], edge_feat=ef[:ne])

    def lba_window_device(self, slot, d_kf_slots, d_poses, pose_cap, d_point_ids, d_points,
                          point_cap, d_edges, d_edge_feat, edge_cap, d_counts, d_status, ctx=None):
        L.check(L.lib().orbg_map_lba_window_device(
            self._c(ctx), self._h, int(slot), d_kf_slots, d_poses, int(pose_cap), d_point_ids,
            d_points, int(point_cap), d_edges, d_edge_feat, int(edge_cap), d_counts, d_status),
            "orbg_map_lba_window_device")

    def LbaApply(self, window, poses, points, erase, d_cams_out=None):
        """Optimizer.cc:943-978 on the table for a window of LbaWindow: the flagged observations
        erased (mono edges first, then stereo), SetPose of the local keyframes, the window
        points' positions and UpdateNormalAndDepth; d_cams_out (a device pointer, FRUSTUM_DTYPE
        per slot) gets the local keyframes' new Tcw.  Returns (observations erased, points gone
        bad)."""
        ks, ids = _i32(window["kf_slots"]), _i32(window["point_ids"])
        ed = np.ascontiguousarray(window["edges"], L.EDGE_DTYPE).reshape(-1)
        ef = _i32(window["edge_feat"])
        po = np.ascontiguousarray(poses, L.POSE_DTYPE).reshape(-1)
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        er = np.ascontiguousarray(np.asarray(erase) != 0, np.uint8).reshape(-1)
        if len(po) != len(ks) or len(pts) != len(ids) or not (len(ed) == len(ef) == len(er)):
            raise ValueError("the window and the estimates differ in length")
        out = np.zeros(2, np.int32)
        L.check(L.lib().orbg_map_lba_apply(self._c(), self._h, L.ptr(ks), int(window["nlocal"]),
                                           len(ks), L.ptr(ids), len(ids), L.ptr(ed), L.ptr(ef),
                                           len(ed), L.ptr(po), L.ptr(pts), L.ptr(er), d_cams_out,
                                           L.ptr(out)), "orbg_map_lba_apply")
        return int(out[0]), int(out[1])

    def lba_apply_device(self, d_kf_slots, pose_cap, d_point_ids, point_cap, d_edges, d_edge_feat,
                         edge_cap, d_counts, d_poses, d_points, d_erase, d_cams_out, d_out,
                         ctx=None):
        L.check(L.lib().orbg_map_lba_apply_device(
            self._c(ctx), self._h, d_kf_slots, int(pose_cap), d_point_ids, int(point_cap), d_edges,
            d_edge_feat, int(edge_cap), d_counts, d_poses, d_points, d_erase, d_cams_out, d_out),
            "orbg_map_lba_apply_device")

    def LocalBundleAdjustment(self, slot, stop_flag=None, d_cams_out=None, post_iteration=None):
        """Optimizer::LocalBundleAdjustment(slot, stop_flag, map) in one call: the window, the
        stop check, optimize(5) / the outlier pass / optimize(10) on the device estimates, the
        write-back.  stop_flag: a one-byte host buffer (numpy uint8 [1] or ctypes c_bool), polled
        as g2o polls it; post_iteration(it): a callback after every LM iteration (it may raise
        the flag).  Returns the report as a dict (stopped = 1: the flag was up, nothing written)."""
        from .optimizer import _lm_report, _stop_flag_address
        rep, ctl = L.MapLbaReport(), L.LmControl()
        ctl.force_stop = _stop_flag_address(stop_flag)
        pi = L.LM_POST_ITERATION((lambda u, it: post_iteration(it)) if post_iteration else 0)
        ctl.post_iteration = pi
        L.check(L.lib().orbg_map_local_ba(self._c(), self._h, int(slot), C.byref(ctl), d_cams_out,
                                          C.byref(rep)), "orbg_map_local_ba")
        out = {k: int(getattr(rep, k)) for k in ("nlocal", "nfixed", "npoints", "nedges", "nerased",
                                                 "npoints_bad", "stopped")}
        out.update(lm=[_lm_report(rep.lba.lm[0]), _lm_report(rep.lba.lm[1])],
                   do_more=int(rep.lba.do_more), n_outliers=int(rep.lba.n_outliers),
                   n_erase=int(rep.lba.n_erase))
        return out

    # ---- Optimizer::GlobalBundleAdjustemnt and RunGlobalBundleAdjustment on the table ----
    def gba_state(self, first_slot=0, nslots=None, first_point=0, npoints=None):
        """dict of mTcwGBA / mTcwBefGBA float32 [n, 3, 4] and kf_ba_global int32 [n] of the slot
        range, mPosGBA float32 [m, 3] and mp_ba_global int32 [m] of the point range"""
        ns = self.max_keyframes - first_slot if nslots is None else int(nslots)
        npt = self.max_points - first_point if npoints is None else int(npoints)
        out = dict(TcwGBA=np.zeros((ns, 3, 4), np.float32), TcwBefGBA=np.zeros((ns, 3, 4), np.float32),
                   kf_ba_global=np.zeros(ns, np.int32), PosGBA=np.zeros((npt, 3), np.float32),
                   mp_ba_global=np.zeros(npt, np.int32))
        L.check(L.lib().orbg_map_get_gba_state(
            self._c(), self._h, int(first_slot), ns, L.ptr(out["TcwGBA"]), L.ptr(out["TcwBefGBA"]),
            L.ptr(out["kf_ba_global"]), int(first_point), npt, L.ptr(out["PosGBA"]),
            L.ptr(out["mp_ba_global"])), "orbg_map_get_gba_state")
        return out

    def SetGbaState(self, first_slot=0, TcwGBA=None, TcwBefGBA=None, kf_ba_global=None,
                    first_point=0, PosGBA=None, mp_ba_global=None):
        """Uploads the global BA state of a map built from host objects; None leaves that array
        as it is.  The slot arrays share one length, the point arrays another."""
        T = None if TcwGBA is None else np.ascontiguousarray(TcwGBA, np.float32).reshape(-1, 12)
        B = None if TcwBefGBA is None else np.ascontiguousarray(TcwBefGBA, np.float32).reshape(-1, 12)
        k = None if kf_ba_global is None else _i32(kf_ba_global)
        X = None if PosGBA is None else np.ascontiguousarray(PosGBA, np.float32).reshape(-1, 3)
        q = None if mp_ba_global is None else _i32(mp_ba_global)
        ns = {len(a) for a in (T, B, k) if a is not None}
        npt = {len(a) for a in (X, q) if a is not None}
        if len(ns) > 1 or len(npt) > 1:
            raise ValueError("the state arrays differ in length")
        L.check(L.lib().orbg_map_set_gba_state(
            self._c(), self._h, int(first_slot), ns.pop() if ns else 0, L.ptr(T), L.ptr(B), L.ptr(k),
            int(first_point), npt.pop() if npt else 0, L.ptr(X), L.ptr(q)), "orbg_map_set_gba_state")

    def GbaWindow(self, robust, pose_cap=None, point_cap=None, edge_cap=None):
        """The graph Optimizer::BundleAdjustment builds from every keyframe and map point
        (Optimizer.cc:113-246) as a dict: kf_slots (live and not bad, ascending), poses POSE_DTYPE
        (fixed iff mnId 0), point_ids (good, with an edge), points float64 [n, 3], edges
        EDGE_DTYPE, edge_feat, left_out (good points without an edge).  The keyframe data must be
        attached and the poses set."""
        K = self.max_keyframes
        pc = K if pose_cap is None else int(pose_cap)
        qc = self.max_points if point_cap is None else int(point_cap)
        ec = K * self.kf_cap if edge_cap is None else int(edge_cap)
        ks, po = np.zeros(pc, np.int32), np.zeros(pc, L.POSE_DTYPE)
        ids, pts = np.zeros(qc, np.int32), np.zeros((qc, 3), np.float64)
        ed, ef = np.zeros(ec, L.EDGE_DTYPE), np.zeros(ec, np.int32)
        cnt = np.zeros(4, np.int32)
        rc = L.lib().orbg_map_gba_window(self._c(), self._h, int(bool(robust)), L.ptr(ks), L.ptr(po),
                                         pc, L.ptr(ids), L.ptr(pts), qc, L.ptr(ed), L.ptr(ef), ec,
                                         L.ptr(cnt))
        self.gba_counts = cnt.tolist()      # the full counts, also after ORBG_ERANGE
        L.check(rc, "orbg_map_gba_window")
        npo, nq, ne, left = cnt.tolist()
        return dict(kf_slots=ks[:npo], poses=po[:npo], point_ids=ids[:nq], points=pts[:nq],
                    edges=ed[:ne], edge_feat=ef[:ne], left_out=left)

    def gba_window_device(self, robust, d_kf_slots, d_poses, pose_cap, d_point_ids, d_points,
                          point_cap, d_edges, d_edge_feat, edge_cap, d_counts, d_status, ctx=None):
        L.check(L.lib().orbg_map_gba_window_device(
            self._c(ctx), self._h, int(bool(robust)), d_kf_slots, d_poses, int(pose_cap), d_point_ids,
            d_points, int(point_cap), d_edges, d_edge_feat, int(edge_cap), d_counts, d_status),
            "orbg_map_gba_window_device")

    def GbaStore(self, window, poses, points, loop_kf, d_cams_out=None):
        """Optimizer.cc:273-318 for a window of GbaWindow.  loop_kf == 0: SetPose, SetWorldPos and
        UpdateNormalAndDepth; otherwise mTcwGBA / mPosGBA and mnBAGlobalForKF = loop_kf.  Returns
        (keyframes written, points written)."""
        ks, ids = _i32(window["kf_slots"]), _i32(window["point_ids"])
        po = np.ascontiguousarray(poses, L.POSE_DTYPE).reshape(-1)
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        if len(po) != len(ks) or len(pts) != len(ids):
            raise ValueError("the window and the estimates differ in length")
        out = np.zeros(2, np.int32)
        L.check(L.lib().orbg_map_gba_store(self._c(), self._h, L.ptr(ks), len(ks), L.ptr(ids),
                                           len(ids), L.ptr(po), L.ptr(pts), int(loop_kf), d_cams_out,
                                           L.ptr(out)), "orbg_map_gba_store")
        return int(out[0]), int(out[1])

    def gba_store_device(self, d_kf_slots, pose_cap, d_point_ids, point_cap, d_counts, d_poses,
                         d_points, loop_kf, d_cams_out, d_out, ctx=None):
        L.check(L.lib().orbg_map_gba_store_device(
            self._c(ctx), self._h, d_kf_slots, int(pose_cap), d_point_ids, int(point_cap), d_counts,
            d_poses, d_points, int(loop_kf), d_cams_out, d_out), "orbg_map_gba_store_device")

    def keyframe_flags(self, first=0, n=None):
        """KF_ROOT | KF_BAD per slot, and 4 for a live slot"""
        n = self.max_keyframes - first if n is None else int(n)
        out = np.zeros(n, np.int32)
        L.check(L.lib().orbg_map_get_keyframe_flags(self._c(), self._h, int(first), n, L.ptr(out)),
                "orbg_map_get_keyframe_flags")
        return out

    def _origins(self, origins):
        """mvpKeyFrameOrigins as slots; None: the live KF_ROOT slots"""
        if origins is not None:
            return _i32(origins)
        f = self.keyframe_flags()
        return _i32(np.nonzero((f & (4 | KF_ROOT)) == (4 | KF_ROOT))[0])

    def GbaUpdate(self, loop_kf, origins=None, d_cams_out=None):
        """The map update of LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:1056-1116):
        the spanning-tree propagation from the origins (mvpKeyFrameOrigins as slots) and the map
        points.  Returns [visited, propagated, points from mPosGBA, points moved, points skipped,
        0]."""
        o = self._origins(origins)
        out = np.zeros(6, np.int32)
        L.check(L.lib().orbg_map_gba_update(self._c(), self._h, L.ptr(o), len(o), int(loop_kf),
                                            d_cams_out, L.ptr(out)), "orbg_map_gba_update")
        return out.tolist()

    def gba_update_device(self, d_origins, norigins, loop_kf, d_cams_out, d_out, d_status, ctx=None):
        L.check(L.lib().orbg_map_gba_update_device(
            self._c(ctx), self._h, d_origins, int(norigins), int(loop_kf), d_cams_out, d_out,
            d_status), "orbg_map_gba_update_device")

    @staticmethod
    def _gba_report(rep):
        from .optimizer import _lm_report
        out = {k: int(getattr(rep, k)) for k in ("nposes", "npoints", "nedges", "nleft_out", "stopped")}
        out.update(lm=_lm_report(rep.gba.lm), store=list(rep.store), update=list(rep.update),
                   plan={k: int(getattr(rep.gba.plan, k)) for k, _ in L.BaSparseInfo._fields_})
        return out

    def _lm_control(self, stop_flag, post_iteration):
        from .optimizer import _stop_flag_address
        ctl = L.LmControl()
        ctl.force_stop = _stop_flag_address(stop_flag)
        pi = L.LM_POST_ITERATION((lambda u, it: post_iteration(it)) if post_iteration else 0)
        ctl.post_iteration = pi
        return ctl, pi

    def GlobalBundleAdjustment(self, iterations=5, stop_flag=None, loop_kf=0, robust=True,
                               d_cams_out=None, post_iteration=None):
        """Optimizer::GlobalBundleAdjustemnt(map, iterations, stop_flag, loop_kf, robust) in one
        call: the window, optimize(iterations) on the device estimates, the store.  Returns the
        report as a dict."""
        rep = L.MapGbaReport()
        ctl, keep = self._lm_control(stop_flag, post_iteration)
        L.check(L.lib().orbg_map_global_ba(self._c(), self._h, int(iterations), int(bool(robust)),
                                           int(loop_kf), C.byref(ctl), d_cams_out, C.byref(rep)),
                "orbg_map_global_ba")
        return self._gba_report(rep)

    def RunGlobalBundleAdjustment(self, loop_kf, origins=None, stop_flag=None, d_cams_out=None,
                                  post_iteration=None):
        """LoopClosing::RunGlobalBundleAdjustment(loop_kf): global BA with 10 iterations, not
        robust, then the map update unless the flag is up (stopped = 1: the GBA state is stored,
        poses and positions are untouched)."""
        o = self._origins(origins)
        rep = L.MapGbaReport()
        ctl, keep = self._lm_control(stop_flag, post_iteration)
        L.check(L.lib().orbg_map_run_global_ba(self._c(), self._h, L.ptr(o), len(o), int(loop_kf),
                                               C.byref(ctl), d_cams_out, C.byref(rep)),
                "orbg_map_run_global_ba")
        return self._gba_report(rep)

    # ---- LocalMapping::ProcessNewKeyFrame / CreateNewMapPoints on the table ----
    def AttachKeyFrameGeometry(self, d_kps_raw, d_depth, d_kf_cams):
        """What the triangulation reads beside AttachKeyFrames' arrays, device pointers indexed
        by slot with the attached cap: mvKeys (None: mvKeysUn), mvDepth (needed with mvuRight),
        KF_CAMERA_DTYPE records of which the intrinsics fx .. mbf are read (the pose is the
        Map's own, SetPoses).  d_kf_cams None detaches."""
        L.check(L.lib().orbg_map_attach_keyframe_geometry(self._c(), self._h, d_kps_raw, d_depth,
                                                          d_kf_cams),
                "orbg_map_attach_keyframe_geometry")

    def create_new_points_device(self, slot, current_kf_id, monocular, first_id, d_abort, d_recent,
                                 recent_cap, d_nrecent, d_neigh, d_neigh_status, d_nmatches,
                                 d_nnew, d_tri_status, d_out, ctx=None):
        L.check(L.lib().orbg_map_create_new_points_device(
            self._c(ctx), self._h, int(slot), int(current_kf_id), int(bool(monocular)),
            int(first_id), d_abort, d_recent, int(recent_cap), d_nrecent, d_neigh, d_neigh_status,
            d_nmatches, d_nnew, d_tri_status, d_out), "orbg_map_create_new_points_device")

    def CreateNewMapPoints(self, slot, current_kf_id, monocular, first_id, recent, abort=None,
                           recent_cap=None, tri_status=False):
        """LocalMapping::CreateNewMapPoints on the table: the new points get the ids first_id,
        first_id + 1, .. in creation order and are appended to `recent`.  abort: None or an
        int (CheckNewKeyFrames() from the second neighbour on).  Returns (recent, report);
        report: neigh, status (0 processed, 1 baseline, 2 aborted, 3 unusable), nmatches, nnew
        per neighbour, created, needed, bits (CNP_*), rc (ORBG_OK or ORBG_ERANGE when a cap cut
        the creation short) and, if asked for, tri_status [neighbours][kf_cap]."""
        r = _i32(recent)
        cap = len(r) + self.kf_cap if recent_cap is None else int(recent_cap)
        buf = np.full(max(cap, 1), -1, np.int32)
        buf[:len(r)] = r
        n = C.c_int32(len(r))
        ab = None if abort is None else np.array([int(abort)], np.int32)
        ng, st, nm, nw = (np.zeros(20, np.int32) for _ in range(4))
        ts = np.zeros((20, self.kf_cap), np.int8) if tri_status else None
        out = np.zeros(4, np.int32)
        rc = L.lib().orbg_map_create_new_points(
            self._c(), self._h, int(slot), int(current_kf_id), int(bool(monocular)), int(first_id),
            L.ptr(ab), L.ptr(buf), cap, C.byref(n), L.ptr(ng), L.ptr(st), L.ptr(nm), L.ptr(nw),
            L.ptr(ts), L.ptr(out))
        if rc != L.ORBG_ERANGE:
            L.check(rc, "orbg_map_create_new_points")
        k = int(out[0])
        rep = dict(neigh=ng[:k].tolist(), status=st[:k].tolist(), nmatches=nm[:k].tolist(),
                   nnew=nw[:k].tolist(), created=int(out[1]), needed=int(out[2]), bits=int(out[3]),
                   rc=rc)
        if tri_status:
            rep["tri_status"] = ts[:k]
        return buf[:n.value].copy(), rep

    def process_new_keyframe_device(self, slot, d_point_ids, d_octaves, d_feat_flags, n, d_Tcw,
                                    mnid, kf_flags, d_in_keyframe, d_recent, recent_cap, d_nrecent,
                                    d_out, ctx=None):
        L.check(L.lib().orbg_map_process_new_keyframe_device(
            self._c(ctx), self._h, int(slot), d_point_ids, d_octaves, d_feat_flags, int(n), d_Tcw,
            int(mnid), int(kf_flags), d_in_keyframe, d_recent, int(recent_cap), d_nrecent, d_out),
            "orbg_map_process_new_keyframe_device")

    def ProcessNewKeyFrame(self, slot, point_ids, octaves, feat_flags, Tcw, mnid, in_keyframe=None,
                           recent=(), root=False, recent_cap=None):
        """The table side of LocalMapping::ProcessNewKeyFrame: the row, features, pose and mnId
        of `slot` are stored (a bad or out-of-range id as -1), the ids flagged in_keyframe
        (pMP->IsInKeyFrame(pKF) as Tracking left it) are appended to `recent`, the other good
        points get UpdateNormalAndDepth and ComputeDistinctiveDescriptors, then
        UpdateConnections(slot).  Returns (recent, report)."""
        p = _i32(point_ids)
        o = np.ascontiguousarray(octaves, np.uint8).reshape(-1)
        f = None if feat_flags is None else np.ascontiguousarray(feat_flags, np.uint8).reshape(-1)
        k = None if in_keyframe is None else np.ascontiguousarray(np.asarray(in_keyframe) != 0,
                                                                   np.uint8).reshape(-1)
        if len(o) != len(p) or any(x is not None and len(x) != len(p) for x in (f, k)):
            raise ValueError("the row's arrays differ in length")
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        r = _i32(recent)
        cap = len(r) + len(p) if recent_cap is None else int(recent_cap)
        buf = np.full(max(cap, 1), -1, np.int32)
        buf[:len(r)] = r
        n = C.c_int32(len(r))
        out = np.zeros(4, np.int32)
        rc = L.lib().orbg_map_process_new_keyframe(
            self._c(), self._h, int(slot), L.ptr(p), L.ptr(o), L.ptr(f), len(p), L.ptr(T), int(mnid),
            KF_ROOT if root else 0, L.ptr(k), L.ptr(buf), cap, C.byref(n), L.ptr(out))
        if rc != L.ORBG_ERANGE:
            L.check(rc, "orbg_map_process_new_keyframe")
        return buf[:n.value].copy(), dict(appended=int(out[0]), updated=int(out[1]),
                                          needed=int(out[2]), bits=int(out[3]), rc=rc)
