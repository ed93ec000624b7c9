// map_args.h -- device layout and launch arguments of the covisibility Map (map_kernels.hip:
// KeyFrame::UpdateConnections, Tracking::UpdateLocalKeyFrames / UpdateLocalPoints,
// MapPoint::UpdateNormalAndDepth; map_cull_kernels.hip; map_edit_kernels.hip;
// map_loop_kernels.hip, map_lba_kernels.hip, map_gba_kernels.hip, map_create_kernels.hip), shared with the
// host entry points (api_map.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbg.h"

namespace orbg {

#define ORBG_MAP_MAX_KEYFRAMES 8192   // = ORBG_KFDB_MAX_KEYFRAMES: a slot is 13 bits of a sort key
#define ORBG_MAP_MAX_KF_CAP 8192      // a feature index is 13 bits of an observation entry
#define ORBG_MAP_MAX_FRAME_CAP 8192   // UpdateLocalPoints sorts the frame's own points in LDS
#define ORBG_MAP_NEIGH 10             // GetBestCovisibilityKeyFrames(10)
#define ORBG_MAP_TH 15                // UpdateConnections' th
#define ORBG_MAP_MAX_LOCAL 80         // UpdateLocalKeyFrames' size limit
#define MAP_KF_LIVE 4                 // kf_flags: beside ORBG_MAP_KF_ROOT (1) and ORBG_MAP_KF_BAD (2)
#define MAP_NOT_ERASE 1               // kf_erase: mbNotErase
#define MAP_TO_BE_ERASED 2            //           mbToBeErased

// An orbg_map's device state.  Slot s (the caller's KeyFrame handle, as orbg_kfdb's) owns row s
// of kf_points / kf_oct and of W / ord_*; point p owns mp[p], mdesc[p], mp_ref[p].  The
// observation index is a CSR over the points: obs[obs_off[p] .. obs_off[p + 1]) are p's
// observations as slot << 16 | feature index, ascending slot, rebuilt from the live rows when
// stale.  child_head / child_next are the spanning tree's children lists (ascending slot),
// rebuilt from `parent` when stale.  dirty / mark hold the number of the call that last set
// them (UpdateConnections' second kernel re-sorts the rows this call marked dirty).  row_touch
// holds the number of the culling call in which an erasure last changed Observations() of one
// of the row's points or removed one from it.
struct MapDev {
    int32_t K, cap, P;
    int32_t *kf_flags;          // [K] MAP_KF_LIVE | ORBG_MAP_KF_*
    int32_t *kf_n;              // [K]
    int32_t *kf_points;         // [K][cap] point id, -1 = none
    uint8_t *kf_oct;            // [K][cap] mvKeysUn[idx].octave
    float *kf_centre;           // [K][3] GetCameraCenter()
    int32_t *parent;            // [K] slot or -1
    int32_t *first_conn;        // [K] mbFirstConnection
    orbg_map_point *mp;         // [P]
    uint8_t *mdesc;             // [P][32]
    int32_t *mp_ref;            // [P] mpRefKF as a slot
    uint16_t *W;                // [K][K] mConnectedKeyFrameWeights, 0 = not connected
    uint16_t *ord_slot;         // [K][K] mvpOrderedConnectedKeyFrames
    uint16_t *ord_w;            // [K][K] mvOrderedWeights
    int32_t *nord;              // [K]
    int32_t *neigh;             // [K][10] the first ten of ord_slot, -1 padded
    int32_t *obs_off;           // [P + 1]
    int32_t *obs_cnt;           // [P] histogram, then the fill cursors
    int32_t *part;              // [ceil(P / 2048) + 1] the scan's tile sums
    uint32_t *obs_tmp;          // [K * cap] the fill, in arrival order
    uint32_t *obs;              // [K * cap]
    int32_t *child_head;        // [K]
    int32_t *child_next;        // [K]
    int32_t *dirty, *mark;      // [K]
    int32_t *nlive;             // [1]
    uint8_t *kf_feat;           // [K][cap] ORBG_MAP_FEAT_*
    int32_t *kf_erase;          // [K] MAP_NOT_ERASE | MAP_TO_BE_ERASED
    int32_t *mp_first;          // [P] mnFirstKFid
    int32_t *mp_visible;        // [P] mnVisible
    int32_t *mp_found;          // [P] mnFound
    int32_t *row_touch;         // [K]
    int32_t *cull_list;         // [K] KeyFrameCulling's copy of the ordered list
    int32_t *cull_score;        // [K][2] nMPs, nRedundant of the list entries at the call's start
    int32_t *cull_out;          // [4] a status for the host forms
    int32_t *mp_replaced;       // [P] mpReplaced as an id, -1 = none
    // map_edit_kernels.hip: valid where the stamp equals the number of the running call
    int32_t *ed_next, *ed_tail; // [P] the points merged into a point during this call, as a list
    int32_t *ed_chain;          // [P] stamp of ed_next / ed_tail
    int32_t *ed_inkf;           // [P] stamp: the point entered the Fuse keyframe's row in this call
    int32_t *ed_mark;           // [P] stamp: the point is already listed for its descriptor
    int32_t *ed_first;          // [P] SearchInNeighbors: first position of a fuse candidate
    // map_loop_kernels.hip: what LoopClosing::CorrectLoop reads beside the table
    float *kf_Tcw;              // [K][12] GetPose(), 3x4 row-major
    int32_t *kf_pose;           // [K] 1 = the slot has a pose
    int32_t *kf_mnid;           // [K] mnId, the slot by default
    int32_t *le_n;              // [K] mspLoopEdges
    int32_t *le_slot;           // [K][ORBG_MAP_MAX_LOOP_EDGES] in arrival order
    int32_t *mp_corr_kf;        // [P] mnCorrectedByKF
    int32_t *mp_corr_ref;       // [P] mnCorrectedReference
    float *lp_T, *lp_c;         // [K][12], [K][3] the corrected poses / centres of a running Propagate
    int32_t *lp_pos;            // [K] position in mvpCurrentConnectedKFs, -1 = not a member
    int32_t *lp_hdr;            // [16] LOOP_HDR_*
    uint16_t *lp_snap;          // [K] LoopConnections: vpPreviousNeighbors
    int32_t *mp_corr_slot;      // [P] the slot Propagate wrote mnCorrectedReference for (a hint: checked against kf_mnid)
    int32_t *lp_vmap;           // [K] essential graph: slot -> vertex, -1 = none
    int32_t *lp_ecnt;           // [K + 1] its kind-1 edges per vertex, then their offsets
    // map_gba_kernels.hip: what global BA leaves for LoopClosing::RunGlobalBundleAdjustment
    float *kf_TcwGBA;           // [K][12] mTcwGBA, 3x4 row-major
    float *kf_TcwBef;           // [K][12] mTcwBefGBA
    int32_t *kf_gba;            // [K] KeyFrame::mnBAGlobalForKF, 0 for a slot that becomes live
    float *mp_posGBA;           // [P][3] mPosGBA
    int32_t *mp_gba;            // [P] MapPoint::mnBAGlobalForKF, 0 for a created point
};
#define LOOP_HDR_SLOT 0               // the slot of the running UpdateConnections, -1 = none
#define LOOP_HDR_NSET 1               // members the running call acts on
#define LOOP_HDR_NSNAP 3
#define LOOP_HDR_NVERT 4
#define LOOP_HDR_N0 5                 // kept kind-0 edges
#define LOOP_HDR_SKIP 6               // edges left out: an end is not a vertex
#define LOOP_HDR_BITS 7               // ORBG_LOOP_* of the running assembly

struct MapScales {
    float scale[16];
    int32_t nlevels;
};

struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_map_set_keyframes(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                             const int32_t *points, const uint8_t *oct, int row_cap,
                             const int32_t *counts, const float *centres, const int32_t *flags);
int launch_map_set_points(hipStream_t st, const MapDev &M, const int32_t *ids, int first, int n,
                          const orbg_map_point *mps, const uint8_t *desc, const int32_t *ref);
int launch_map_point_bad(hipStream_t st, const MapDev &M, int id);
int launch_map_set_parent(hipStream_t st, const MapDev &M, int slot, int parent);
int launch_map_resort(hipStream_t st, const MapDev &M, int epoch);
int launch_map_erase(hipStream_t st, const MapDev &M, int slot, int epoch);
int launch_map_count(hipStream_t st, const MapDev &M);
int launch_map_rebuild(hipStream_t st, const MapDev &M, Prof *prof);
int launch_map_tree(hipStream_t st, const MapDev &M);
int launch_map_update_connections(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                                  int epoch, Prof *prof);
int launch_map_connected(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                         int32_t *conn, int conn_cap, int32_t *nconn);
int launch_map_local_keyframes(hipStream_t st, const MapDev &M, int32_t *frame_points,
                               int frame_cap, const int32_t *counts, int nframes,
                               int32_t *local_kfs, int lkf_cap, int32_t *nlocal, int32_t *ref_kf,
                               Prof *prof);
int launch_map_local_points(hipStream_t st, const MapDev &M, const int32_t *local_kfs, int lkf_cap,
                            const int32_t *nlocal, const int32_t *frame_points, int frame_cap,
                            const int32_t *counts, int nframes, int32_t *cnt, int32_t *ids,
                            orbg_map_point *mps, uint8_t *qdesc, int lp_cap, int32_t *nlp,
                            Prof *prof);
int launch_map_normal_depth(hipStream_t st, const MapDev &M, const int32_t *ids, int n,
                            const MapScales &S, Prof *prof);

// map_cull_kernels.hip
int launch_map_point_defaults(hipStream_t st, const MapDev &M);
int launch_map_set_features(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                            const uint8_t *flags, int row_cap, const int32_t *counts);
int launch_map_set_point_stats(hipStream_t st, const MapDev &M, const int32_t *ids, int first, int n,
                               const int32_t *first_kf, const int32_t *visible,
                               const int32_t *found);
int launch_map_point_nobs(hipStream_t st, const MapDev &M, int first, int n, int32_t *nobs);
int launch_map_increase(hipStream_t st, int32_t *counter, int P, const int32_t *ids,
                        const orbg_map_projection *proj, int n, int amount);
// on: 1 SetNotErase, 0 SetErase, -1 SetBadFlag; status (device): SetBadFlag's, or 1 when
// SetErase erased
int launch_map_set_bad(hipStream_t st, const MapDev &M, int slot, int on, int epoch,
                       int32_t *status, Prof *prof);
int launch_map_keyframe_culling(hipStream_t st, const MapDev &M, int slot, int monocular,
                                int epoch, orbg_cull_record *rec, int rec_cap, int32_t *nrec,
                                Prof *prof);
int launch_map_point_culling(hipStream_t st, const MapDev &M, int32_t *recent, int n,
                             int current_kf_id, int monocular, int32_t *nout, int32_t *status,
                             Prof *prof);

// map_edit_kernels.hip: the attached keyframe data, the map-owned workspace of one Fuse /
// SearchInNeighbors call (ncap entries per array) and the launches
#define ORBG_MAP_MAX_TARGETS 120      // SearchInNeighbors: 20 first-level + 20 * 5 second-level
#define ORBG_MAP_TH_LOW 50            // ORBmatcher::TH_LOW
struct MapAttach {
    orbg_keyframes kfs;               // indexed by slot, rows of `cap`
    int32_t cap;
    const orbg_frustum_camera *cams;  // [K]
};
struct MapEditWs {
    int32_t ncap;
    int32_t *hdr;                     // [16] MAP_HDR_*: the job (slot, count, active), the search's own count
    orbg_frustum_camera *cam;         // [1] the job's camera
    int32_t *targets;                 // [ORBG_MAP_MAX_TARGETS + 8], ntargets behind them
    int32_t *snap;                    // [cap + 1] the slot's row, its length behind it
    int32_t *ids;                     // [ncap + 1] fuse candidates, their count behind them
    orbg_map_point *mps;              // [ncap] the search inputs
    uint8_t *mdesc;                   // [ncap][32]
    int32_t *bidx, *bdist;            // [ncap] the search outputs
    int32_t *hits, *surv;             // [ncap] the points with a target, the survivors
    int32_t *dd_off, *dd_best;        // [ncap + 1], [ncap]
    uint8_t *dd_desc;                 // [ncap][32]
};
#define MAP_HDR_SLOT 0
#define MAP_HDR_N 1
#define MAP_HDR_ACTIVE 2
#define MAP_HDR_SEARCH 3
#define MAP_HDR_CUR 8                 // the searched slot, for UpdateConnections
#define MAP_HDR_TOT 10                // [2] launch_map_distinctive's totals
int launch_map_add_observations(hipStream_t st, const MapDev &M, const int32_t *slots,
                                const int32_t *idx, const int32_t *ids, int n, int32_t *status);
// ComputeDistinctiveDescriptors of ids[i], i < min(n, dn[0]) (dn NULL: n), over a current
// observation index; rows = M.obs_tmp, off [n + 1] / tot [2] / best [n] / desc [n][32] workspace
int launch_map_distinctive(hipStream_t st, const MapDev &M, const MapAttach &A, const int32_t *ids,
                           int n, const int32_t *dn, int epoch, int32_t *off, int32_t *tot,
                           int32_t *best, uint8_t *desc);
int launch_map_replace(hipStream_t st, const MapDev &M, const int32_t *olds, const int32_t *news,
                       int n, int epoch, int32_t *status, int32_t *surv);
// job: slot >= 0: that slot with n ids; slot < 0: entry `entry` of W.targets with W.snap
// (entry < ORBG_MAP_MAX_TARGETS) or the slot `cur` with W.ids (entry == ORBG_MAP_MAX_TARGETS)
int launch_map_fuse_job(hipStream_t st, const MapDev &M, const MapAttach &A, const MapEditWs &W,
                        int slot, int n, int entry, int cur);
int launch_map_fuse_gather(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                           int nmax);
int launch_map_fuse_update(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                           int nmax, int epoch, int32_t *best_idx, int32_t *best_dist,
                           int32_t *status, int32_t *nfused, int nfused_at_ntargets);
// CorrectLoop's loop fusion and SearchAndFuse (map_edit_kernels.hip); surv [M.cap], counts [2]
int launch_map_loop_fusion(hipStream_t st, const MapDev &M, int cur, const int32_t *matched, int nm,
                           int epoch, int32_t *surv, int32_t *counts);
int launch_map_sf_job(hipStream_t st, const MapDev &M, const MapAttach &A, const MapEditWs &W,
                      const int32_t *set, int set_cap, const int32_t *nset, int rank,
                      const orbg_sim3d *corrected, int n);
int launch_map_sf_update(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                         int nmax, int epoch, int32_t *counts);
int launch_map_sin_targets(hipStream_t st, const MapDev &M, const MapEditWs &W, int slot,
                           int current_kf_id, int monocular, int32_t *targets, int target_cap,
                           int32_t *ntargets, int32_t *nfused);
int launch_map_sin_candidates(hipStream_t st, const MapDev &M, const MapEditWs &W);
int launch_map_sin_row(hipStream_t st, const MapDev &M, const MapEditWs &W, int slot);


// map_loop_kernels.hip
int launch_map_loop_defaults(hipStream_t st, const MapDev &M);
int launch_map_set_poses(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                         const float *Tcw, const int32_t *mnid);
int launch_map_add_loop_edge(hipStream_t st, const MapDev &M, int a, int b, int32_t *status);
// UpdateConnections(cur), the set and the two Sim3 tables; then the map-point loop, SetPose and
// UpdateConnections per member.  status [4]: bits, the set's full length
int launch_map_propagate(hipStream_t st, const MapDev &M, int cur, const orbg_sim3d *Scw,
                         int32_t *set, int set_cap, int32_t *nset, orbg_sim3d *corrected,
                         orbg_sim3d *noncorrected, int32_t *status, const MapScales &S,
                         int *epoch, Prof *prof);
// rows [set_cap][K] / cnt [set_cap]: each member's new connections, the caller's workspace
int launch_map_loop_connections(hipStream_t st, const MapDev &M, const int32_t *set, int set_cap,
                                const int32_t *nset, uint16_t *rows, int32_t *cnt, int32_t *pairs,
                                int pair_cap, int32_t *npairs, int *epoch, Prof *prof);
// Optimizer.cc:1040-1258 on the map: vertices, Scw / Snc per vertex, the edge list in the
// reference's order.  status [4]: ORBG_LOOP_* bits, the edges left out because an end is no vertex
int launch_map_essential_graph(hipStream_t st, const MapDev &M, int cur, int loop,
                               const orbg_sim3d *corrected, const orbg_sim3d *noncorrected,
                               const int32_t *set, int set_cap, const int32_t *nset,
                               const int32_t *pairs, int pair_cap, const int32_t *npairs,
                               int32_t *vert_slot, int32_t *nvert, int32_t *fixed, orbg_sim3d *Scw,
                               orbg_sim3d *Snc, orbg_eg_edge *edges, int edge_cap, int32_t *nedge,
                               int32_t *status);
// :1264-1323: SetPose per vertex, ref[p] and the gathered positions (pts [P][3], ref [P])
int launch_map_apply_poses(hipStream_t st, const MapDev &M, int cur, const int32_t *vert_slot,
                           const int32_t *nvert, const float *Tiw, float *pts, int32_t *ref);
int launch_map_set_corrected(hipStream_t st, const MapDev &M, int first, int n, const int32_t *by,
                             const int32_t *ref);
int launch_map_scatter_points(hipStream_t st, const MapDev &M, const float *pts, const int32_t *ref);

// map_lba_kernels.hip: Optimizer::LocalBundleAdjustment's window and write-back
// (src/Optimizer.cc:635-851, 943-978).  The map-owned marks of one call:
#define ORBG_LBA_MAX_POINTS 0x7FFFE   // a window position is 19 bits of the fixed cameras' sort key
struct MapLbaWs {
    int32_t pcap;                     // entries of eoff / ids
    int32_t *hdr;                     // [16] LBA_HDR_*
    int32_t *lrank;                   // [K] rank among the local keyframes, -1 none, -2 local but bad
    int32_t *ffirst;                  // [K] least window position of a local point the slot observes
    int32_t *pidx;                    // [K] slot -> pose index, -1 = no vertex
    int32_t *lslot;                   // [K] pose index -> slot
    int32_t *fixed;                   // [K] pose index -> the vertex is fixed
    int32_t *cnt;                     // [K + 1] points first listed per local keyframe, then offsets
    int32_t *eoff;                    // [pcap + 1] edges per window point, then their offsets
    int32_t *ids;                     // [pcap] Apply: the window's points, -1 behind them
};
#define LBA_HDR_NLOCAL 0
#define LBA_HDR_NPOSE 1
#define LBA_HDR_NPOINT 2
#define LBA_HDR_NEDGE 3
#define LBA_HDR_BITS 4                // ORBG_LBA_*
#define LBA_HDR_NERASED 8             // Apply
#define LBA_HDR_NBAD 9
struct MapLbaWindow {
    int32_t *kf_slots;                // [pose_cap]
    orbg_pose *poses;                 // [pose_cap]
    int32_t *point_ids;               // [point_cap]
    double *points;                   // [point_cap][3]
    orbg_edge *edges;                 // [edge_cap]
    int32_t *edge_feat;               // [edge_cap]
    int32_t pose_cap, point_cap, edge_cap;
    int32_t *counts;                  // [4] nlocal, npose, npoint, nedge
};
struct MapLbaConst {
    float inv_sigma2[16];             // mvInvLevelSigma2
    double huber_mono, huber_stereo;  // (float)sqrt(5.991), (float)sqrt(7.815)
};
// status [4]: [0] = ORBG_LBA_* bits
int launch_map_lba_window(hipStream_t st, const MapDev &M, const MapAttach &A, const MapLbaWs &W,
                          int slot, const MapLbaWindow &O, const MapLbaConst &C, int32_t *status,
                          Prof *prof);
// out [2]: erased observations, points gone bad; cams_out may be NULL
int launch_map_lba_apply(hipStream_t st, const MapDev &M, const MapLbaWs &W, const MapLbaWindow &O,
                         const uint8_t *erase, orbg_frustum_camera *cams_out, int32_t *out,
                         Prof *prof);

// map_gba_kernels.hip: Optimizer::GlobalBundleAdjustemnt's window and store (src/Optimizer.cc:
// 113-320) and RunGlobalBundleAdjustment's map update (src/LoopClosing.cc:1056-1116).  The
// map-owned marks of one call, sized by K and P alone:
struct MapGbaWs {
    int32_t *hdr;                     // [16] GBA_HDR_*
    int32_t *pidx;                    // [K] slot -> pose index, -1 = no vertex
    int32_t *fixed;                   // [K] pose index -> the vertex is fixed
    int32_t *ne;                      // [P] edges of the point, 0 = not in the window
    int32_t *pi;                      // [P] id -> window position, -1 = none
    int32_t *eoff;                    // [P] id -> its first edge
    int32_t *ids;                     // [P] Store: the points written, -1 elsewhere
    int32_t *org;                     // [K] Update: 1 = an origin
    int32_t *vis;                     // [K] Update: 0 not visited, else 1 + parents up to the nearest slot in the BA
    float *gT;                        // [K][12] Update: the propagated mTcwGBA, staged
};
#define GBA_HDR_NPOSE 0
#define GBA_HDR_NPOINT 1
#define GBA_HDR_NEDGE 2
#define GBA_HDR_LEFT 3                // good points without an edge (vbNotIncludedMP)
#define GBA_HDR_BITS 4                // ORBG_LBA_*
// O.counts [4]: npose, npoint, nedge, points left out; status [4]: [0] = ORBG_LBA_* bits
int launch_map_gba_window(hipStream_t st, const MapDev &M, const MapAttach &A, const MapGbaWs &W,
                          int robust, const MapLbaWindow &O, const MapLbaConst &C, int32_t *status,
                          Prof *prof);
// counts as the window left them; out [2] (zeroed by the caller): keyframes, points written
int launch_map_gba_store(hipStream_t st, const MapDev &M, const MapGbaWs &W, const int32_t *counts,
                         const int32_t *kf_slots, int pose_cap, const int32_t *point_ids,
                         int point_cap, const orbg_pose *poses, const double *points, int loop_kf,
                         orbg_frustum_camera *cams_out, int32_t *out, Prof *prof);
// out [6] and status [4] zeroed by the caller; status [0] = ORBG_GBA_* bits
int launch_map_gba_update(hipStream_t st, const MapDev &M, const MapGbaWs &W, const int32_t *origins,
                          int norigins, int loop_kf, orbg_frustum_camera *cams_out, int32_t *out,
                          int32_t *status, Prof *prof);

// map_create_kernels.hip: LocalMapping::CreateNewMapPoints and ProcessNewKeyFrame on the table.
// The attached geometry (orbg_map_attach_keyframe_geometry, not owned) and the map-owned
// workspace of one call; acap = the attached row length, cap = the Map's.
#define ORBG_CNP_MAX_NEIGH 20         // GetBestCovisibilityKeyFrames(20), monocular
struct MapGeom {
    const orbg_keypoint *kps_raw;     // [K][acap] mvKeys, NULL: mvKeysUn
    const float *depth;               // [K][acap] mvDepth
    const orbg_kf_camera *cams;       // [K] fx .. mbf read
};
struct MapCreateWs {
    int32_t acap;
    int32_t *hdr;                     // [16] CNP_HDR_*
    int32_t *kf1, *kf2;               // [20] the pair launches' keyframes (skipped: the slot twice)
    int32_t *nstat;                   // [20] the neighbours' statuses
    int32_t *counts, *nfv;            // [K] N / mFeatVec size of the running pair's keyframes
    orbg_kf_camera *cams;             // [K] stored Tcw + attached intrinsics, current and neighbours
    uint8_t *has_mp;                  // [K][acap] row[idx] >= 0 of the running pair's keyframes
    orbg_triangulation_pair *geo;     // [20]
    int32_t *match;                   // [acap] the running pair's vMatches12
    int32_t *nm;                      // [1]
    float *x3d;                       // [acap][3]
    int8_t *tst;                      // [acap] ORBG_TRI_*
    int32_t *nnew;                    // [1]
    uint8_t *virt;                    // [acap] the current keyframe's features whose point a cap left out
    int32_t *ids;                     // [cap + 1] the points to update, -1 padded, their count behind
    int32_t *row;                     // [cap] ProcessNewKeyFrame: the row as it is stored
    float *centre;                    // [3] its camera centre
};
#define CNP_HDR_NN 0                  // neighbours taken from the list
#define CNP_HDR_NNEW 1                // points created so far
#define CNP_HDR_NEED 2                // points a large enough cap would have created
#define CNP_HDR_BITS 3                // ORBG_CNP_*
#define CNP_HDR_ABORT 4               // the latched d_abort
#define CNP_HDR_REC0 5                // d_nrecent[0] when the call started
#define CNP_HDR_SLOT 8                // ProcessNewKeyFrame: slot, N, kf flags, mnId
#define CNP_HDR_N 9
#define CNP_HDR_FLAGS 10
#define CNP_HDR_MNID 11
// the neighbours, their statuses (baseline / median depth, one workgroup each) and cameras
int launch_map_cnp_neighbours(hipStream_t st, const MapDev &M, const MapAttach &A, const MapGeom &G,
                              const MapCreateWs &W, int slot, int monocular, const int32_t *nrecent,
                              int32_t *neigh);
// before pair i's search: the abort latch, N / nfv and has_mp of both keyframes from the rows
int launch_map_cnp_pair(hipStream_t st, const MapDev &M, const MapAttach &A, const MapCreateWs &W,
                        int slot, int i, const int32_t *abort);
// after pair i's triangulation: ids by an in-order scan, records, both rows, recent
int launch_map_cnp_insert(hipStream_t st, const MapDev &M, const MapCreateWs &W, int slot, int i,
                          int current_kf_id, int first_id, int32_t *recent, int recent_cap,
                          int32_t *nrecent, int32_t *nmatches, int32_t *nnew, int8_t *tri_status);
int launch_map_cnp_finish(hipStream_t st, const MapDev &M, const MapCreateWs &W, int first_id,
                          int32_t *neigh_status, int32_t *out);
// ProcessNewKeyFrame: the row with bad / out-of-range ids as -1, the centre, recent and W.ids
int launch_map_pnk_prepare(hipStream_t st, const MapDev &M, const MapCreateWs &W, int slot,
                           const int32_t *point_ids, int n, const float *Tcw, int mnid, int flags,
                           const uint8_t *in_keyframe, int32_t *recent, int recent_cap,
                           int32_t *nrecent, int32_t *out);

}  // namespace orbg
