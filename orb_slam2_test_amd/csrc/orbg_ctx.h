// orbg_ctx.h -- host-only internals shared by the host files (orbg_api.hip, api_*.hip): the
// context, errors, profiling, the environment-knob reader and the buffer helpers.  Not for
// kernel files (they see orbg_launch.h only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cfloat>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <array>
#include <map>
#include <vector>

#include "orbg_launch.h"
#include "bow_args.h"

// ---------------------------------------------------------------------------
// errors: one thread_local message (orbg_api.hip), set by set_err and read by
// orbg_last_error
// ---------------------------------------------------------------------------
namespace orbg {
int set_err(int code, const char *fmt, ...);
}
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess)                                                              \
            return set_err(ORBG_EIO, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_),   \
                           __FILE__, __LINE__);                                            \
    } while (0)

// ---------------------------------------------------------------------------
// profiling: HIP events around every launch on the context stream
// ---------------------------------------------------------------------------
namespace orbg {
struct ProfKind {
    const char *name;
    double total_ms = 0;
    int64_t launches = 0;
};
struct Prof {
    bool on = false;
    std::vector<ProfKind> kinds;
    struct Pending {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        hipEventCreate(&e);
        return e;
    }
    int kind(const char *n)
    {
        for (size_t i = 0; i < kinds.size(); i++)
            if (!strcmp(kinds[i].name, n)) return (int)i;
        kinds.push_back(ProfKind{n});
        return (int)kinds.size() - 1;
    }
    void begin(hipStream_t s, const char *n, hipEvent_t *a)
    {
        if (!on) return;
        *a = get();
        hipEventRecord(*a, s);
        (void)n;
    }
    void end(hipStream_t s, const char *n, hipEvent_t a)
    {
        if (!on) return;
        hipEvent_t b = get();
        hipEventRecord(b, s);
        pending.push_back(Pending{kind(n), a, b});
    }
    void collect()
    {
        for (auto &p : pending) {
            hipEventSynchronize(p.b);
            float ms = 0;
            hipEventElapsedTime(&ms, p.a, p.b);
            kinds[p.kind].total_ms += ms;
            kinds[p.kind].launches++;
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
};
}  // namespace orbg

// Developer what-if knob ORBG_SKIP=<names> (developer builds only, `make DEV=1` defines
// ORBG_DEV_KNOBS): launches whose profile name is listed are not issued (their consumers
// read the previous batch's buffers), so a bench run shows what a kernel costs inside the
// overlapped pipeline.  Wrong results: a production build compiles it out and orbg_create
// warns when the variable is set.
namespace orbg {
#ifdef ORBG_DEV_KNOBS
extern std::atomic<int> g_extract_batches;  // batches issued, all contexts (ORBG_SKIP_AFTER)
bool prof_skip(const char *name);
#else
inline bool prof_skip(const char *) { return false; }
#endif
}  // namespace orbg
// events on `st`, the stream the kernel is launched on (a local in every caller)
#define PROF_LAUNCH(ctxp, name, ...)                                                       \
    do {                                                                                   \
        if (prof_skip(name)) break;                                                        \
        hipEvent_t ev_a_ = nullptr;                                                        \
        (ctxp)->prof.begin(st, name, &ev_a_);                                              \
        __VA_ARGS__;                                                                       \
        (ctxp)->prof.end(st, name, ev_a_);                                                 \
    } while (0)

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct orbg_ctx {
    int device = 0;
    orbg_params p{};
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    // second stream for independent work inside one call (blur beside FAST+quadtree, knn2
    // beside SearchForInitialization); forked from / joined into `stream` with events
    hipStream_t aux_stream = nullptr;
    // quadtree stream (high priority, its own hardware queue): the quadtree runs beside the
    // GaussianBlur, fork after the FAST cells (ev_fast), join before k_octree (ev_oct).
    // oct_mode 0: everything on the extraction stream, 1: level 0 only, 2: all levels.
    hipStream_t ostream = nullptr;
    hipEvent_t ev_fast = nullptr, ev_oct = nullptr;
    // pipelined front, level 0 (FAST cells + GaussianBlur need only the input images) on
    // `fstream` beside the pyramid (ORBG_SIDE: 0 off, 1 normal priority, 2 high)
    hipStream_t fstream = nullptr;
    int side_mode = 1;
    hipEvent_t ev_f0[2] = {nullptr, nullptr}, ev_b0[2] = {nullptr, nullptr},
               ev_pfork[2] = {nullptr, nullptr}, ev_pyr[2] = {nullptr, nullptr};
    bool blur_side = false;  // ORBG_BLUR_SIDE
    // non-pipelined batches (the single-frame drop-in): k_octree, the fallback quadtree for
    // levels past k_octree_lds' capacity, on `fstream` beside the k_octree_lds launches once
    // every level's FAST cells are written (ev_big_a: level 0 on the quadtree stream, ev_big_b:
    // levels 1.. on the extraction stream), joined before k_orient_desc (ev_big); it only scans
    // the cell counts unless a level overflows.  ORBG_BIG_SIDE=1 (off by default: the single
    // frame measured 0.26 -> 0.32-0.36 ms, the level-1.. FAST launch 15 -> 51 us behind the
    // extra stream's waits, profiles/r05q_single_ab.txt)
    bool big_side = false;
    hipEvent_t ev_big_a = nullptr, ev_big_b = nullptr, ev_big = nullptr;
    // small batches: the side blur on `fstream` right behind k_pyramid (ORBG_BLUR_Q3), joined
    // before k_orient_desc
    bool blur_q3 = false;
    bool sblur = true;  // ORBG_SBLUR=0: small batches blur on the extraction stream (A/B)
    hipEvent_t ev_sblur = nullptr;
    // ORBG_OCT_GATE (read at orbg_create, default 1): the quadtree fallback launches of a
    // pipelined batch (the split level-0 pair's second launch, k_octree) exit at once unless an
    // earlier launch of the batch flagged a level for them (d_err[3], d_err[2]); 0 = they
    // always scan (A/B, and the parity test's ungated twin)
    bool oct_gate = true;
    bool fast_blur_env = false;  // ORBG_FAST_BLUR (read at orbg_create): the fused blur plan
    bool blur_tiled_env = true;  // ORBG_BLUR_TILED (read at orbg_create; 0: row-major blur)
    bool serial = false;     // orbg_set_serial: no stream overlap (isolated kernel timing)
    // orbg_extract's single-frame hipGraphs: the whole frame (H2D of the pinned input, the
    // extraction's launches on the context and quadtree streams, k_pack_frame, D2H of the
    // packed outputs) captured once per output slot and image size, then replayed with one
    // hipGraphLaunch.  ORBG_GRAPH=1|2|3 (graph_mode below); 0, the default, launches eagerly.
    int graph_mode = 0;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};
    uint64_t gkey[2] = {0, 0};   // (plan generation, w, h) the graph was captured for
    int gwarm[2] = {0, 0};       // eager frames seen for gkey_next (capture after one)
    uint64_t gkey_seen[2] = {0, 0};
    uint64_t plan_gen = 0;
    uint8_t *h_gin = nullptr, *h_gout = nullptr;  // pinned graph input / output
    size_t gin_bytes = 0, gout_bytes = 0;
    bool ba_jacobians = true;  // orbg_ba_set_jacobians
    bool ba_edge_errors = true;  // orbg_ba_set_edge_errors
    int oct_mode = 0;
    int blur0_mode = 0;  // measured: 2.013 vs 2.025 ms per 256 frames with it on
    int fast0_mode = 1;  // level-0 FAST cells on `ostream` beside the resize chain (ORBG_FAST0)
    // Pipelined batches (orbg_set_pipeline): the front of a batch (pyramid, FAST cells,
    // GaussianBlur: image work) runs on `stream`, its back (quadtree, orientation +
    // descriptors, stereo: keypoint work) on `ostream`, so the front of batch k+1 overlaps
    // the back of batch k.  The per-batch intermediates (pyramid, blur, FAST cells) alternate
    // between two slots with the outputs: ev_cells[s] / ev_front[s] = slot s's FAST cells /
    // whole front written (on `stream`), ev_back[s] = slot s's last back reader done (on
    // `ostream`); the front into slot s waits for ev_back[s].
    int pipelined = 0;
    bool last_piped = false;  // the last batch took the pipelined path (back_stream)
    // stereo summary (orbg_stereo_summary) on the match stream: ev_sback = stereo outputs
    // written (back stream), ev_ssum = the summary's reads done (match stream; the next
    // stereo batch waits for it before overwriting d_snvalid / d_spairs)
    hipEvent_t ev_sback = nullptr, ev_ssum = nullptr;
    bool ssum_pending = false;
    // caller reads of the outputs (orbg_batch_acquire / orbg_batch_release): ev_rel[s] = the
    // caller's reads of output slot s issued so far, ev_srel = of the stereo outputs; the
    // slot's next extraction / the next stereo pass waits for them
    hipEvent_t ev_rel[2] = {nullptr, nullptr}, ev_srel = nullptr;
    bool rel_pending[2] = {false, false}, srel_pending = false;
    // entry points that write caller buffers on `mstream` (orbg_batch_summary /
    // orbg_batch_matches / orbg_match_pose_batch_device / orbg_stereo_summary) first order
    // `mstream` after the work queued on the context stream so far (ev_caller): a fill the
    // caller queued there before the call can never land after liborbg's write
    hipEvent_t ev_caller = nullptr;
    hipEvent_t ev_cells[2] = {nullptr, nullptr}, ev_front[2] = {nullptr, nullptr};
    hipEvent_t ev_back[2] = {nullptr, nullptr};
    bool back_pending[2] = {false, false};
    hipEvent_t ev_fork[2] = {nullptr, nullptr}, ev_join[2] = {nullptr, nullptr};
    // Batch matching and the trajectory summary run on `mstream`, so the matching of batch k
    // overlaps the extraction of batch k+1 on `stream`.  The per-frame outputs (kps, desc,
    // counts) alternate between two slots: ev_ext[s] = slot s written (on `stream`),
    // ev_mat[s] = slot s no longer read (on `mstream`); extraction into slot s waits for
    // ev_mat[s], matching of slot s waits for ev_ext[s].
    hipStream_t mstream = nullptr;
    hipEvent_t ev_ext[2] = {nullptr, nullptr}, ev_mat[2] = {nullptr, nullptr};
    bool mat_pending[2] = {false, false};
    int slot = 0;  // slot of the last extraction
    float scale[16], inv_scale[16], sigma2[16], inv_sigma2[16];
    int32_t fpl[16], umax[16];
    // plan
    int gw = 0, gh = 0, gbatch = 0;
    OrbgGeom geom{};
    std::vector<OrbgCell> cells;
    std::vector<int32_t> tile_base;  // k_blur2 tile bases (L + 1)
    // k_fast_rows strips (fast_rows_kernels.hip): fr_ok = every level's cells fit a strip
    // (wCell <= 32); ftile_base[l] = first strip of level l (L + 1 entries); fr_mode 0 forces
    // k_fast2 (ORBG_FAST_ROWS=0, developer A/B)
    OrbgFastTile *d_ftiles = nullptr;
    std::vector<int32_t> ftile_base;
    bool fr_ok = false;
    int fr_mode = 0;  // k_fast_rows opt-in (ORBG_FAST_ROWS=1) until it beats k_fast2
    OctLdsDims oct_dims[3] = {};  // levels 0, 1.., and level 0's batch first launch (kcap 0: none)
    // device
    OrbgGeom *d_geom = nullptr;
    OrbgCell *d_cells = nullptr;
    int32_t *d_tile_base = nullptr;
    int2 *d_rtab = nullptr;
    // k_pyramid (all levels in one launch): octet / row records and band closures; pyr_ok
    // = the plan passed k_pyramid's checks (else the k_resize chain)
    uint4 *d_ptab = nullptr;
    int4 *d_ytab4 = nullptr;
    int4 *d_bands = nullptr;
    PyrArgs pyr_args{};
    bool pyr_ok = false;
    int pyr_wg = 512;  // k_pyramid workgroup size (ORBG_PYR_WG)
    uint32_t *d_ctab = nullptr;  // quadtree path-code tables (xs | ys per level)
    uint4 *d_odtab = nullptr;    // k_orient_desc IC_Angle byte tables (make_od_tab)
    uint8_t *d_img = nullptr;
    size_t img_bytes = 0;
    uint8_t *d_pack = nullptr;  // orbg_download_frame: error word, count, kps, desc
    size_t pack_bytes = 0;
    // zero-copy host block (coherent pinned, device-mapped; ORBG_ZC, default 1): k_pack_frame
    // stores orbg_download_frame's packed outputs straight into it, and the
    // SearchForInitialization host entry's inputs are read from it by one copy kernel and its
    // outputs written into it by the resolver -- kernels instead of DMA submissions, whose
    // start latency (6-9 us each) the single-frame path otherwise waits for
    uint8_t *h_zc = nullptr, *h_zc_dev = nullptr;
    size_t zc_bytes = 0;
    // orbg_extract's image in coherent host memory, pulled by k_copy16 (ORBG_IMG_PULL)
    uint8_t *h_imz = nullptr, *h_imz_dev = nullptr;
    size_t imz_bytes = 0;
    int zc_mode = -1;  // -1: read ORBG_ZC on first use
    // orbg_extract's zero-copy outputs written by k_orient_desc itself (the packed block's
    // device pointer while launch_extract runs; null otherwise)
    uint8_t *hc_dst = nullptr;
    bool hc_done = false;  // the last extraction's frame 0 is already in the packed block
    // with hc_dst: k_octree (the fallback quadtree) not launched; a level it would have taken
    // shows in the packed header's word 3 and the frame is extracted again with it
    bool skip_big = false;
    // the single-frame skip path's fallback tag (OctLdsDims::tag; 0 = off) and its counter
    int32_t oct_tag = 0;
    int32_t sf_seq = 0;
    uint8_t *d_pyr = nullptr, *d_blur = nullptr;  // = pyr_slot[slot], blur_slot[slot]
    int32_t *d_cell_cnt = nullptr;                 // = cnt_slot[slot]
    uint2 *d_cell_kp = nullptr;                    // = ckp_slot[slot]
    uint8_t *pyr_slot[2] = {nullptr, nullptr}, *blur_slot[2] = {nullptr, nullptr};
    int32_t *cnt_slot[2] = {nullptr, nullptr};
    uint2 *ckp_slot[2] = {nullptr, nullptr};
    uint32_t *d_keys = nullptr, *d_knode = nullptr, *d_act = nullptr;
    uint8_t *d_qk = nullptr;
    int4 *d_nodes = nullptr;
    uint32_t *d_lvl_kp = nullptr;
    uint16_t *d_lvl_idx = nullptr;  // slot -> winner list position (octree -> orient)
    int32_t *d_lvl_cnt = nullptr;
    orbg_keypoint *d_kps = nullptr;  // = kps_slot[slot]
    uint8_t *d_desc = nullptr;        // = desc_slot[slot]
    int32_t *d_counts = nullptr;      // = counts_slot[slot]
    orbg_keypoint *kps_slot[2] = {nullptr, nullptr};
    uint8_t *desc_slot[2] = {nullptr, nullptr};
    int32_t *counts_slot[2] = {nullptr, nullptr};
    int32_t *d_err = nullptr;
    // last batch
    const uint8_t *last_img = nullptr;
    int64_t last_fs = 0;
    int last_pitch = 0;
    int last_n = 0;
    // matching (batch)
    int32_t *d_pairs = nullptr;
    int pair_cap = 0;
    std::vector<int32_t> h_pairs;  // last uploaded (f1, f2) lists
    int32_t *d_knn = nullptr, *d_m12 = nullptr, *d_nm = nullptr;
    uint32_t *d_topk = nullptr;
    int32_t *d_topk_n = nullptr;
    int last_npairs = 0;
    // stereo (ComputeStereoMatches) of the last batch
    int32_t *d_spairs = nullptr;
    std::vector<int32_t> h_spairs;  // last uploaded (left, right) lists
    float *d_uright = nullptr, *d_depth = nullptr;
    int32_t *d_snvalid = nullptr;
    void *d_sscr = nullptr;
    int stereo_cap = 0, last_nstereo = 0;
    // single-pair / host-data scratch
    void *d_scr = nullptr;
    size_t scr_bytes = 0;
    // pinned host staging of the host-data entry points (orbg_extract, orbg_download_frame,
    // orbg_search_for_initialization): one DMA per direction instead of pageable copies
    uint8_t *h_stage = nullptr;
    size_t stage_bytes = 0;
    // tracking matchers: K-lists of the queries
    void *d_trk = nullptr;
    size_t trk_bytes = 0;
    void *d_sim3 = nullptr;  // SearchBySim3's vnMatch1 / vnMatch2 scratch
    size_t sim3_bytes = 0;
    // batched-sequence pose stub (orbg_match_pose_batch_device): edges, counts, cameras, poses
    void *d_mpose = nullptr;
    size_t mpose_bytes = 0;
    // orbg_set_camera: distorted camera of the batched-sequence mode (has_cam: k1 != 0);
    // the batch matching undistorts into d_kps_un ([kps_un_frames][frame_cap], match stream)
    bool has_cam = false;
    orbg_camera cam{};
    orbg_keypoint *d_kps_un = nullptr;
    size_t kps_un_n = 0;
    bool kps_un_valid = false;
    orbg::Prof prof;
};

// DBoW2 vocabulary handle (api_bow.hip: the vocabulary entries fill it; api_place.hip reads its
// scoring type)
struct orbg_vocab {
    int device = 0;
    int k = 0, L = 0, scoring = 0, weighting = 0, nnodes = 0, nwords = 0;
    int group = 16, root_c0 = 0, root_c1 = 0;
    orbg::BowSlot *d_slots = nullptr;
};

// ---------------------------------------------------------------------------
// internals with more than one user; each is defined once, in the file named
// ---------------------------------------------------------------------------
namespace orbg {
template <typename T>
int dalloc(T **p, size_t n)
{
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess)
        return set_err(ORBG_ENOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T),
                       hipGetErrorString(e));
    return ORBG_OK;
}
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// stream the last batch's per-frame outputs were written on (and stereo runs on): the back
// stream only if that batch actually took the pipelined path (orbg_set_serial on a
// pipelined context runs everything on the context stream)
inline hipStream_t back_stream(orbg_ctx *c) { return c->last_piped ? c->ostream : c->stream; }

// an integer environment knob: atoi of the variable, `dflt` when it is unset.  Whether a knob
// is read per process, per context or per plan is its reader's business.
inline int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// orbg_api.hip: the context's pinned stage and device scratch, grown on demand
int stage(orbg_ctx *c, size_t bytes, uint8_t **out);
int scratch(orbg_ctx *c, size_t bytes, void **p);
// orbg_api.hip: `mstream` ordered after everything queued on the context stream so far
// (ev_caller), ahead of a write to a caller's buffer on `mstream`
hipError_t order_after_caller(orbg_ctx *c);

// orbg_api.hip: orbg_local_ba_optimize's body on device-resident estimates (fixed [npose] and
// the edge records on the host, erase [nedge] out); api_map.hip runs it on the Map's window
int lba_optimize_device(orbg_ctx *c, orbg_pose *d_poses, int npose, double *d_points, int npoint,
                        const orbg_edge *edges, int nedge, const uint8_t *fixed,
                        const orbg_lm_control *control,
                        int (*point_is_bad)(void *user, int point), void *user, uint8_t *erase,
                        orbg_lba_report *rep);
// orbg_api.hip: orbg_global_ba_optimize's body on device-resident estimates (the graph, the
// sparse plan with fixed [npose], optimize(iterations)); api_map.hip runs it on the Map's window
int gba_optimize_device(orbg_ctx *c, orbg_pose *d_poses, int npose, double *d_points, int npoint,
                        const orbg_edge *edges, int nedge, const uint8_t *fixed, int iterations,
                        const orbg_lm_control *control, orbg_gba_report *rep);

// Byte layout of the buffers of an entry point on host arrays: take() hands out the offsets
// of 256-byte-aligned sub-buffers (an empty array still gets 256 bytes of its own, so it
// never aliases its neighbour), then one block of total() bytes is acquired.
struct Layout {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off += al256(bytes ? bytes : 1);
        return o;
    }
    size_t total() const { return off; }
    // a layout behind `bytes` that the caller has laid out itself
    static Layout starting_at(size_t bytes)
    {
        Layout l;
        l.off = bytes;
        return l;
    }
    template <typename T>
    static T *at(void *base, size_t o)
    {
        return (T *)((uint8_t *)base + o);
    }
    // the context scratch of total() bytes
    int device(orbg_ctx *c, uint8_t **d) const
    {
        void *p;
        int rc = scratch(c, off, &p);
        *d = (uint8_t *)p;
        return rc;
    }
    // the pinned stage of total() bytes, the context stream drained so the host may write it
    int host(orbg_ctx *c, uint8_t **h) const
    {
        int rc = stage(c, off, h);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        return ORBG_OK;
    }
};
}  // namespace orbg

