// map_loop_kernels.hip -- LoopClosing::CorrectLoop on the covisibility Map (src/LoopClosing.cc:
// 744-843 and 882-911): the state it reads beside the observation table (keyframe poses, mnId,
// loop edges, mnCorrectedByKF / mnCorrectedReference), the Sim3 propagation over the current
// keyframe's neighbours with its map-point loop, and the LoopConnections set difference.
//
//   k_loop_set_poses   KeyFrame::SetPose per entry: Tcw, and Ow = -Rcw^T tcw as the float
//                      cv::Mat product (double sums, one rounding) into kf_centre.
//   k_loop_set         mvpCurrentConnectedKFs = cur's ordered list + cur, the membership table
//                      lp_pos, the checks (cur live, set_cap, every member has a pose).
//   k_loop_sim3        one thread per member: NonCorrectedSim3 = Sim3(Riw, tiw, 1),
//                      CorrectedSim3 = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc the float
//                      product, and the corrected pose [R | t / s] with its centre, staged in
//                      lp_T / lp_c (the poses themselves are still read).
//   k_loop_points      one workgroup per member, one lane per row entry.  The reference walks
//                      CorrectedSim3 in slot order, so a point is corrected by the lowest member
//                      slot that holds it: the lane whose slot is the first member among the
//                      point's (ascending-slot) observations moves it, writes the two
//                      mnCorrected* fields and runs UpdateNormalAndDepth, where a member below
//                      the owner contributes its corrected centre (its SetPose has run by
//                      then) and every other observer its old one.
//   k_loop_apply       SetPose of every member from the staged poses.
//   k_lc_*             LoopConnections, member by member in vector order: snapshot of the
//                      ordered list, the UpdateConnections launch of map_kernels.hip, then the
//                      non-zeros of the W row minus the snapshot minus the set in ascending
//                      slot order (ordered compaction); k_lc_emit writes the groups in
//                      ascending member slot.
// No result depends on thread order: no atomics on results, one writer per point.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "sim3opt_args.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

__device__ __forceinline__ void loop_sim3_of_pose(const float *T, Sim3d *S)
{
    double R[3][3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = (double)T[r * 4 + c];
        S->t[r] = (double)T[r * 4 + 3];
    }
    q_from_rot(R, S->q);
    S->s = 1.0;
}

__global__ void k_loop_defaults(MapDev M)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < M.K) M.kf_mnid[s] = s;
}

__global__ void k_loop_set_poses(MapDev M, const int32_t *slots, int n, const float *Tcw,
                                 const int32_t *mnid)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s < 0 || s >= M.K) return;
    if (Tcw) {
        float T[12];
        for (int k = 0; k < 12; k++) T[k] = Tcw[(size_t)i * 12 + k];
        for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = T[k];
        loop_centre(T, M.kf_centre + s * 3);
        M.kf_pose[s] = 1;
    }
    if (mnid) M.kf_mnid[s] = mnid[i];
}

// status: 0 added (or already there), 1 a side is full: nothing changes
__global__ void k_loop_add_edge(MapDev M, int a, int b, int32_t *status)
{
    const int e[2][2] = {{a, b}, {b, a}};
    bool have[2];
    for (int k = 0; k < 2; k++) {
        have[k] = false;
        const int n = M.le_n[e[k][0]];
        for (int i = 0; i < n; i++) have[k] |= M.le_slot[e[k][0] * ORBG_MAP_MAX_LOOP_EDGES + i] == e[k][1];
        if (!have[k] && n >= ORBG_MAP_MAX_LOOP_EDGES) {
            *status = 1;
            return;
        }
    }
    for (int k = 0; k < 2; k++)
        if (!have[k]) M.le_slot[e[k][0] * ORBG_MAP_MAX_LOOP_EDGES + M.le_n[e[k][0]]++] = e[k][1];
    *status = 0;
}

__global__ void k_loop_hdr(MapDev M, int cur)
{
    M.lp_hdr[LOOP_HDR_SLOT] = cur;
    M.lp_hdr[LOOP_HDR_NSET] = 0;
}

__global__ __launch_bounds__(MAP_T) void k_loop_set(MapDev M, int cur, int32_t *set, int set_cap,
                                                    int32_t *nset, int32_t *status)
{
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) M.lp_pos[t] = -1;
    __syncthreads();
    const bool live = (M.kf_flags[cur] & MAP_KF_LIVE) != 0;
    const int n = live ? M.nord[cur] + 1 : 0;
    const uint16_t *os = M.ord_slot + (size_t)cur * M.K;
    int st = live ? 0 : ORBG_LOOP_DEAD;
    if (n > set_cap) st |= ORBG_LOOP_SET_RANGE;
    if (!st)
        for (int i = threadIdx.x; i < n; i += MAP_T) {
            const int s = i < n - 1 ? (int)os[i] : cur;
            if (!M.kf_pose[s]) bad = 1;  // every writer stores 1
        }
    __syncthreads();
    if (bad) st |= ORBG_LOOP_NO_POSE;
    const int na = st ? 0 : n;
    for (int i = threadIdx.x; i < set_cap; i += MAP_T) {
        const int s = i < na ? (i < n - 1 ? (int)os[i] : cur) : -1;
        set[i] = s;
        if (s >= 0) M.lp_pos[s] = i;
    }
    if (threadIdx.x == 0) {
        M.lp_hdr[LOOP_HDR_NSET] = na;
        *nset = na;
        status[0] = st;
        status[1] = n;
    }
}

__global__ __launch_bounds__(64) void k_loop_sim3(MapDev M, int cur, const orbg_sim3d *scw,
                                                  const int32_t *set, orbg_sim3d *corrected,
                                                  orbg_sim3d *noncorrected)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M.lp_hdr[LOOP_HDR_NSET]) return;
    const int s = set[i];
    const float *Tiw = M.kf_Tcw + (size_t)s * 12;
    Sim3d Scw, nc, corr;
    for (int k = 0; k < 4; k++) Scw.q[k] = scw->q[k];
    for (int k = 0; k < 3; k++) Scw.t[k] = scw->t[k];
    Scw.s = scw->s;
    loop_sim3_of_pose(Tiw, &nc);
    if (s != cur) {
        const float *Tc = M.kf_Tcw + (size_t)cur * 12;
        float Ow[3], Tic[12];
        loop_centre(Tc, Ow);  // Twc = [Rcw^T | Ow]
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 4; c++) {  // Tic = Tiw * Twc: the sums over all four terms
                double a = 0.0;
                for (int k = 0; k < 3; k++)
                    a += (double)Tiw[r * 4 + k] * (double)(c < 3 ? Tc[c * 4 + k] : Ow[k]);
                a += (double)Tiw[r * 4 + 3] * (c < 3 ? 0.0 : 1.0);
                Tic[r * 4 + c] = (float)a;
            }
        }
        Sim3d Sic;
        loop_sim3_of_pose(Tic, &Sic);
        so_mul(Sic, Scw, &corr);
    } else {
        corr = Scw;
    }
    orbg_sim3d o;
    for (int k = 0; k < 4; k++) o.q[k] = corr.q[k];
    for (int k = 0; k < 3; k++) o.t[k] = corr.t[k];
    o.s = corr.s;
    corrected[s] = o;
    for (int k = 0; k < 4; k++) o.q[k] = nc.q[k];
    for (int k = 0; k < 3; k++) o.t[k] = nc.t[k];
    o.s = nc.s;
    noncorrected[s] = o;
    // correctedTiw = [R | t * (1 / s)]
    double R[3][3];
    q_to_rot(corr.q, R);
    const double inv = 1. / corr.s;
    float *T = M.lp_T + (size_t)s * 12;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r][c];
        T[r * 4 + 3] = (float)(corr.t[r] * inv);
    }
    loop_centre(T, M.lp_c + s * 3);
}

__global__ __launch_bounds__(MAP_T) void k_loop_points(MapDev M, int cur, const int32_t *set,
                                                       const orbg_sim3d *corrected,
                                                       const orbg_sim3d *noncorrected, MapScales S)
{
    if ((int)blockIdx.x >= M.lp_hdr[LOOP_HDR_NSET]) return;
    const int s = set[blockIdx.x];
    const int curid = M.kf_mnid[cur], sid = M.kf_mnid[s];
    Sim3d Siw, Sc, Swi;
    for (int k = 0; k < 4; k++) {
        Siw.q[k] = noncorrected[s].q[k];
        Sc.q[k] = corrected[s].q[k];
    }
    for (int k = 0; k < 3; k++) {
        Siw.t[k] = noncorrected[s].t[k];
        Sc.t[k] = corrected[s].t[k];
    }
    Siw.s = noncorrected[s].s;
    Sc.s = corrected[s].s;
    so_inverse(Sc, &Swi);
    const int n = min(M.kf_n[s], M.cap);
    for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
        const int p = M.kf_points[(size_t)s * M.cap + idx];
        if (!map_point_ok(M, p)) continue;
        const int e0 = M.obs_off[p], e1 = M.obs_off[p + 1];
        int owner = -1;
        for (int e = e0; e < e1 && owner < 0; e++) {
            const int t = (int)(M.obs[e] >> 16);
            if (M.lp_pos[t] >= 0) owner = t;
        }
        if (owner != s) continue;                 // a lower member corrects it
        if (M.mp_corr_kf[p] == curid) continue;   // only this lane writes it
        orbg_map_point r = M.mp[p];
        const double x[3] = {(double)r.x, (double)r.y, (double)r.z};
        double y[3], z[3];
        so_map(Siw, x, y);
        so_map(Swi, y, z);
        r.x = (float)z[0];
        r.y = (float)z[1];
        r.z = (float)z[2];
        M.mp_corr_kf[p] = curid;
        M.mp_corr_ref[p] = sid;
        M.mp_corr_slot[p] = s;
        // UpdateNormalAndDepth as k_map_normal_depth states it, the members below s moved
        const int ref = M.mp_ref[p];
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, dist = 0.0f;
        int ridx = -1;
        for (int e = e0; e < e1; e++) {
            const uint32_t ob = M.obs[e];
            const int t = (int)(ob >> 16);
            // the reference's rule (a member below the owner has had its SetPose).  On this table
            // the owner is the lowest observing member, so the first branch is never taken; it
            // states the rule and costs one compare
            const float *O = (M.lp_pos[t] >= 0 && t < s ? M.lp_c : M.kf_centre) + t * 3;
            const float dx = r.x - O[0], dy = r.y - O[1], dz = r.z - O[2];
            double sq = (double)dx * (double)dx;
            sq += (double)dy * (double)dy;
            sq += (double)dz * (double)dz;
            const double nrm = sqrt(sq);
            const float a = (float)(1.0 / nrm);
            nx = nx + dx * a;
            ny = ny + dy * a;
            nz = nz + dz * a;
            if (t == ref) {
                ridx = (int)(ob & 0xFFFFu);
                dist = (float)nrm;
            }
        }
        if (ridx >= 0) {
            const int level = min((int)M.kf_oct[(size_t)ref * M.cap + ridx], 15);
            const float maxd = dist * S.scale[level];
            const float inv = (float)(1.0 / (double)(e1 - e0));
            r.nx = nx * inv;
            r.ny = ny * inv;
            r.nz = nz * inv;
            r.max_dist = maxd;
            r.min_dist = maxd / S.scale[S.nlevels - 1];
        }
        M.mp[p] = r;
    }
}

__global__ __launch_bounds__(64) void k_loop_apply(MapDev M, const int32_t *set)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M.lp_hdr[LOOP_HDR_NSET]) return;
    const int s = set[i];
    for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = M.lp_T[(size_t)s * 12 + k];
    for (int k = 0; k < 3; k++) M.kf_centre[s * 3 + k] = M.lp_c[s * 3 + k];
}

// ---------------------------------------------------------------------------
// LoopConnections
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_lc_begin(MapDev M, const int32_t *set, int set_cap,
                                                    const int32_t *nset, int32_t *cnt)
{
    for (int t = threadIdx.x; t < M.K; t += MAP_T) M.lp_pos[t] = -1;
    __syncthreads();
    const int n = min(max(*nset, 0), set_cap);
    for (int i = threadIdx.x; i < set_cap; i += MAP_T) {
        cnt[i] = 0;
        if (i < n && set[i] >= 0 && set[i] < M.K)
            atomicMax(&M.lp_pos[set[i]], i);  // a repeated slot: its last entry
    }
    if (threadIdx.x == 0) M.lp_hdr[LOOP_HDR_NSET] = n;
}

__global__ __launch_bounds__(MAP_T) void k_lc_snapshot(MapDev M, const int32_t *set, int i)
{
    int s = i < M.lp_hdr[LOOP_HDR_NSET] ? set[i] : -1;
    if (s >= M.K) s = -1;
    const int n = s >= 0 ? M.nord[s] : 0;
    for (int k = threadIdx.x; k < n; k += MAP_T) M.lp_snap[k] = M.ord_slot[(size_t)s * M.K + k];
    if (threadIdx.x == 0) {
        M.lp_hdr[LOOP_HDR_SLOT] = s;
        M.lp_hdr[LOOP_HDR_NSNAP] = n;
    }
}

__global__ __launch_bounds__(MAP_T) void k_lc_diff(MapDev M, int i, uint16_t *rows, int32_t *cnt)
{
    __shared__ uint32_t prev[ORBG_MAP_MAX_KEYFRAMES / 32];
    __shared__ int scr[16];
    const int s = M.lp_hdr[LOOP_HDR_SLOT];
    if (s < 0) return;
    for (int k = threadIdx.x; k < ORBG_MAP_MAX_KEYFRAMES / 32; k += MAP_T) prev[k] = 0;
    __syncthreads();
    const int ns = M.lp_hdr[LOOP_HDR_NSNAP];
    for (int k = threadIdx.x; k < ns; k += MAP_T) {
        const int t = M.lp_snap[k];
        atomicOr(&prev[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    const uint16_t *w = M.W + (size_t)s * M.K;
    int c = 0;
    for (int t = t0; t < t1; t++)
        c += w[t] && !(prev[t >> 5] >> (t & 31) & 1u) && M.lp_pos[t] < 0;
    int total;
    int pos = block_scan(c, scr, &total);
    uint16_t *out = rows + (size_t)i * M.K;
    for (int t = t0; t < t1; t++)
        if (w[t] && !(prev[t >> 5] >> (t & 31) & 1u) && M.lp_pos[t] < 0) out[pos++] = (uint16_t)t;
    if (threadIdx.x == 0) cnt[i] = total;
}

// the map-of-sets' iteration order: groups in ascending member slot (at most MAP_T members)
__global__ __launch_bounds__(MAP_T) void k_lc_emit(MapDev M, const int32_t *set,
                                                   const uint16_t *rows, const int32_t *cnt,
                                                   int32_t *pairs, int pair_cap, int32_t *npairs)
{
    __shared__ int slot[MAP_T], byrank[MAP_T], off[MAP_T + 1];
    const int n = M.lp_hdr[LOOP_HDR_NSET];
    const int i = threadIdx.x;
    int mine = -1;
    if (i < n) {
        mine = set[i];
        if (mine < 0 || mine >= M.K || M.lp_pos[mine] != i) mine = -1;  // a repeated slot: its last entry
    }
    slot[i] = mine;
    __syncthreads();
    if (i < n) {
        int r = 0;
        for (int k = 0; k < n; k++) r += slot[k] < mine || (slot[k] == mine && k < i);
        byrank[r] = i;
    }
    __syncthreads();
    if (i == 0) {
        int o = 0;
        for (int r = 0; r < n; r++) {
            off[r] = o;
            o += slot[byrank[r]] < 0 ? 0 : cnt[byrank[r]];
        }
        off[n] = o;
        *npairs = o;
    }
    __syncthreads();
    for (int r = 0; r < n; r++) {
        const int m = byrank[r];
        if (slot[m] < 0) continue;
        const int c = off[r + 1] - off[r];
        for (int k = i; k < c; k += MAP_T)
            if (off[r] + k < pair_cap) {
                pairs[2 * (size_t)(off[r] + k)] = slot[m];
                pairs[2 * (size_t)(off[r] + k) + 1] = rows[(size_t)m * M.K + k];
            }
    }
}

// ---------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph's walk over the map (src/Optimizer.cc:1040-1258)
// ---------------------------------------------------------------------------
#define EG_MIN_FEAT 100  // minFeat

__device__ __forceinline__ bool eg_vertex(const MapDev &M, int s)
{
    return (M.kf_flags[s] & (MAP_KF_LIVE | ORBG_MAP_KF_BAD)) == MAP_KF_LIVE;
}

// the membership table from a set in device memory (the caller's, after Propagate)
__global__ __launch_bounds__(MAP_T) void k_eg_begin(MapDev M, const int32_t *set, int set_cap,
                                                    const int32_t *nset)
{
    for (int t = threadIdx.x; t < M.K; t += MAP_T) M.lp_pos[t] = -1;
    __syncthreads();
    const int n = min(max(*nset, 0), set_cap);
    for (int i = threadIdx.x; i < n; i += MAP_T)
        if (set[i] >= 0 && set[i] < M.K) M.lp_pos[set[i]] = i;
    if (threadIdx.x == 0) {
        M.lp_hdr[LOOP_HDR_NSET] = n;
        M.lp_hdr[LOOP_HDR_SKIP] = 0;
        M.lp_hdr[LOOP_HDR_BITS] = 0;
    }
}

// vertices: the live, not-bad slots in ascending slot order, with vScw and the
// non-corrected Sim3 per vertex
__global__ __launch_bounds__(MAP_T) void k_eg_vertices(MapDev M, int loop,
                                                       const orbg_sim3d *corrected,
                                                       const orbg_sim3d *noncorrected,
                                                       int32_t *vert_slot, int32_t *nvert,
                                                       int32_t *fixed, orbg_sim3d *Scw,
                                                       orbg_sim3d *Snc)
{
    __shared__ int scr[16];
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += eg_vertex(M, t);
    int total;
    int v = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++) {
        if (!eg_vertex(M, t)) {
            M.lp_vmap[t] = -1;
            continue;
        }
        M.lp_vmap[t] = v;
        vert_slot[v] = t;
        orbg_sim3d a;
        if (M.lp_pos[t] >= 0) {
            a = corrected[t];
            Scw[v] = a;
            Snc[v] = noncorrected[t];
        } else {
            if (!M.kf_pose[t]) M.lp_hdr[LOOP_HDR_BITS] = ORBG_LOOP_NO_POSE;  // every writer stores it
            Sim3d S;
            loop_sim3_of_pose(M.kf_Tcw + (size_t)t * 12, &S);
            for (int k = 0; k < 4; k++) a.q[k] = S.q[k];
            for (int k = 0; k < 3; k++) a.t[k] = S.t[k];
            a.s = S.s;
            Scw[v] = a;
            Snc[v] = a;
        }
        v++;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *nvert = total;
        *fixed = M.lp_vmap[loop];
        M.lp_hdr[LOOP_HDR_NVERT] = total;
    }
}

// kind 0: the LoopConnections pairs with W >= minFeat, or the (cur, loop) pair, in order
__global__ __launch_bounds__(MAP_T) void k_eg_kind0(MapDev M, int cur, int loop,
                                                    const int32_t *pairs, int pair_cap,
                                                    const int32_t *npairs, orbg_eg_edge *edges,
                                                    int edge_cap)
{
    __shared__ int scr[16];
    __shared__ int base, skipped;
    if (threadIdx.x == 0) base = skipped = 0;
    __syncthreads();
    const int n = min(max(*npairs, 0), pair_cap);
    const int idc = M.kf_mnid[cur], idl = M.kf_mnid[loop];
    for (int b0 = 0; b0 < n; b0 += MAP_T) {
        const int e = b0 + threadIdx.x;
        int keep = 0, i = -1, j = -1;
        if (e < n) {
            i = pairs[2 * e];
            j = pairs[2 * e + 1];
            if (i >= 0 && i < M.K && j >= 0 && j < M.K) {
                const bool pass = (M.kf_mnid[i] == idc && M.kf_mnid[j] == idl) ||
                                  M.W[(size_t)i * M.K + j] >= EG_MIN_FEAT;
                if (pass) {
                    if (M.lp_vmap[i] >= 0 && M.lp_vmap[j] >= 0)
                        keep = 1;
                    else
                        atomicAdd(&skipped, 1);
                }
            }
        }
        int total;
        const int pos = base + block_scan(keep, scr, &total);
        if (keep && pos < edge_cap) {
            edges[pos].i = M.lp_vmap[i];
            edges[pos].j = M.lp_vmap[j];
            edges[pos].kind = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        M.lp_hdr[LOOP_HDR_N0] = base;
        M.lp_hdr[LOOP_HDR_SKIP] = skipped;
    }
}

// the kind-1 edges of slot s (a vertex) in the reference's order: the count, written from
// out[0] on when out is not NULL (entries at or past out_cap dropped)
__device__ int eg_vertex_edges(const MapDev &M, int s, const orbg_eg_edge *e0, int n0, int e0_cap,
                               const int32_t *vert_slot, orbg_eg_edge *out, int out_cap, int *skipped)
{
    const int v = M.lp_vmap[s], ids = M.kf_mnid[s];
    int n = 0;
    auto put = [&](int t) {
        if (out && n < out_cap) {
            out[n].i = v;
            out[n].j = M.lp_vmap[t];
            out[n].kind = 1;
        }
        n++;
    };
    const int par = M.parent[s];
    if (par >= 0) {  // spanning tree edge
        if (par < M.K && M.lp_vmap[par] >= 0)
            put(par);
        else
            ++*skipped;
    }
    const int nle = min(M.le_n[s], ORBG_MAP_MAX_LOOP_EDGES);
    const int32_t *le = M.le_slot + s * ORBG_MAP_MAX_LOOP_EDGES;
    int last = -1;
    for (int k = 0; k < nle; k++) {  // a std::set<KeyFrame*>: ascending slot
        int nx = M.K;
        for (int i = 0; i < nle; i++)
            if (le[i] > last && le[i] < nx) nx = le[i];
        if (nx >= M.K) break;
        last = nx;
        if (M.kf_mnid[nx] < ids) {
            if (M.lp_vmap[nx] >= 0)
                put(nx);
            else
                ++*skipped;
        }
    }
    // GetCovisiblesByWeight(minFeat): the entries before the first weight below it; none when
    // no weight is below it (upper_bound returns end(): KeyFrame.cc:240)
    const int no = M.nord[s];
    const uint16_t *os = M.ord_slot + (size_t)s * M.K, *ow = M.ord_w + (size_t)s * M.K;
    int np = 0;
    while (np < no && ow[np] >= EG_MIN_FEAT) np++;
    if (np == no) np = 0;
    const int nk0 = min(n0, e0_cap);
    for (int k = 0; k < np; k++) {
        const int t = os[k];
        if (t == par || M.parent[t] == s) continue;  // pParentKF, hasChild
        bool isle = false;
        for (int i = 0; i < nle; i++) isle |= le[i] == t;
        if (isle) continue;
        if (M.lp_vmap[t] < 0 || !(M.kf_mnid[t] < ids)) continue;  // isBad, mnId
        const int idt = M.kf_mnid[t];
        bool ins = false;  // sInsertedEdges: (min mnId, max mnId) of the kept kind-0 edges
        for (int i = 0; i < nk0 && !ins; i++) {
            const int a = M.kf_mnid[vert_slot[e0[i].i]], b = M.kf_mnid[vert_slot[e0[i].j]];
            ins = (a == ids && b == idt) || (a == idt && b == ids);
        }
        if (!ins) put(t);
    }
    return n;
}

__global__ __launch_bounds__(MAP_T) void k_eg_count(MapDev M, const orbg_eg_edge *edges,
                                                    int edge_cap, const int32_t *vert_slot)
{
    const int s = blockIdx.x * MAP_T + threadIdx.x;
    if (s >= M.K) return;
    int skipped = 0;
    M.lp_ecnt[s] = M.lp_vmap[s] >= 0 ? eg_vertex_edges(M, s, edges, M.lp_hdr[LOOP_HDR_N0], edge_cap,
                                                       vert_slot, nullptr, 0, &skipped)
                                     : 0;
    if (skipped) atomicAdd(&M.lp_hdr[LOOP_HDR_SKIP], skipped);
}

// exclusive scan of lp_ecnt in place (one workgroup), the totals
__global__ __launch_bounds__(MAP_T) void k_eg_scan(MapDev M, int loop, int32_t *nedge,
                                                   int32_t *status)
{
    __shared__ int scr[16];
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += M.lp_ecnt[t];
    int total;
    int o = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++) {
        const int k = M.lp_ecnt[t];
        M.lp_ecnt[t] = o;
        o += k;
    }
    if (threadIdx.x == 0) {
        M.lp_ecnt[M.K] = total;
        *nedge = M.lp_hdr[LOOP_HDR_N0] + total;
        status[0] = M.lp_hdr[LOOP_HDR_BITS] | (M.lp_vmap[loop] < 0 ? ORBG_LOOP_DEAD : 0);
        status[1] = M.lp_hdr[LOOP_HDR_SKIP];
    }
}

__global__ __launch_bounds__(MAP_T) void k_eg_emit(MapDev M, orbg_eg_edge *edges, int edge_cap,
                                                   const int32_t *vert_slot)
{
    const int s = blockIdx.x * MAP_T + threadIdx.x;
    if (s >= M.K || M.lp_vmap[s] < 0) return;
    const int n0 = M.lp_hdr[LOOP_HDR_N0];
    const int at = n0 + M.lp_ecnt[s];
    if (at >= edge_cap) return;
    int skipped = 0;
    eg_vertex_edges(M, s, edges, n0, edge_cap, vert_slot, edges + at, edge_cap - at, &skipped);
}

// ---------------------------------------------------------------------------
// the optimised poses and the map points' correction (Optimizer.cc:1264-1323)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_apply_vmap(MapDev M, const int32_t *vert_slot,
                                                      const int32_t *nvert)
{
    for (int t = threadIdx.x; t < M.K; t += MAP_T) M.lp_vmap[t] = -1;
    __syncthreads();
    const int n = min(*nvert, M.K);
    for (int v = threadIdx.x; v < n; v += MAP_T)
        if (vert_slot[v] >= 0 && vert_slot[v] < M.K) M.lp_vmap[vert_slot[v]] = v;
}

__global__ __launch_bounds__(MAP_T) void k_apply_poses(MapDev M, const int32_t *vert_slot,
                                                       const int32_t *nvert, const float *Tiw)
{
    const int v = blockIdx.x * MAP_T + threadIdx.x;
    if (v >= min(*nvert, M.K)) return;
    const int s = vert_slot[v];
    if (s < 0 || s >= M.K) return;
    float T[12];
    for (int k = 0; k < 12; k++) T[k] = Tiw[(size_t)v * 12 + k];
    for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = T[k];
    loop_centre(T, M.kf_centre + s * 3);
    M.kf_pose[s] = 1;
}

// nIDr as a vertex: mnCorrectedReference's keyframe if mnCorrectedByKF is cur's mnId, else the
// reference keyframe; -1 (the point stays) for a bad point or a keyframe that is no vertex
__global__ __launch_bounds__(MAP_T) void k_apply_ref(MapDev M, int cur, float *pts, int32_t *ref)
{
    const int p = blockIdx.x * MAP_T + threadIdx.x;
    if (p >= M.P) return;
    const orbg_map_point r = M.mp[p];
    pts[3 * (size_t)p] = r.x;
    pts[3 * (size_t)p + 1] = r.y;
    pts[3 * (size_t)p + 2] = r.z;
    int v = -1;
    if (r.flags & ORBG_MP_VALID) {
        int s = M.mp_ref[p];
        if (M.mp_corr_kf[p] == M.kf_mnid[cur]) {
            // mnCorrectedReference is an mnId: mp_corr_slot remembers the slot Propagate wrote it
            // for; where that no longer carries the id (ids set since, or fields uploaded by the
            // caller), the lowest live slot with the id
            const int id = M.mp_corr_ref[p];
            s = M.mp_corr_slot[p];
            if (s < 0 || s >= M.K || M.kf_mnid[s] != id || !(M.kf_flags[s] & MAP_KF_LIVE)) {
                s = -1;
                for (int t = 0; t < M.K && s < 0; t++)
                    if ((M.kf_flags[t] & MAP_KF_LIVE) && M.kf_mnid[t] == id) s = t;
            }
        }
        if (s >= 0 && s < M.K) v = M.lp_vmap[s];
    }
    ref[p] = v;
}

__global__ void k_loop_set_corrected(MapDev M, int first, int n, const int32_t *by, const int32_t *ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    M.mp_corr_kf[first + i] = by[i];
    M.mp_corr_ref[first + i] = ref[i];
    M.mp_corr_slot[first + i] = -1;  // looked up by mnId when it is needed
}

__global__ __launch_bounds__(MAP_T) void k_apply_scatter(MapDev M, const float *pts,
                                                         const int32_t *ref)
{
    const int p = blockIdx.x * MAP_T + threadIdx.x;
    if (p >= M.P || ref[p] < 0) return;
    M.mp[p].x = pts[3 * (size_t)p];
    M.mp[p].y = pts[3 * (size_t)p + 1];
    M.mp[p].z = pts[3 * (size_t)p + 2];
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_loop_defaults(hipStream_t st, const MapDev &M)
{
    hipLaunchKernelGGL(k_loop_defaults, dim3((M.K + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M);
    return last_rc();
}

int launch_map_set_poses(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                         const float *Tcw, const int32_t *mnid)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_loop_set_poses, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, slots,
                       n, Tcw, mnid);
    return last_rc();
}

int launch_map_add_loop_edge(hipStream_t st, const MapDev &M, int a, int b, int32_t *status)
{
    hipLaunchKernelGGL(k_loop_add_edge, dim3(1), dim3(1), 0, st, M, a, b, status);
    return last_rc();
}

int launch_map_propagate(hipStream_t st, const MapDev &M, int cur, const orbg_sim3d *Scw,
                         int32_t *set, int set_cap, int32_t *nset, orbg_sim3d *corrected,
                         orbg_sim3d *noncorrected, int32_t *status, const MapScales &S,
                         int *epoch, Prof *prof)
{
    hipLaunchKernelGGL(k_loop_hdr, dim3(1), dim3(1), 0, st, M, cur);
    int rc = launch_map_update_connections(st, M, M.lp_hdr + LOOP_HDR_SLOT, 1, ++*epoch, prof);
    if (rc) return rc;
    const int g = (set_cap + 63) / 64;
    hipLaunchKernelGGL(k_loop_set, dim3(1), dim3(MAP_T), 0, st, M, cur, set, set_cap, nset, status);
    hipLaunchKernelGGL(k_loop_sim3, dim3(g), dim3(64), 0, st, M, cur, Scw, set, corrected,
                       noncorrected);
    hipLaunchKernelGGL(k_loop_points, dim3(set_cap), dim3(MAP_T), 0, st, M, cur, set, corrected,
                       noncorrected, S);
    hipLaunchKernelGGL(k_loop_apply, dim3(g), dim3(64), 0, st, M, set);
    rc = launch_map_update_connections(st, M, set, set_cap, ++*epoch, prof);
    return rc ? rc : last_rc();
}

int launch_map_loop_connections(hipStream_t st, const MapDev &M, const int32_t *set, int set_cap,
                                const int32_t *nset, uint16_t *rows, int32_t *cnt, int32_t *pairs,
                                int pair_cap, int32_t *npairs, int *epoch, Prof *prof)
{
    hipLaunchKernelGGL(k_lc_begin, dim3(1), dim3(MAP_T), 0, st, M, set, set_cap, nset, cnt);
    for (int i = 0; i < set_cap; i++) {
        hipLaunchKernelGGL(k_lc_snapshot, dim3(1), dim3(MAP_T), 0, st, M, set, i);
        const int rc = launch_map_update_connections(st, M, M.lp_hdr + LOOP_HDR_SLOT, 1, ++*epoch,
                                                     prof);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lc_diff, dim3(1), dim3(MAP_T), 0, st, M, i, rows, cnt);
    }
    hipLaunchKernelGGL(k_lc_emit, dim3(1), dim3(MAP_T), 0, st, M, set, rows, cnt, pairs, pair_cap,
                       npairs);
    return last_rc();
}

int launch_map_essential_graph(hipStream_t st, const MapDev &M, int cur, int loop,
                               const orbg_sim3d *corrected, const orbg_sim3d *noncorrected,
                               const int32_t *set, int set_cap, const int32_t *nset,
                               const int32_t *pairs, int pair_cap, const int32_t *npairs,
                               int32_t *vert_slot, int32_t *nvert, int32_t *fixed, orbg_sim3d *Scw,
                               orbg_sim3d *Snc, orbg_eg_edge *edges, int edge_cap, int32_t *nedge,
                               int32_t *status)
{
    const int g = (M.K + MAP_T - 1) / MAP_T;
    hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(MAP_T), 0, st, M, set, set_cap, nset);
    hipLaunchKernelGGL(k_eg_vertices, dim3(1), dim3(MAP_T), 0, st, M, loop, corrected, noncorrected,
                       vert_slot, nvert, fixed, Scw, Snc);
    hipLaunchKernelGGL(k_eg_kind0, dim3(1), dim3(MAP_T), 0, st, M, cur, loop, pairs, pair_cap, npairs,
                       edges, edge_cap);
    hipLaunchKernelGGL(k_eg_count, dim3(g), dim3(MAP_T), 0, st, M, edges, edge_cap, vert_slot);
    hipLaunchKernelGGL(k_eg_scan, dim3(1), dim3(MAP_T), 0, st, M, loop, nedge, status);
    hipLaunchKernelGGL(k_eg_emit, dim3(g), dim3(MAP_T), 0, st, M, edges, edge_cap, vert_slot);
    return last_rc();
}

int launch_map_apply_poses(hipStream_t st, const MapDev &M, int cur, const int32_t *vert_slot,
                           const int32_t *nvert, const float *Tiw, float *pts, int32_t *ref)
{
    hipLaunchKernelGGL(k_apply_vmap, dim3(1), dim3(MAP_T), 0, st, M, vert_slot, nvert);
    hipLaunchKernelGGL(k_apply_poses, dim3((M.K + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                       vert_slot, nvert, Tiw);
    hipLaunchKernelGGL(k_apply_ref, dim3((M.P + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, cur, pts,
                       ref);
    return last_rc();
}

int launch_map_set_corrected(hipStream_t st, const MapDev &M, int first, int n, const int32_t *by,
                             const int32_t *ref)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_loop_set_corrected, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                       first, n, by, ref);
    return last_rc();
}

int launch_map_scatter_points(hipStream_t st, const MapDev &M, const float *pts, const int32_t *ref)
{
    hipLaunchKernelGGL(k_apply_scatter, dim3((M.P + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, pts,
                       ref);
    return last_rc();
}

}  // namespace orbg
