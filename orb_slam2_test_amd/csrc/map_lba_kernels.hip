// map_lba_kernels.hip -- Optimizer::LocalBundleAdjustment on the covisibility Map
// (src/Optimizer.cc:633-979): the window the reference collects from KeyFrame and MapPoint
// objects (:635-851) and the write-back of the optimised estimates (:943-978).
//
// The window.  Every list is fixed by the table alone, never by the order in which threads run:
//   k_lba_local    lLocalKeyFrames: the slot, then its ordered covisibility list without the bad
//                  entries (ordered compaction); lrank[t] = rank, -2 for a bad entry (marked
//                  local, listed nowhere).
//   k_lba_pcount / k_lba_pscan / k_lba_pgather
//                  lLocalMapPoints: one workgroup per local keyframe, its row in feature order.
//                  A good point is kept at its first occurrence, that is when no observer with
//                  a lower rank (or a lower feature of the same row) holds it -- read from the
//                  observation index, as k_map_lp_count does.  Counts, their scan, then the
//                  ordered gather of ids and positions.  The gather also counts the point's
//                  edges (observers that are not bad) and gives every observer outside the
//                  local part the least window position that sees it (an integer atomicMin).
//   k_lba_fixed    lFixedCameras in order of first appearance = ascending (that position, slot):
//                  the observations of one point are in ascending slot.  Keys compacted in slot
//                  order, sorted in LDS; then the vertices' SE3Quat (Converter::toSE3Quat).
//   k_lba_escan    the edge offsets (one workgroup, tiles of MAP_SCAN_TILE with a carry), the
//                  counts and the status.
//   k_lba_edges    one thread per window point: its edges in ascending observer slot.
// The write-back.
//   k_lba_erase    one thread per window point (the first edge of its group): the flagged
//                  observations, mono edges first and then stereo edges, each in edge order.
//                  EraseObservation touches the point's own state and its own row entries only,
//                  so the points are independent and the result is the sequential one.
//   k_lba_write    SetPose of the local keyframes (Converter::toCvMat(SE3Quat)), the attached
//                  cameras' Tcw, SetWorldPos of every window point.
// UpdateNormalAndDepth is map_kernels.hip's, over a rebuilt observation index.  The conversions and
// the edge record are map_ba_device.h's, shared with map_gba_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "map_ba_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

#define LBA_POS_MASK 0x7FFFFu

// ---------------------------------------------------------------------------
// the window
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_lba_local(MapDev M, MapLbaWs W, int slot,
                                                     int32_t *kf_slots, int pose_cap)
{
    __shared__ int scr[16];
    __shared__ int nopose;
    if (threadIdx.x == 0) nopose = 0;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        W.lrank[t] = -1;
        W.ffirst[t] = INT_MAX;
        W.pidx[t] = -1;
    }
    __syncthreads();
    const bool live = (M.kf_flags[slot] & MAP_KF_LIVE) != 0;
    const int n = live ? min(M.nord[slot], M.K - 1) + 1 : 0;  // entry 0 is the slot itself
    const uint16_t *os = M.ord_slot + (size_t)slot * M.K;
    const int C = (n + MAP_T - 1) / MAP_T;
    const int i0 = min((int)threadIdx.x * C, n), i1 = min(i0 + C, n);
    int c = 0;
    for (int i = i0; i < i1; i++) c += i == 0 || lba_kf_good(M, os[i - 1]);
    int total;
    int pos = block_scan(c, scr, &total);
    for (int i = i0; i < i1; i++) {
        const int s = i == 0 ? slot : (int)os[i - 1];
        if (i > 0 && !lba_kf_good(M, s)) {
            W.lrank[s] = -2;
            continue;
        }
        W.lrank[s] = pos;
        W.pidx[s] = pos;
        W.lslot[pos] = s;
        W.fixed[pos] = M.kf_mnid[s] == 0;
        if (pos < pose_cap) kf_slots[pos] = s;
        if (!M.kf_pose[s]) nopose = 1;  // every writer stores 1
        pos++;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        W.hdr[LBA_HDR_NLOCAL] = total;
        W.hdr[LBA_HDR_NPOSE] = total;
        W.hdr[LBA_HDR_NPOINT] = 0;
        W.hdr[LBA_HDR_NEDGE] = 0;
        W.hdr[LBA_HDR_BITS] = (live ? 0 : ORBG_LBA_DEAD) | (nopose ? ORBG_LBA_NO_POSE : 0);
    }
}

// feature idx of slot s (local rank r) holds point p's first occurrence in the local rows
__device__ __forceinline__ bool lba_first(const MapDev &M, const MapLbaWs &W, int s, int r, int idx,
                                          int p)
{
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        const uint32_t ob = M.obs[e];
        const int u = (int)(ob >> 16), j = (int)(ob & 0xFFFFu);
        const int ru = W.lrank[u];
        if (ru >= 0 && (ru < r || (u == s && j < idx))) return false;
    }
    return true;
}

__global__ __launch_bounds__(MAP_T) void k_lba_pcount(MapDev M, MapLbaWs W)
{
    __shared__ int scr[16];
    const int r = blockIdx.x;
    if (r >= W.hdr[LBA_HDR_NLOCAL]) return;
    const int s = W.lslot[r];
    const int n = min(M.kf_n[s], M.cap);
    int c = 0;
    for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
        const int p = M.kf_points[(size_t)s * M.cap + idx];
        c += map_point_ok(M, p) && lba_first(M, W, s, r, idx, p);
    }
    int total;
    block_scan(c, scr, &total);
    if (threadIdx.x == 0) W.cnt[r] = total;
}

__global__ __launch_bounds__(MAP_T) void k_lba_pscan(MapDev M, MapLbaWs W)
{
    __shared__ int scr[16];
    const int n = W.hdr[LBA_HDR_NLOCAL];
    const int C = (n + MAP_T - 1) / MAP_T;
    const int i0 = min((int)threadIdx.x * C, n), i1 = min(i0 + C, n);
    int c = 0;
    for (int i = i0; i < i1; i++) c += W.cnt[i];
    int total;
    int o = block_scan(c, scr, &total);
    for (int i = i0; i < i1; i++) {
        const int k = W.cnt[i];
        W.cnt[i] = o;
        o += k;
    }
    if (threadIdx.x == 0) W.hdr[LBA_HDR_NPOINT] = total;
}

__global__ __launch_bounds__(MAP_T) void k_lba_pgather(MapDev M, MapLbaWs W, int32_t *point_ids,
                                                       double *points, int point_cap)
{
    __shared__ int scr[16];
    const int r = blockIdx.x;
    if (r >= W.hdr[LBA_HDR_NLOCAL]) return;
    const int s = W.lslot[r];
    const int n = min(M.kf_n[s], M.cap);
    int base = W.cnt[r], nedge = 0;
    for (int b0 = 0; b0 < n; b0 += MAP_T) {  // uniform trip count
        const int idx = b0 + threadIdx.x;
        int p = -1, keep = 0;
        if (idx < n) {
            p = M.kf_points[(size_t)s * M.cap + idx];
            keep = map_point_ok(M, p) && lba_first(M, W, s, r, idx, p);
        }
        int total;
        const int i = base + block_scan(keep, scr, &total);
        base += total;
        if (!keep) continue;
        if (i < point_cap) {
            const orbg_map_point mp = M.mp[p];
            point_ids[i] = p;
            points[3 * (size_t)i] = (double)mp.x;
            points[3 * (size_t)i + 1] = (double)mp.y;
            points[3 * (size_t)i + 2] = (double)mp.z;
        }
        int ne = 0;
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) {
            const int u = (int)(M.obs[e] >> 16);
            if (M.kf_flags[u] & ORBG_MAP_KF_BAD) continue;
            ne++;
            if (W.lrank[u] == -1 && i < (int)LBA_POS_MASK) atomicMin(&W.ffirst[u], i);
        }
        if (i < W.pcap) W.eoff[i] = ne;
        nedge += ne;
    }
    if (nedge) atomicAdd(&W.hdr[LBA_HDR_NEDGE], nedge);
}

__global__ __launch_bounds__(MAP_T) void k_lba_fixed(MapDev M, MapLbaWs W, int32_t *kf_slots,
                                                     orbg_pose *poses, int pose_cap)
{
    __shared__ int scr[16];
    __shared__ int nopose;
    uint32_t *srt = (uint32_t *)map_smem;
    if (threadIdx.x == 0) nopose = 0;
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += W.ffirst[t] != INT_MAX;
    int total;
    int pos = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++)
        if (W.ffirst[t] != INT_MAX)
            srt[pos++] = (LBA_POS_MASK - (uint32_t)W.ffirst[t]) << 13 | (MAP_SLOT_MASK - (uint32_t)t);
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    __syncthreads();
    for (int i = total + threadIdx.x; i < n2; i += MAP_T) srt[i] = 0;
    lds_sort_desc(srt, n2);
    const int nlocal = W.hdr[LBA_HDR_NLOCAL];
    for (int k = threadIdx.x; k < total; k += MAP_T) {
        const int t = (int)(MAP_SLOT_MASK - (srt[k] & MAP_SLOT_MASK));
        const int v = nlocal + k;
        if (v < M.K) {  // the parts are disjoint, so nlocal + total <= K
            W.pidx[t] = v;
            W.lslot[v] = t;
            W.fixed[v] = 1;
        }
        if (v < pose_cap) kf_slots[v] = t;
        if (!M.kf_pose[t]) nopose = 1;
    }
    __syncthreads();
    const int npose = min(nlocal + total, M.K);
    for (int v = threadIdx.x; v < min(npose, pose_cap); v += MAP_T)
        lba_se3quat(M.kf_Tcw + (size_t)W.lslot[v] * 12, W.fixed[v], &poses[v]);
    if (threadIdx.x == 0) {
        W.hdr[LBA_HDR_NPOSE] = npose;
        if (nopose) W.hdr[LBA_HDR_BITS] |= ORBG_LBA_NO_POSE;
    }
}

__global__ __launch_bounds__(MAP_T) void k_lba_escan(MapLbaWs W, int pose_cap, int point_cap,
                                                     int edge_cap, int32_t *counts,
                                                     int32_t *status)
{
    __shared__ int scr[16];
    const int npoint = W.hdr[LBA_HDR_NPOINT];
    const int n = min(npoint, min(point_cap, W.pcap));
    constexpr int PER = MAP_SCAN_TILE / MAP_T;
    int carry = 0;
    for (int b0 = 0; b0 < n; b0 += MAP_SCAN_TILE) {  // uniform trip count
        const int base = b0 + threadIdx.x * PER;
        int v[PER], c = 0;
        for (int k = 0; k < PER; k++) {
            v[k] = base + k < n ? W.eoff[base + k] : 0;
            c += v[k];
        }
        int total;
        int run = carry + block_scan(c, scr, &total);
        for (int k = 0; k < PER; k++) {
            if (base + k < n) W.eoff[base + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        W.eoff[n] = carry;
        int bits = W.hdr[LBA_HDR_BITS];
        if (W.hdr[LBA_HDR_NPOSE] > pose_cap || npoint > point_cap || W.hdr[LBA_HDR_NEDGE] > edge_cap)
            bits |= ORBG_LBA_RANGE;
        W.hdr[LBA_HDR_BITS] = bits;
        for (int k = 0; k < 4; k++) counts[k] = W.hdr[k];
        status[0] = bits;
        status[1] = status[2] = status[3] = 0;
    }
}

__global__ __launch_bounds__(MAP_T) void k_lba_edges(MapDev M, MapAttach A, MapLbaWs W,
                                                     const int32_t *point_ids, int point_cap,
                                                     orbg_edge *edges, int32_t *edge_feat,
                                                     int edge_cap, MapLbaConst C, int32_t *status)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= min(W.hdr[LBA_HDR_NPOINT], min(point_cap, W.pcap))) return;
    const int p = point_ids[i];
    int at = W.eoff[i];
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        const uint32_t ob = M.obs[e];
        const int u = (int)(ob >> 16), j = (int)(ob & 0xFFFFu);
        if (M.kf_flags[u] & ORBG_MAP_KF_BAD) continue;
        const int k = at++;
        if (k >= edge_cap) continue;
        orbg_edge E;
        if (!lba_fill_edge(A, C, u, j, i, W.pidx[u], 1, &E)) atomicOr(&status[0], ORBG_LBA_FEATURE);
        edges[k] = E;
        edge_feat[k] = j;
    }
}

// ---------------------------------------------------------------------------
// the write-back
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_lba_begin(MapLbaWs W)
{
    W.hdr[LBA_HDR_NERASED] = 0;
    W.hdr[LBA_HDR_NBAD] = 0;
}

__global__ __launch_bounds__(MAP_T) void k_lba_erase(MapDev M, MapLbaWs W, const int32_t *counts,
                                                     const int32_t *kf_slots, int pose_cap,
                                                     const int32_t *point_ids, int point_cap,
                                                     const orbg_edge *edges,
                                                     const int32_t *edge_feat, int edge_cap,
                                                     const uint8_t *erase)
{
    const int e0 = blockIdx.x * MAP_T + threadIdx.x;
    const int npose = min(counts[1], pose_cap), npoint = min(counts[2], point_cap);
    const int nedge = min(counts[3], edge_cap);
    if (e0 >= nedge) return;
    const int i = edges[e0].point;
    if (e0 > 0 && edges[e0 - 1].point == i) return;  // the group's first edge walks it
    if (i < 0 || i >= npoint) return;
    const int p = point_ids[i];
    if (!map_point_ok(M, p)) return;
    int nobs = cull_nobs(M, p), nerased = 0;
    bool bad = false;
    for (int pass = 0; pass < 2 && !bad; pass++)  // vpEdgesMono, then vpEdgesStereo
        for (int e = e0; e < nedge && edges[e].point == i && !bad; e++) {
            if (!erase[e] || (edges[e].stereo != 0) != (pass != 0)) continue;
            const int v = edges[e].pose, j = edge_feat[e];
            if (v < 0 || v >= npose || j < 0 || j >= M.cap) continue;
            const int u = kf_slots[v];
            if (u < 0 || u >= M.K || !(M.kf_flags[u] & MAP_KF_LIVE)) continue;
            if (M.kf_points[(size_t)u * M.cap + j] != p) continue;
            nobs -= cull_weight(M, u, j);
            M.kf_points[(size_t)u * M.cap + j] = -1;  // EraseMapPointMatch
            nerased++;
            if (M.mp_ref[p] == u) {  // the lowest remaining observing slot
                int low = -1;
                const int o1 = M.obs_off[p + 1];
                for (int o = M.obs_off[p]; o < o1 && low < 0; o++) {
                    int t, k;
                    if (cull_obs(M, M.obs[o], p, &t, &k)) low = t;
                }
                M.mp_ref[p] = low;
            }
            if (nobs <= 2) {
                cull_point_bad(M, p);
                bad = true;
            }
        }
    if (nerased) atomicAdd(&W.hdr[LBA_HDR_NERASED], nerased);
    if (bad) atomicAdd(&W.hdr[LBA_HDR_NBAD], 1);
}

__global__ __launch_bounds__(MAP_T) void k_lba_write(MapDev M, MapLbaWs W, const int32_t *counts,
                                                     const int32_t *kf_slots, int pose_cap,
                                                     const int32_t *point_ids, int point_cap,
                                                     const orbg_pose *poses, const double *points,
                                                     orbg_frustum_camera *cams_out, int32_t *out)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i < min(min(counts[0], counts[1]), pose_cap)) {
        const int s = kf_slots[i];
        if (s >= 0 && s < M.K) {
            float T[12];
            lba_tcw(poses[i], T);
            for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = T[k];
            loop_centre(T, M.kf_centre + s * 3);
            M.kf_pose[s] = 1;
            if (cams_out)
                for (int k = 0; k < 12; k++) cams_out[s].Tcw[k] = T[k];
        }
    }
    if (i < min(point_cap, W.pcap)) {
        int p = i < counts[2] ? point_ids[i] : -1;
        if (p >= M.P) p = -1;
        W.ids[i] = p;
        if (p >= 0) {
            M.mp[p].x = (float)points[3 * (size_t)i];
            M.mp[p].y = (float)points[3 * (size_t)i + 1];
            M.mp[p].z = (float)points[3 * (size_t)i + 2];
        }
    }
    if (i == 0) {
        out[0] = W.hdr[LBA_HDR_NERASED];
        out[1] = W.hdr[LBA_HDR_NBAD];
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_lba_window(hipStream_t st, const MapDev &M, const MapAttach &A, const MapLbaWs &W,
                          int slot, const MapLbaWindow &O, const MapLbaConst &C, int32_t *status,
                          Prof *prof)
{
    const size_t lds = (size_t)map_pow2(M.K) * 4;
    if (map_attr((const void *)k_lba_fixed, lds)) return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_lba_window", &ev);
    hipLaunchKernelGGL(k_lba_local, dim3(1), dim3(MAP_T), 0, st, M, W, slot, O.kf_slots, O.pose_cap);
    hipLaunchKernelGGL(k_lba_pcount, dim3(M.K), dim3(MAP_T), 0, st, M, W);
    hipLaunchKernelGGL(k_lba_pscan, dim3(1), dim3(MAP_T), 0, st, M, W);
    hipLaunchKernelGGL(k_lba_pgather, dim3(M.K), dim3(MAP_T), 0, st, M, W, O.point_ids, O.points,
                       O.point_cap);
    hipLaunchKernelGGL(k_lba_fixed, dim3(1), dim3(MAP_T), lds, st, M, W, O.kf_slots, O.poses,
                       O.pose_cap);
    hipLaunchKernelGGL(k_lba_escan, dim3(1), dim3(MAP_T), 0, st, W, O.pose_cap, O.point_cap,
                       O.edge_cap, O.counts, status);
    if (O.point_cap > 0)
        hipLaunchKernelGGL(k_lba_edges, dim3((O.point_cap + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st,
                           M, A, W, O.point_ids, O.point_cap, O.edges, O.edge_feat, O.edge_cap, C,
                           status);
    prof_end(prof, st, "map_lba_window", ev);
    return last_rc();
}

int launch_map_lba_apply(hipStream_t st, const MapDev &M, const MapLbaWs &W, const MapLbaWindow &O,
                         const uint8_t *erase, orbg_frustum_camera *cams_out, int32_t *out,
                         Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_lba_apply", &ev);
    hipLaunchKernelGGL(k_lba_begin, dim3(1), dim3(1), 0, st, W);
    if (O.edge_cap > 0)
        hipLaunchKernelGGL(k_lba_erase, dim3((O.edge_cap + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                           W, O.counts, O.kf_slots, O.pose_cap, O.point_ids, O.point_cap, O.edges,
                           O.edge_feat, O.edge_cap, erase);
    const int n = std::max(std::max(std::min(O.pose_cap, M.K), O.point_cap), 1);
    hipLaunchKernelGGL(k_lba_write, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, W, O.counts,
                       O.kf_slots, O.pose_cap, O.point_ids, O.point_cap, O.poses, O.points, cams_out,
                       out);
    prof_end(prof, st, "map_lba_apply", ev);
    return last_rc();
}

}  // namespace orbg
