// map_kernels.hip -- the covisibility Map on gfx950: the table "which keyframe slot observes
// which map point" and the three reference functions that count, sort and gather over it
// (KeyFrame::UpdateConnections, src/KeyFrame.cc:375-515 with AddConnection / EraseConnection /
// UpdateBestCovisibles; Tracking::UpdateLocalKeyFrames and UpdateLocalPoints,
// src/Tracking.cc:1731-1925; MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:457-518).
//
//   k_map_obs_count / k_map_scan_* / k_map_obs_fill / k_map_obs_place
//                    the point -> observations CSR from the live rows: histogram (integer
//                    atomics), exclusive scan (tile sums, a one-workgroup scan of the sums,
//                    tiles), fill in arrival order, then every entry is placed at its rank by
//                    slot inside its point's segment, so a segment is in ascending slot order
//                    whatever the arrival order was.
//   k_map_tree_*     the spanning tree's children lists (ascending slot) from `parent`.
//   k_map_update     one workgroup per slot s: an LDS histogram over the slots, filled from
//                    the observations of the row's points; W[s][*] = the histogram; the
//                    AddConnection writes W[t][s] (t marked dirty when the value changed); s's
//                    own ordered list from the slots with weight >= 15 (or pKFmax alone), keys
//                    weight << 13 | slot compacted in slot order and bitonic-sorted descending
//                    = descending weight, ties by descending slot; the first parent.
//   k_map_resort     UpdateBestCovisibles of the rows marked dirty by this call that are not
//                    members of its batch: all non-zero weights of the row, the same sort.
//   k_map_local_kfs  one workgroup per frame: vote histogram in LDS, the voted slots in
//                    ascending order (ordered compaction), then the reference's sequential
//                    expansion by one thread over state staged in LDS.
//   k_map_lp_count / k_map_lp_gather
//                    one workgroup per (local keyframe, frame): a point is kept at its first
//                    occurrence, that is when the least list position among its observing
//                    slots is this keyframe's; counts, then the ordered gather of ids,
//                    records and descriptors.
//   k_map_normal_depth  one thread per point, its observations in ascending slot order.
// No result depends on thread order: the atomics are integer counters.
// The workgroup scan, the LDS sort and the ordered-list store are in map_device.h, shared with
// map_cull_kernels.hip (SetBadFlag, KeyFrameCulling, MapPointCulling over the same table).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

// ---------------------------------------------------------------------------
// mutations
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_set_kf(MapDev M, const int32_t *slots,
                                                      const int32_t *points, const uint8_t *oct,
                                                      int row_cap, const int32_t *counts,
                                                      const float *centres, const int32_t *flags)
{
    const int i = blockIdx.x;
    const int s = slots[i];
    if (s < 0 || s >= M.K) return;
    const int n = min(max(counts[i], 0), min(row_cap, M.cap));
    int32_t *dp = M.kf_points + (size_t)s * M.cap;
    uint8_t *dq = M.kf_oct + (size_t)s * M.cap;
    for (int k = threadIdx.x; k < M.cap; k += MAP_T) {
        int32_t p = k < n ? points[(size_t)i * row_cap + k] : -1;
        if (p >= M.P) p = -1;
        dp[k] = p < 0 ? -1 : p;
        dq[k] = k < n ? oct[(size_t)i * row_cap + k] : 0;
    }
    const int was = M.kf_flags[s];
    if (!(was & MAP_KF_LIVE))  // a new KeyFrame's keypoints: no feature flags yet
        for (int k = threadIdx.x; k < M.cap; k += MAP_T) M.kf_feat[(size_t)s * M.cap + k] = 0;
    __syncthreads();  // every thread has read kf_flags[s]
    if (threadIdx.x == 0) {
        M.kf_flags[s] = MAP_KF_LIVE | (flags[i] & (ORBG_MAP_KF_ROOT | ORBG_MAP_KF_BAD));
        M.kf_n[s] = n;
        for (int k = 0; k < 3; k++) M.kf_centre[s * 3 + k] = centres[i * 3 + k];
        if (!(was & MAP_KF_LIVE)) {  // a new KeyFrame: no parent yet, mbFirstConnection
            M.parent[s] = -1;
            M.first_conn[s] = 1;
            M.kf_erase[s] = 0;
            M.kf_gba[s] = 0;
        }
    }
}

__global__ void k_map_set_points(MapDev M, const int32_t *ids, int first, int n,
                                 const orbg_map_point *mps, const uint8_t *desc, const int32_t *ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = ids ? ids[i] : first + i;
    if (p < 0 || p >= M.P) return;
    M.mp[p] = mps[i];
    for (int k = 0; k < 32; k++) M.mdesc[(size_t)p * 32 + k] = desc[(size_t)i * 32 + k];
    M.mp_ref[p] = ref[i];
}

__global__ void k_map_point_bad(MapDev M, int p) { M.mp[p].flags &= ~ORBG_MP_VALID; }

__global__ void k_map_set_parent(MapDev M, int s, int parent) { M.parent[s] = parent; }

// SetBadFlag's table side: the row, W[s][*] and every W[t][s] > 0 (t marked dirty)
__global__ __launch_bounds__(MAP_T) void k_map_erase(MapDev M, int s, int epoch)
{
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        if (M.W[(size_t)t * M.K + s]) {
            M.W[(size_t)t * M.K + s] = 0;
            M.dirty[t] = epoch;
        }
        M.W[(size_t)s * M.K + t] = 0;
    }
    for (int k = threadIdx.x; k < M.cap; k += MAP_T) M.kf_points[(size_t)s * M.cap + k] = -1;
    if (threadIdx.x < ORBG_MAP_NEIGH) M.neigh[s * ORBG_MAP_NEIGH + threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        M.kf_flags[s] = (M.kf_flags[s] & ORBG_MAP_KF_ROOT) | ORBG_MAP_KF_BAD;
        M.kf_n[s] = 0;
        M.nord[s] = 0;
        M.mark[s] = epoch;  // its own (now empty) list is not re-sorted
    }
}

__global__ __launch_bounds__(MAP_T) void k_map_count(MapDev M)
{
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int c = 0;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) c += (M.kf_flags[t] & MAP_KF_LIVE) != 0;
    atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) M.nlive[0] = cnt;
}

// ---------------------------------------------------------------------------
// the observation index
// ---------------------------------------------------------------------------
template <int PASS>  // 0: histogram, 1: fill, 2: place by rank
__global__ __launch_bounds__(MAP_T) void k_map_obs(MapDev M)
{
    const int s = blockIdx.x;
    if (!(M.kf_flags[s] & MAP_KF_LIVE)) return;
    const int n = min(M.kf_n[s], M.cap);
    for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
        const int p = M.kf_points[(size_t)s * M.cap + idx];
        if (p < 0 || p >= M.P) continue;
        if (PASS == 0) {
            atomicAdd(&M.obs_cnt[p], 1);
        } else if (PASS == 1) {
            const int e = M.obs_off[p] + atomicAdd(&M.obs_cnt[p], 1);
            M.obs_tmp[e] = (uint32_t)s << 16 | (uint32_t)idx;
        } else {
            // rank by the whole entry (slot, then idx): unique even if a row breaks the
            // once-per-row precondition, so every place of the segment is written
            const int e0 = M.obs_off[p], e1 = M.obs_off[p + 1];
            const uint32_t mine = (uint32_t)s << 16 | (uint32_t)idx;
            int rank = 0;
            for (int e = e0; e < e1; e++) rank += M.obs_tmp[e] < mine;
            M.obs[e0 + rank] = mine;
        }
    }
}

__global__ __launch_bounds__(MAP_T) void k_map_scan_sum(const int32_t *cnt, int n, int32_t *part)
{
    __shared__ int scr[4];
    const int base = blockIdx.x * MAP_SCAN_TILE + threadIdx.x * (MAP_SCAN_TILE / MAP_T);
    int c = 0;
    for (int k = 0; k < MAP_SCAN_TILE / MAP_T; k++)
        if (base + k < n) c += cnt[base + k];
    int total;
    block_scan(c, scr, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(MAP_T) void k_map_scan_part(int32_t *part, int nt)
{
    __shared__ int scr[4];
    int carry = 0;
    for (int base = 0; base < nt; base += MAP_T) {  // uniform trip count
        const int i = base + threadIdx.x;
        const int v = i < nt ? part[i] : 0;
        int total;
        const int ex = block_scan(v, scr, &total);
        if (i < nt) part[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(MAP_T) void k_map_scan_tile(const int32_t *cnt, int n,
                                                         const int32_t *part, int32_t *off)
{
    __shared__ int scr[4];
    const int base = blockIdx.x * MAP_SCAN_TILE + threadIdx.x * (MAP_SCAN_TILE / MAP_T);
    int v[MAP_SCAN_TILE / MAP_T], c = 0;
    for (int k = 0; k < MAP_SCAN_TILE / MAP_T; k++) {
        v[k] = base + k < n ? cnt[base + k] : 0;
        c += v[k];
    }
    int total;
    int run = part[blockIdx.x] + block_scan(c, scr, &total);
    for (int k = 0; k < MAP_SCAN_TILE / MAP_T; k++) {
        if (base + k < n) off[base + k] = run;
        run += v[k];
        if (base + k == n - 1) off[n] = run;
    }
}

__global__ void k_map_tree_head(MapDev M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M.K) return;
    const int par = M.parent[c];
    if (par >= 0 && par < M.K) atomicMin((unsigned int *)&M.child_head[par], (unsigned int)c);
}

__global__ void k_map_tree_next(MapDev M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M.K) return;
    const int par = M.parent[c];
    int nx = -1;
    if (par >= 0 && par < M.K)
        for (int d = c + 1; d < M.K; d++)
            if (M.parent[d] == par) {
                nx = d;
                break;
            }
    M.child_next[c] = nx;
}

// ---------------------------------------------------------------------------
// KeyFrame::UpdateConnections
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_update(MapDev M, const int32_t *slots, int epoch,
                                                      int bn)
{
    uint32_t *hist = (uint32_t *)map_smem;
    uint32_t *srt = (uint32_t *)(map_smem + map_off_b(M.K));
    int *scr = (int *)(map_smem + map_off_scr(M.K, bn));
    const int s = slots[blockIdx.x];
    if (s < 0 || s >= M.K) return;
    if (!(M.kf_flags[s] & MAP_KF_LIVE)) return;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) hist[t] = 0;
    if (threadIdx.x == 0) scr[8] = scr[9] = 0;
    __syncthreads();
    const int n = min(M.kf_n[s], M.cap);
    for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
        const int p = M.kf_points[(size_t)s * M.cap + idx];
        if (!map_point_ok(M, p)) continue;
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) {
            const int t = (int)(M.obs[e] >> 16);
            if (t != s) atomicAdd(&hist[t], 1u);
        }
    }
    __syncthreads();
    // nmax / pKFmax by strict > in ascending slot order = the greatest weight, lowest slot
    uint32_t best = 0;
    int n15 = 0;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        const uint32_t w = hist[t];
        if (w) best = max(best, w << 13 | (MAP_SLOT_MASK - (uint32_t)t));
        n15 += w >= ORBG_MAP_TH;
    }
    if (best) atomicMax((unsigned int *)&scr[8], best);
    if (n15) atomicAdd(&scr[9], n15);
    __syncthreads();
    best = (uint32_t)scr[8];
    n15 = scr[9];
    if (!best) return;  // KFcounter.empty(): nothing changes
    const int kmax = (int)(MAP_SLOT_MASK - (best & MAP_SLOT_MASK));
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        const uint32_t w = hist[t];
        M.W[(size_t)s * M.K + t] = (uint16_t)w;
        const bool pair = n15 ? w >= ORBG_MAP_TH : t == kmax;
        if (pair) {  // AddConnection(this, w) on t
            uint16_t *wt = M.W + (size_t)t * M.K + s;
            if (*wt != (uint16_t)w) {
                *wt = (uint16_t)w;
                M.dirty[t] = epoch;
            }
        }
        hist[t] = pair ? w << 13 | (uint32_t)t : 0;
    }
    if (threadIdx.x == 0) M.mark[s] = epoch;
    __syncthreads();
    map_store_order(M, s, hist, srt, scr);
    if (threadIdx.x == 0 && M.first_conn[s] && !(M.kf_flags[s] & ORBG_MAP_KF_ROOT)) {
        M.parent[s] = (int32_t)(srt[0] & MAP_SLOT_MASK);
        M.first_conn[s] = 0;
    }
}

__global__ __launch_bounds__(MAP_T) void k_map_resort(MapDev M, int epoch, int bn)
{
    uint32_t *keys = (uint32_t *)map_smem;
    uint32_t *srt = (uint32_t *)(map_smem + map_off_b(M.K));
    int *scr = (int *)(map_smem + map_off_scr(M.K, bn));
    const int t = blockIdx.x;
    if (M.dirty[t] != epoch || M.mark[t] == epoch) return;
    for (int u = threadIdx.x; u < M.K; u += MAP_T) {
        const uint32_t w = M.W[(size_t)t * M.K + u];
        keys[u] = w ? w << 13 | (uint32_t)u : 0;
    }
    __syncthreads();
    map_store_order(M, t, keys, srt, scr);
}

// GetConnectedKeyFrames: the non-zeros of the W row, ascending
__global__ __launch_bounds__(MAP_T) void k_map_connected(MapDev M, const int32_t *slots,
                                                         int32_t *conn, int conn_cap,
                                                         int32_t *nconn)
{
    __shared__ int scr[4];
    const int s = slots[blockIdx.x];
    if (s < 0 || s >= M.K) {  // uniform
        if (threadIdx.x == 0) nconn[blockIdx.x] = 0;
        return;
    }
    const uint16_t *w = M.W + (size_t)s * M.K;
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += w[t] != 0;
    int total;
    int pos = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++)
        if (w[t]) {
            if (pos < conn_cap) conn[(size_t)blockIdx.x * conn_cap + pos] = t;
            pos++;
        }
    if (threadIdx.x == 0) nconn[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// Tracking::UpdateLocalKeyFrames
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_local_kfs(MapDev M, int32_t *frame_points,
                                                         int frame_cap, const int32_t *counts,
                                                         int32_t *local_kfs, int lkf_cap,
                                                         int32_t *nlocal, int32_t *ref_kf, int bn)
{
    uint32_t *hist = (uint32_t *)map_smem;  // votes | MAP_BADBIT | MAP_MARKBIT
    int32_t *list = (int32_t *)(map_smem + map_off_b(M.K));
    int32_t *pre = (int32_t *)(map_smem + map_off_pre(M.K, bn));
    int *scr = (int *)(map_smem + map_off_scr(M.K, bn));
    const int f = blockIdx.x;
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        const int fl = M.kf_flags[t];
        hist[t] = (fl & ORBG_MAP_KF_BAD) || !(fl & MAP_KF_LIVE) ? MAP_BADBIT : 0;
    }
    if (threadIdx.x == 0) scr[8] = scr[9] = 0;
    __syncthreads();
    int32_t *fp = frame_points + (size_t)f * frame_cap;
    const int nfp = min(max(counts[f], 0), frame_cap);
    for (int i = threadIdx.x; i < nfp; i += MAP_T) {
        const int p = fp[i];
        if (p < 0 || p >= M.P) continue;
        if (!(M.mp[p].flags & ORBG_MP_VALID)) {
            fp[i] = -1;  // mCurrentFrame.mvpMapPoints[i] = NULL
            continue;
        }
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) atomicAdd(&hist[M.obs[e] >> 16], 1u);
    }
    __syncthreads();
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    uint32_t best = 0;
    int any = 0, c = 0;
    for (int t = t0; t < t1; t++) {
        const uint32_t v = hist[t] & MAP_VOTES;
        if (!v) continue;
        any = 1;
        if (hist[t] & MAP_BADBIT) continue;
        c++;
        best = max(best, v << 13 | (MAP_SLOT_MASK - (uint32_t)t));
    }
    if (best) atomicMax((unsigned int *)&scr[8], best);
    if (any) scr[9] = 1;
    int n0;
    int pos = block_scan(c, scr, &n0);
    if (!scr[9]) {  // keyframeCounter.empty(): the reference returns
        if (threadIdx.x == 0) nlocal[f] = ref_kf[f] = -1;
        return;
    }
    for (int t = t0; t < t1; t++)
        if ((hist[t] & MAP_VOTES) && !(hist[t] & MAP_BADBIT)) {
            list[pos++] = t;
            hist[t] |= MAP_MARKBIT;
        }
    __syncthreads();
    if (n0 <= ORBG_MAP_MAX_LOCAL)  // else the expansion loop leaves at once
        for (int j = threadIdx.x; j < n0 * MAP_PRE; j += MAP_T) {
            const int kf = list[j / MAP_PRE], k = j % MAP_PRE;
            pre[j] = k < ORBG_MAP_NEIGH ? M.neigh[kf * ORBG_MAP_NEIGH + k]
                     : k == ORBG_MAP_NEIGH ? M.child_head[kf]
                                           : M.parent[kf];
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = n0;
        for (int i = 0; i < n0; i++) {  // the initial list only: the end iterator is fixed
            if (n > ORBG_MAP_MAX_LOCAL) break;
            const int32_t *q = pre + i * MAP_PRE;
            for (int k = 0; k < ORBG_MAP_NEIGH; k++) {
                const int nb = q[k];
                if (nb < 0 || nb >= M.K) continue;
                if (!(hist[nb] & (MAP_BADBIT | MAP_MARKBIT))) {
                    list[n++] = nb;
                    hist[nb] |= MAP_MARKBIT;
                    break;
                }
            }
            for (int ch = q[ORBG_MAP_NEIGH]; ch >= 0 && ch < M.K; ch = M.child_next[ch])
                if (!(hist[ch] & (MAP_BADBIT | MAP_MARKBIT))) {
                    list[n++] = ch;
                    hist[ch] |= MAP_MARKBIT;
                    break;
                }
            const int par = q[ORBG_MAP_NEIGH + 1];
            if (par >= 0 && par < M.K && !(hist[par] & MAP_MARKBIT)) {
                list[n++] = par;
                hist[par] |= MAP_MARKBIT;
                break;  // Tracking.cc:1912
            }
        }
        scr[10] = n;
    }
    __syncthreads();
    const int n = scr[10];
    for (int i = threadIdx.x; i < min(n, lkf_cap); i += MAP_T)
        local_kfs[(size_t)f * lkf_cap + i] = list[i];
    if (threadIdx.x == 0) {
        nlocal[f] = n;
        const uint32_t b = (uint32_t)scr[8];
        ref_kf[f] = b ? (int32_t)(MAP_SLOT_MASK - (b & MAP_SLOT_MASK)) : -1;
    }
}

// ---------------------------------------------------------------------------
// Tracking::UpdateLocalPoints (+ SearchLocalPoints' flags)
// ---------------------------------------------------------------------------
// pos[t] = least position of slot t in the frame's local keyframe list (0xFFFFFFFF: not in it)
__device__ __forceinline__ void map_list_pos(const MapDev &M, const int32_t *lk, int nl,
                                             uint32_t *pos)
{
    for (int t = threadIdx.x; t < M.K; t += MAP_T) pos[t] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = threadIdx.x; i < nl; i += MAP_T) {
        const int t = lk[i];
        if (t >= 0 && t < M.K) atomicMin(&pos[t], (uint32_t)i);
    }
    __syncthreads();
}

// feature idx of slot s (at list position j) holds a point's first occurrence in the list
__device__ __forceinline__ bool map_lp_keep(const MapDev &M, const uint32_t *pos, int s, int j,
                                            int idx, int *pout)
{
    const int p = M.kf_points[(size_t)s * M.cap + idx];
    *pout = p;
    if (!map_point_ok(M, p)) return false;
    uint32_t least = 0xFFFFFFFFu;
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) least = min(least, pos[M.obs[e] >> 16]);
    return least == (uint32_t)j;
}

__global__ __launch_bounds__(MAP_T) void k_map_lp_count(MapDev M, const int32_t *local_kfs,
                                                        int lkf_cap, const int32_t *nlocal,
                                                        int32_t *cnt, int bn)
{
    uint32_t *pos = (uint32_t *)map_smem;
    int *scr = (int *)(map_smem + map_off_scr(M.K, bn));
    const int j = blockIdx.x, f = blockIdx.y;
    const int nl = min(max(nlocal[f], 0), lkf_cap);
    const int32_t *lk = local_kfs + (size_t)f * lkf_cap;
    if (j >= nl) {  // uniform
        if (threadIdx.x == 0) cnt[(size_t)f * lkf_cap + j] = 0;
        return;
    }
    if (threadIdx.x == 0) scr[8] = 0;
    map_list_pos(M, lk, nl, pos);
    const int s = lk[j];
    int c = 0;
    if (s >= 0 && s < M.K && pos[s] == (uint32_t)j && (M.kf_flags[s] & MAP_KF_LIVE)) {
        const int n = min(M.kf_n[s], M.cap);
        for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
            int p;
            c += map_lp_keep(M, pos, s, j, idx, &p);
        }
    }
    if (c) atomicAdd(&scr[8], c);
    __syncthreads();
    if (threadIdx.x == 0) cnt[(size_t)f * lkf_cap + j] = scr[8];
}

__global__ __launch_bounds__(MAP_T) void k_map_lp_gather(MapDev M, const int32_t *local_kfs,
                                                         int lkf_cap, const int32_t *nlocal,
                                                         const int32_t *cnt,
                                                         const int32_t *frame_points, int frame_cap,
                                                         const int32_t *counts, int32_t *ids,
                                                         orbg_map_point *mps, uint8_t *qdesc,
                                                         int lp_cap, int32_t *nlp, int bn)
{
    uint32_t *pos = (uint32_t *)map_smem;
    uint32_t *fps = (uint32_t *)(map_smem + map_off_b(M.K));  // the frame's points + 1, descending
    int *scr = (int *)(map_smem + map_off_scr(M.K, bn));
    const int j = blockIdx.x, f = blockIdx.y;
    const int nl = min(max(nlocal[f], 0), lkf_cap);
    const int32_t *lk = local_kfs + (size_t)f * lkf_cap;
    if (j >= nl && j > 0) return;  // uniform (workgroup 0 writes the frame's count)
    int before = 0, all = 0;
    for (int i = threadIdx.x; i < nl; i += MAP_T) {
        const int v = cnt[(size_t)f * lkf_cap + i];
        all += v;
        if (i < j) before += v;
    }
    if (threadIdx.x == 0) scr[8] = scr[9] = 0;
    __syncthreads();
    if (before) atomicAdd(&scr[8], before);
    if (all) atomicAdd(&scr[9], all);
    __syncthreads();
    const int base = scr[8];
    if (j == 0 && threadIdx.x == 0) nlp[f] = scr[9];
    if (j >= nl) return;
    map_list_pos(M, lk, nl, pos);
    const int s = lk[j];
    if (!(s >= 0 && s < M.K && pos[s] == (uint32_t)j && (M.kf_flags[s] & MAP_KF_LIVE))) return;
    // mnLastFrameSeen == mCurrentFrame.mnId: membership in the frame's own points
    const int nfp = min(max(counts[f], 0), frame_cap);
    int n2 = 1;
    while (n2 < nfp) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += MAP_T) {
        const int p = i < nfp ? frame_points[(size_t)f * frame_cap + i] : -1;
        fps[i] = p < 0 ? 0u : (uint32_t)p + 1u;
    }
    lds_sort_desc(fps, n2);
    // ordered compaction: a contiguous chunk of the row per thread, its keeps as a bit mask
    const int n = min(M.kf_n[s], M.cap);
    const int C = (n + MAP_T - 1) / MAP_T;  // <= 32
    const int i0 = min((int)threadIdx.x * C, n), i1 = min(i0 + C, n);
    uint32_t keep = 0;
    for (int idx = i0; idx < i1; idx++) {
        int p;
        if (map_lp_keep(M, pos, s, j, idx, &p)) keep |= 1u << (idx - i0);
    }
    int total;
    int o = base + block_scan(__popc(keep), scr, &total);
    for (int idx = i0; idx < i1; idx++) {
        if (!(keep >> (idx - i0) & 1u)) continue;
        if (o < lp_cap) {
            const int p = M.kf_points[(size_t)s * M.cap + idx];
            const uint32_t key = (uint32_t)p + 1u;
            int lo = 0, hi = n2;  // first entry <= key in the descending array
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (fps[mid] > key)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            const bool in_frame = lo < n2 && fps[lo] == key;
            orbg_map_point r = M.mp[p];
            r.flags = (in_frame ? 0 : ORBG_MP_VALID) |
                      (M.obs_off[p + 1] > M.obs_off[p] ? ORBG_MP_HAS_OBS : 0);
            const size_t q = (size_t)f * lp_cap + o;
            ids[q] = p;
            mps[q] = r;
            const uint32_t *src = (const uint32_t *)(M.mdesc + (size_t)p * 32);
            uint8_t *dst = qdesc + q * 32;
            for (int k = 0; k < 8; k++) {
                const uint32_t v = src[k];
                dst[4 * k] = (uint8_t)v;
                dst[4 * k + 1] = (uint8_t)(v >> 8);
                dst[4 * k + 2] = (uint8_t)(v >> 16);
                dst[4 * k + 3] = (uint8_t)(v >> 24);
            }
        }
        o++;
    }
}

// ---------------------------------------------------------------------------
// MapPoint::UpdateNormalAndDepth
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_normal_depth(MapDev M, const int32_t *ids, int n,
                                                            MapScales S)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= n) return;
    const int p = ids ? ids[i] : i;
    if (p < 0 || p >= M.P) return;
    orbg_map_point r = M.mp[p];
    if (!(r.flags & ORBG_MP_VALID)) return;
    const int e0 = M.obs_off[p], e1 = M.obs_off[p + 1];
    if (e0 == e1) return;
    const int ref = M.mp_ref[p];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, dist = 0.0f;
    int ridx = -1;
    for (int e = e0; e < e1; e++) {
        const uint32_t ob = M.obs[e];
        const int s = (int)(ob >> 16);
        const float *O = M.kf_centre + s * 3;
        const float dx = r.x - O[0], dy = r.y - O[1], dz = r.z - O[2];  // mWorldPos - Owi
        double sq = (double)dx * (double)dx;                            // cv::norm: double, in order
        sq += (double)dy * (double)dy;
        sq += (double)dz * (double)dz;
        const double nrm = sqrt(sq);
        const float a = (float)(1.0 / nrm);  // Mat / double: the float alpha 1. / s
        nx = nx + dx * a;
        ny = ny + dy * a;
        nz = nz + dz * a;
        if (s == ref) {
            ridx = (int)(ob & 0xFFFFu);
            dist = (float)nrm;  // const float dist = cv::norm(PC)
        }
    }
    if (ridx < 0) return;  // the reference keyframe does not observe the point
    int level = M.kf_oct[(size_t)ref * M.cap + ridx];
    level = min(level, 15);
    const float maxd = dist * S.scale[level];
    const float mind = maxd / S.scale[S.nlevels - 1];
    const float inv = (float)(1.0 / (double)(e1 - e0));  // normal / n
    r.nx = nx * inv;
    r.ny = ny * inv;
    r.nz = nz * inv;
    r.max_dist = maxd;
    r.min_dist = mind;
    M.mp[p] = r;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_set_keyframes(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                             const int32_t *points, const uint8_t *oct, int row_cap,
                             const int32_t *counts, const float *centres, const int32_t *flags)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_set_kf, dim3(n), dim3(MAP_T), 0, st, M, slots, points, oct, row_cap,
                       counts, centres, flags);
    return last_rc();
}

int launch_map_set_points(hipStream_t st, const MapDev &M, const int32_t *ids, int first, int n,
                          const orbg_map_point *mps, const uint8_t *desc, const int32_t *ref)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_set_points, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, ids,
                       first, n, mps, desc, ref);
    return last_rc();
}

int launch_map_point_bad(hipStream_t st, const MapDev &M, int id)
{
    hipLaunchKernelGGL(k_map_point_bad, dim3(1), dim3(1), 0, st, M, id);
    return last_rc();
}

int launch_map_set_parent(hipStream_t st, const MapDev &M, int slot, int parent)
{
    hipLaunchKernelGGL(k_map_set_parent, dim3(1), dim3(1), 0, st, M, slot, parent);
    return last_rc();
}

int launch_map_resort(hipStream_t st, const MapDev &M, int epoch)
{
    const int bn = map_pow2(M.K);
    const size_t lds = map_lds(M.K, bn);
    if (map_attr((const void *)k_map_resort, lds)) return ORBG_EIO;
    hipLaunchKernelGGL(k_map_resort, dim3(M.K), dim3(MAP_T), lds, st, M, epoch, bn);
    return last_rc();
}

int launch_map_erase(hipStream_t st, const MapDev &M, int slot, int epoch)
{
    hipLaunchKernelGGL(k_map_erase, dim3(1), dim3(MAP_T), 0, st, M, slot, epoch);
    if (last_rc()) return ORBG_EIO;
    return launch_map_resort(st, M, epoch);
}

int launch_map_count(hipStream_t st, const MapDev &M)
{
    hipLaunchKernelGGL(k_map_count, dim3(1), dim3(MAP_T), 0, st, M);
    return last_rc();
}

int launch_map_rebuild(hipStream_t st, const MapDev &M, Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_rebuild", &ev);
    const int nt = (M.P + MAP_SCAN_TILE - 1) / MAP_SCAN_TILE;
    if (hipMemsetAsync(M.obs_cnt, 0, (size_t)M.P * 4, st) != hipSuccess) return ORBG_EIO;
    hipLaunchKernelGGL(k_map_obs<0>, dim3(M.K), dim3(MAP_T), 0, st, M);
    hipLaunchKernelGGL(k_map_scan_sum, dim3(nt), dim3(MAP_T), 0, st, M.obs_cnt, M.P, M.part);
    hipLaunchKernelGGL(k_map_scan_part, dim3(1), dim3(MAP_T), 0, st, M.part, nt);
    hipLaunchKernelGGL(k_map_scan_tile, dim3(nt), dim3(MAP_T), 0, st, M.obs_cnt, M.P, M.part,
                       M.obs_off);
    if (hipMemsetAsync(M.obs_cnt, 0, (size_t)M.P * 4, st) != hipSuccess) return ORBG_EIO;
    hipLaunchKernelGGL(k_map_obs<1>, dim3(M.K), dim3(MAP_T), 0, st, M);
    hipLaunchKernelGGL(k_map_obs<2>, dim3(M.K), dim3(MAP_T), 0, st, M);
    prof_end(prof, st, "map_rebuild", ev);
    return last_rc();
}

int launch_map_tree(hipStream_t st, const MapDev &M)
{
    if (hipMemsetAsync(M.child_head, 0xFF, (size_t)M.K * 4, st) != hipSuccess) return ORBG_EIO;
    const int g = (M.K + MAP_T - 1) / MAP_T;
    hipLaunchKernelGGL(k_map_tree_head, dim3(g), dim3(MAP_T), 0, st, M);
    hipLaunchKernelGGL(k_map_tree_next, dim3(g), dim3(MAP_T), 0, st, M);
    return last_rc();
}

int launch_map_update_connections(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                                  int epoch, Prof *prof)
{
    if (n <= 0) return ORBG_OK;
    const int bn = map_pow2(M.K);
    const size_t lds = map_lds(M.K, bn);
    if (map_attr((const void *)k_map_update, lds)) return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_update_connections", &ev);
    hipLaunchKernelGGL(k_map_update, dim3(n), dim3(MAP_T), lds, st, M, slots, epoch, bn);
    const int rc = launch_map_resort(st, M, epoch);
    prof_end(prof, st, "map_update_connections", ev);
    return rc ? rc : last_rc();
}

int launch_map_connected(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                         int32_t *conn, int conn_cap, int32_t *nconn)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_connected, dim3(n), dim3(MAP_T), 0, st, M, slots, conn, conn_cap,
                       nconn);
    return last_rc();
}

int launch_map_local_keyframes(hipStream_t st, const MapDev &M, int32_t *frame_points,
                               int frame_cap, const int32_t *counts, int nframes,
                               int32_t *local_kfs, int lkf_cap, int32_t *nlocal, int32_t *ref_kf,
                               Prof *prof)
{
    if (nframes <= 0) return ORBG_OK;
    const int bn = M.K;
    const size_t lds = map_lds(M.K, bn);
    if (map_attr((const void *)k_map_local_kfs, lds)) return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_local_keyframes", &ev);
    hipLaunchKernelGGL(k_map_local_kfs, dim3(nframes), dim3(MAP_T), lds, st, M, frame_points,
                       frame_cap, counts, local_kfs, lkf_cap, nlocal, ref_kf, bn);
    prof_end(prof, st, "map_local_keyframes", ev);
    return last_rc();
}

int launch_map_local_points(hipStream_t st, const MapDev &M, const int32_t *local_kfs, int lkf_cap,
                            const int32_t *nlocal, const int32_t *frame_points, int frame_cap,
                            const int32_t *counts, int nframes, int32_t *cnt, int32_t *ids,
                            orbg_map_point *mps, uint8_t *qdesc, int lp_cap, int32_t *nlp,
                            Prof *prof)
{
    if (nframes <= 0) return ORBG_OK;
    const int bn = map_pow2(frame_cap);
    const size_t lds = map_lds(M.K, bn);
    if (map_attr((const void *)k_map_lp_count, lds) || map_attr((const void *)k_map_lp_gather, lds))
        return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_local_points", &ev);
    hipLaunchKernelGGL(k_map_lp_count, dim3(lkf_cap, nframes), dim3(MAP_T), lds, st, M, local_kfs,
                       lkf_cap, nlocal, cnt, bn);
    hipLaunchKernelGGL(k_map_lp_gather, dim3(lkf_cap, nframes), dim3(MAP_T), lds, st, M, local_kfs,
                       lkf_cap, nlocal, cnt, frame_points, frame_cap, counts, ids, mps, qdesc,
                       lp_cap, nlp, bn);
    prof_end(prof, st, "map_local_points", ev);
    return last_rc();
}

int launch_map_normal_depth(hipStream_t st, const MapDev &M, const int32_t *ids, int n,
                            const MapScales &S, Prof *prof)
{
    if (n <= 0) return ORBG_OK;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_normal_depth", &ev);
    hipLaunchKernelGGL(k_map_normal_depth, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, ids,
                       n, S);
    prof_end(prof, st, "map_normal_depth", ev);
    return last_rc();
}

}  // namespace orbg
