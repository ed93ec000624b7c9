// map_gba_kernels.hip -- Optimizer::GlobalBundleAdjustemnt on the covisibility Map
// (src/Optimizer.cc:105-320): the window the reference builds from GetAllKeyFrames() /
// GetAllMapPoints() (:113-246) and the store of the optimised estimates (:273-318); and the map
// update of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:1056-1116).
//
// The window.  Every list is fixed by the table alone, never by the order in which threads run:
//   k_gba_kfs      the vertex keyframes: the slots that are live and not bad, ascending (ordered
//                  compaction), their SE3Quat (Converter::toSE3Quat), fixed iff the stored mnId
//                  is 0.
//   k_gba_pcount   one thread per point id: the edges of a good point = its observers in the
//                  observation index that are live and not bad.  A good point without one is
//                  left out and counted (vbNotIncludedMP; an integer atomicAdd).
//   k_gba_pscan    one workgroup, tiles of MAP_SCAN_TILE ids with two carries: a point's window
//                  position and its first edge; the ordered gather of ids and positions; the
//                  counts and the status.
//   k_gba_edges    one thread per window point: its edges in ascending observer slot.
// The reference's other test on an edge, pKF->mnId > maxKFid (:184), can never hold for a
// keyframe that is not bad: maxKFid is the largest mnId over exactly those keyframes (:140-152).
// The store.
//   k_gba_store    a thread per window keyframe and per window point.  loop_kf == 0: SetPose
//                  (Converter::toCvMat(SE3Quat)), the attached cameras' Tcw, SetWorldPos;
//                  otherwise mTcwGBA / mPosGBA and both mnBAGlobalForKF.  A keyframe that has
//                  gone bad or dead and a point that has gone bad are skipped (:279, :303).
//                  UpdateNormalAndDepth is map_kernels.hip's, over the current index.
// The update.  The reference walks the spanning tree breadth first from mvpKeyFrameOrigins; a
// keyframe global BA did not reach gets mTcwGBA = (Tcw_child * Twc_parent) * mTcwGBA_parent, where
// both poses are the ones from before the walk (a keyframe's own SetPose comes after its
// children were handled).  So the result is a function of the state before the call:
//   k_gba_origins  the origins' marks and checks.
//   k_gba_walk     one thread per slot walks its parents up to an origin (a dead slot ends the
//                  walk: not visited; more than K steps: a cycle) and notes how many parents up
//                  its nearest ancestor that carries loop_kf is, itself included.
//   k_gba_chain    one workgroup, level by level: a visited slot d parents below that ancestor
//                  takes the staged result of its parent (level d - 1) into the staged gT.  As
//                  many levels as the longest run of keyframes outside the BA; poses and
//                  centres are not written here, so every product reads the ones from before.
//   k_gba_apply    per visited slot: mTcwBefGBA = Tcw, the staged mTcwGBA and mnBAGlobalForKF,
//                  SetPose(mTcwGBA), its entry of the attached cameras.
//   k_gba_points   per good point: mPosGBA, or the move of k_gba_correct_points (bsolve_kernels.hip)
//                  with the reference keyframe's mTcwBefGBA and GetPoseInverse() after the walk.
// The counters are integer atomics; no result depends on thread order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "map_ba_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

__device__ __forceinline__ bool gba_live(const MapDev &M, int s)
{
    return s >= 0 && s < M.K && (M.kf_flags[s] & MAP_KF_LIVE);
}

// ---------------------------------------------------------------------------
// the window
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_gba_kfs(MapDev M, MapGbaWs W, int32_t *kf_slots,
                                                   orbg_pose *poses, int pose_cap)
{
    __shared__ int scr[16];
    __shared__ int nopose;
    if (threadIdx.x == 0) nopose = 0;
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += lba_kf_good(M, t);
    int total;
    int pos = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++) {
        if (!lba_kf_good(M, t)) {
            W.pidx[t] = -1;
            continue;
        }
        const int fixed = M.kf_mnid[t] == 0;
        W.pidx[t] = pos;
        W.fixed[pos] = fixed;
        if (pos < pose_cap) {
            kf_slots[pos] = t;
            lba_se3quat(M.kf_Tcw + (size_t)t * 12, fixed, &poses[pos]);
        }
        if (!M.kf_pose[t]) nopose = 1;  // every writer stores 1
        pos++;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        W.hdr[GBA_HDR_NPOSE] = total;
        W.hdr[GBA_HDR_NPOINT] = 0;
        W.hdr[GBA_HDR_NEDGE] = 0;
        W.hdr[GBA_HDR_LEFT] = 0;
        W.hdr[GBA_HDR_BITS] = nopose ? ORBG_LBA_NO_POSE : 0;
    }
}

__global__ __launch_bounds__(MAP_T) void k_gba_pcount(MapDev M, MapGbaWs W)
{
    const int p = blockIdx.x * MAP_T + threadIdx.x;
    if (p >= M.P) return;
    int ne = 0;
    if (M.mp[p].flags & ORBG_MP_VALID) {
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) ne += lba_kf_good(M, (int)(M.obs[e] >> 16));
        if (ne == 0) atomicAdd(&W.hdr[GBA_HDR_LEFT], 1);
    }
    W.ne[p] = ne;
}

__global__ __launch_bounds__(MAP_T) void k_gba_pscan(MapDev M, MapGbaWs W, int32_t *point_ids,
                                                     double *points, int pose_cap, int point_cap,
                                                     int edge_cap, int32_t *counts, int32_t *status)
{
    __shared__ int scr[16];
    constexpr int PER = MAP_SCAN_TILE / MAP_T;
    int carry_p = 0, carry_e = 0;
    for (int b0 = 0; b0 < M.P; b0 += MAP_SCAN_TILE) {  // uniform trip count
        const int base = b0 + threadIdx.x * PER;
        int v[PER], ce = 0, cp = 0;
        for (int k = 0; k < PER; k++) {
            v[k] = base + k < M.P ? W.ne[base + k] : 0;
            ce += v[k];
            cp += v[k] > 0;
        }
        int tot_e, tot_p;
        int run_e = carry_e + block_scan(ce, scr, &tot_e);
        int run_p = carry_p + block_scan(cp, scr, &tot_p);
        for (int k = 0; k < PER; k++) {
            const int p = base + k;
            if (p >= M.P) break;
            if (v[k] == 0) {
                W.pi[p] = -1;
                continue;
            }
            W.pi[p] = run_p;
            W.eoff[p] = run_e;
            if (run_p < point_cap) {
                const orbg_map_point mp = M.mp[p];
                point_ids[run_p] = p;
                points[3 * (size_t)run_p] = (double)mp.x;
                points[3 * (size_t)run_p + 1] = (double)mp.y;
                points[3 * (size_t)run_p + 2] = (double)mp.z;
            }
            run_p++;
            run_e += v[k];
        }
        carry_p += tot_p;
        carry_e += tot_e;
    }
    if (threadIdx.x == 0) {
        W.hdr[GBA_HDR_NPOINT] = carry_p;
        W.hdr[GBA_HDR_NEDGE] = carry_e;
        int bits = W.hdr[GBA_HDR_BITS];
        if (W.hdr[GBA_HDR_NPOSE] > pose_cap || carry_p > point_cap || carry_e > edge_cap)
            bits |= ORBG_LBA_RANGE;
        W.hdr[GBA_HDR_BITS] = bits;
        for (int k = 0; k < 4; k++) counts[k] = W.hdr[k];
        status[0] = bits;
        status[1] = status[2] = status[3] = 0;
    }
}

__global__ __launch_bounds__(MAP_T) void k_gba_edges(MapDev M, MapAttach A, MapGbaWs W, int robust,
                                                     orbg_edge *edges, int32_t *edge_feat,
                                                     int edge_cap, MapLbaConst C, int32_t *status)
{
    const int p = blockIdx.x * MAP_T + threadIdx.x;
    if (p >= M.P) return;
    const int i = W.pi[p];
    if (i < 0) return;
    int at = W.eoff[p];
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        const uint32_t ob = M.obs[e];
        const int u = (int)(ob >> 16), j = (int)(ob & 0xFFFFu);
        if (!lba_kf_good(M, u)) continue;
        const int k = at++;
        if (k >= edge_cap) continue;
        orbg_edge E;
        if (!lba_fill_edge(A, C, u, j, i, W.pidx[u], robust, &E)) atomicOr(&status[0], ORBG_LBA_FEATURE);
        edges[k] = E;
        edge_feat[k] = j;
    }
}

// ---------------------------------------------------------------------------
// the store
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_gba_store(MapDev M, MapGbaWs W, const int32_t *counts,
                                                     const int32_t *kf_slots, int pose_cap,
                                                     const int32_t *point_ids, int point_cap,
                                                     const orbg_pose *poses, const double *points,
                                                     int loop_kf, orbg_frustum_camera *cams_out,
                                                     int32_t *out)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i < min(counts[0], pose_cap)) {
        const int s = kf_slots[i];
        if (s >= 0 && s < M.K && lba_kf_good(M, s)) {
            float T[12];
            lba_tcw(poses[i], T);
            if (loop_kf == 0) {
                for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = T[k];
                loop_centre(T, M.kf_centre + s * 3);
                M.kf_pose[s] = 1;
                if (cams_out)
                    for (int k = 0; k < 12; k++) cams_out[s].Tcw[k] = T[k];
            } else {
                for (int k = 0; k < 12; k++) M.kf_TcwGBA[(size_t)s * 12 + k] = T[k];
                M.kf_gba[s] = loop_kf;
            }
            atomicAdd(&out[0], 1);
        }
    }
    if (i < min(point_cap, M.P)) {
        int p = i < counts[1] ? point_ids[i] : -1;
        if (!map_point_ok(M, p)) p = -1;
        W.ids[i] = p;
        if (p >= 0) {
            const float x = (float)points[3 * (size_t)i], y = (float)points[3 * (size_t)i + 1];
            const float z = (float)points[3 * (size_t)i + 2];
            if (loop_kf == 0) {
                M.mp[p].x = x;
                M.mp[p].y = y;
                M.mp[p].z = z;
            } else {
                M.mp_posGBA[3 * (size_t)p] = x;
                M.mp_posGBA[3 * (size_t)p + 1] = y;
                M.mp_posGBA[3 * (size_t)p + 2] = z;
                M.mp_gba[p] = loop_kf;
            }
            atomicAdd(&out[1], 1);
        }
    }
}

// ---------------------------------------------------------------------------
// the update
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_gba_origins(MapDev M, MapGbaWs W, const int32_t *origins,
                                                       int n, int loop_kf, int32_t *status)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= n) return;
    const int s = origins[i];
    if (!gba_live(M, s) || !M.kf_pose[s] || M.kf_gba[s] != loop_kf)
        atomicOr(&status[0], ORBG_GBA_ORIGIN);
    else
        W.org[s] = 1;  // every writer stores 1
}

// vis[s]: 0 = not visited, else 1 + the number of parents up to the nearest ancestor that carries
// loop_kf (s itself: 1)
__global__ __launch_bounds__(MAP_T) void k_gba_walk(MapDev M, MapGbaWs W, int loop_kf,
                                                    int32_t *status)
{
    const int s = blockIdx.x * MAP_T + threadIdx.x;
    if (s >= M.K) return;
    int vis = 0, da = -1;
    if (gba_live(M, s)) {
        int u = s;
        for (int steps = 0;; steps++) {
            if (steps > M.K) {
                atomicOr(&status[0], ORBG_GBA_CYCLE);
                break;
            }
            if (da < 0 && M.kf_gba[u] == loop_kf) da = steps;
            if (W.org[u]) {
                vis = 1;
                break;
            }
            u = M.parent[u];
            if (!gba_live(M, u)) break;
        }
    }
    if (vis && da < 0) vis = 0;  // an origin carries loop_kf, or it is no origin
    if (vis && !M.kf_pose[s]) atomicOr(&status[0], ORBG_GBA_NO_POSE);
    W.vis[s] = vis ? 1 + da : 0;
}

// The chains below the BA, level by level in one workgroup: a slot d parents below its marked
// ancestor takes its parent's result of level d - 1 (the parent is on the same path, so it is
// one level up).  Poses and centres are the ones from before the call: nothing here writes them.
__global__ __launch_bounds__(MAP_T) void k_gba_chain(MapDev M, MapGbaWs W, const int32_t *status)
{
    __shared__ int levels;
    if (threadIdx.x == 0) levels = 0;
    __syncthreads();
    if (status[0]) return;  // uniform: the walk has finished
    int m = 0;
    for (int s = threadIdx.x; s < M.K; s += MAP_T) m = max(m, W.vis[s] - 1);
    atomicMax(&levels, m);
    __syncthreads();
    const int n = levels;
    for (int level = 1; level <= n; level++) {  // uniform trip count
        for (int s = threadIdx.x; s < M.K; s += MAP_T) {
            if (W.vis[s] - 1 != level) continue;
            const int par = M.parent[s];
            const float *Gp = (W.vis[par] == 1 ? M.kf_TcwGBA : W.gT) + (size_t)par * 12;
            float Tcc[12], N[12];
            // Tchildc = pChild->GetPose() * Twc; mTcwGBA = Tchildc * pKF->mTcwGBA
            pose_mul(M.kf_Tcw + (size_t)s * 12, M.kf_Tcw + (size_t)par * 12, true,
                     M.kf_centre + par * 3, Tcc);
            pose_mul(Tcc, Gp, false, nullptr, N);
            for (int k = 0; k < 12; k++) W.gT[(size_t)s * 12 + k] = N[k];
        }
        __syncthreads();  // level d is in memory before level d + 1 reads it
    }
}

__global__ __launch_bounds__(MAP_T) void k_gba_apply(MapDev M, MapGbaWs W, int loop_kf,
                                                     const int32_t *status,
                                                     orbg_frustum_camera *cams_out, int32_t *out)
{
    const int s = blockIdx.x * MAP_T + threadIdx.x;
    if (s >= M.K || status[0]) return;
    const int v = W.vis[s];
    if (!v) return;
    float T[12];
    for (int k = 0; k < 12; k++) M.kf_TcwBef[(size_t)s * 12 + k] = M.kf_Tcw[(size_t)s * 12 + k];
    if (v > 1) {
        for (int k = 0; k < 12; k++) M.kf_TcwGBA[(size_t)s * 12 + k] = W.gT[(size_t)s * 12 + k];
        M.kf_gba[s] = loop_kf;
        atomicAdd(&out[1], 1);
    }
    for (int k = 0; k < 12; k++) T[k] = M.kf_TcwGBA[(size_t)s * 12 + k];
    for (int k = 0; k < 12; k++) M.kf_Tcw[(size_t)s * 12 + k] = T[k];
    loop_centre(T, M.kf_centre + s * 3);
    M.kf_pose[s] = 1;
    if (cams_out)
        for (int k = 0; k < 12; k++) cams_out[s].Tcw[k] = T[k];
    atomicAdd(&out[0], 1);
}

__global__ __launch_bounds__(MAP_T) void k_gba_points(MapDev M, MapGbaWs W, int loop_kf,
                                                      const int32_t *status, int32_t *out)
{
    const int p = blockIdx.x * MAP_T + threadIdx.x;
    if (p >= M.P || status[0]) return;
    if (!(M.mp[p].flags & ORBG_MP_VALID)) return;
    if (M.mp_gba[p] == loop_kf) {
        M.mp[p].x = M.mp_posGBA[3 * (size_t)p];
        M.mp[p].y = M.mp_posGBA[3 * (size_t)p + 1];
        M.mp[p].z = M.mp_posGBA[3 * (size_t)p + 2];
        atomicAdd(&out[2], 1);
        return;
    }
    const int r = M.mp_ref[p];
    if (!gba_live(M, r)) {  // the reference dereferences it
        atomicAdd(&out[4], 1);
        return;
    }
    if (!W.vis[r]) {
        // carries loop_kf from an earlier call, not visited in this one: its mTcwBefGBA is stale
        if (M.kf_gba[r] == loop_kf) atomicAdd(&out[4], 1);
        return;
    }
    // Xc = Rcw X + tcw with mTcwBefGBA, X' = Rwc Xc + twc with GetPoseInverse(): two cv::gemm
    const float *B = M.kf_TcwBef + (size_t)r * 12, *T = M.kf_Tcw + (size_t)r * 12;
    const float *O = M.kf_centre + r * 3;
    const float x[3] = {M.mp[p].x, M.mp[p].y, M.mp[p].z};
    float xc[3], y[3];
    for (int a = 0; a < 3; a++) {
        double t = 0.0;
        for (int k = 0; k < 3; k++) t += (double)B[4 * a + k] * (double)x[k];
        t += (double)B[4 * a + 3];
        xc[a] = (float)t;
    }
    for (int a = 0; a < 3; a++) {
        double t = 0.0;
        for (int k = 0; k < 3; k++) t += (double)T[4 * k + a] * (double)xc[k];
        t += (double)O[a];
        y[a] = (float)t;
    }
    M.mp[p].x = y[0];
    M.mp[p].y = y[1];
    M.mp[p].z = y[2];
    atomicAdd(&out[3], 1);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_gba_window(hipStream_t st, const MapDev &M, const MapAttach &A, const MapGbaWs &W,
                          int robust, const MapLbaWindow &O, const MapLbaConst &C, int32_t *status,
                          Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_gba_window", &ev);
    const int gp = (M.P + MAP_T - 1) / MAP_T;
    hipLaunchKernelGGL(k_gba_kfs, dim3(1), dim3(MAP_T), 0, st, M, W, O.kf_slots, O.poses, O.pose_cap);
    hipLaunchKernelGGL(k_gba_pcount, dim3(gp), dim3(MAP_T), 0, st, M, W);
    hipLaunchKernelGGL(k_gba_pscan, dim3(1), dim3(MAP_T), 0, st, M, W, O.point_ids, O.points,
                       O.pose_cap, O.point_cap, O.edge_cap, O.counts, status);
    hipLaunchKernelGGL(k_gba_edges, dim3(gp), dim3(MAP_T), 0, st, M, A, W, robust, O.edges,
                       O.edge_feat, O.edge_cap, C, status);
    prof_end(prof, st, "map_gba_window", ev);
    return last_rc();
}

int launch_map_gba_store(hipStream_t st, const MapDev &M, const MapGbaWs &W, const int32_t *counts,
                         const int32_t *kf_slots, int pose_cap, const int32_t *point_ids,
                         int point_cap, const orbg_pose *poses, const double *points, int loop_kf,
                         orbg_frustum_camera *cams_out, int32_t *out, Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_gba_store", &ev);
    const int n = std::max(std::max(std::min(pose_cap, M.K), std::min(point_cap, M.P)), 1);
    hipLaunchKernelGGL(k_gba_store, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, W, counts,
                       kf_slots, std::min(pose_cap, M.K), point_ids, point_cap, poses, points,
                       loop_kf, cams_out, out);
    prof_end(prof, st, "map_gba_store", ev);
    return last_rc();
}

int launch_map_gba_update(hipStream_t st, const MapDev &M, const MapGbaWs &W, const int32_t *origins,
                          int norigins, int loop_kf, orbg_frustum_camera *cams_out, int32_t *out,
                          int32_t *status, Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_gba_update", &ev);
    const int gk = (M.K + MAP_T - 1) / MAP_T, gp = (M.P + MAP_T - 1) / MAP_T;
    if (hipMemsetAsync(W.org, 0, (size_t)M.K * 4, st) != hipSuccess) return ORBG_EIO;
    if (norigins > 0)
        hipLaunchKernelGGL(k_gba_origins, dim3((norigins + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                           W, origins, norigins, loop_kf, status);
    hipLaunchKernelGGL(k_gba_walk, dim3(gk), dim3(MAP_T), 0, st, M, W, loop_kf, status);
    hipLaunchKernelGGL(k_gba_chain, dim3(1), dim3(MAP_T), 0, st, M, W, status);
    hipLaunchKernelGGL(k_gba_apply, dim3(gk), dim3(MAP_T), 0, st, M, W, loop_kf, status, cams_out, out);
    hipLaunchKernelGGL(k_gba_points, dim3(gp), dim3(MAP_T), 0, st, M, W, loop_kf, status, out);
    prof_end(prof, st, "map_gba_update", ev);
    return last_rc();
}

}  // namespace orbg
