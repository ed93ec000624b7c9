// map_create_kernels.hip -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:293-576) and
// the table side of LocalMapping::ProcessNewKeyFrame (:164-220) on the device Map, for gfx950.
//
// CreateNewMapPoints is a sequence over the neighbours, because each SearchForTriangulation
// reads has_mp of the current keyframe as the insertion of the neighbours before it left it:
//   k_cnp_neigh    once, one workgroup per neighbour: the first nn entries of the ordered list,
//                  the baseline test (stereo: against mb; monocular: against the neighbour's
//                  ComputeSceneMedianDepth(2), its depths compacted into LDS and sorted there,
//                  4 bytes per feature, kf_cap <= 8192: 32 KiB), the per-slot orbg_kf_camera
//                  (stored Tcw + attached intrinsics) of the current keyframe and the neighbours
//   k_tri_geometry once for the 20 pairs (triangulate_kernels.hip, unchanged)
//   per neighbour i:
//   k_cnp_pair     the abort latch, N / nfv and has_mp = (row[idx] >= 0) of both keyframes; a
//                  skipped neighbour becomes the empty pair (slot, slot) with N = 0
//   k_tri_match, k_triangulate   (mapping_kernels.hip / triangulate_kernels.hip, unchanged)
//   k_cnp_insert   one workgroup: ids by an exclusive scan over idx1 in 256-wide tiles, the
//                  records, both rows, the recent list; past a cap only a mark on the feature
//   k_cnp_finish   the id list for ComputeDistinctiveDescriptors / UpdateNormalAndDepth, d_out
// Nothing here synchronises; every length stays on the device.
#include "map_device.h"

#pragma clang fp contract(off)

namespace orbg {

__device__ __forceinline__ bool cnp_live(const MapDev &M, int s)
{
    return s >= 0 && s < M.K && (M.kf_flags[s] & MAP_KF_LIVE);
}

// N of slot s as every kernel of the sequence reads it
__device__ __forceinline__ int cnp_count(const MapDev &M, const MapAttach &A, int acap, int s)
{
    return min(min(max(A.kfs.counts[s], 0), acap), min(M.kf_n[s], M.cap));
}

// a float as a u32 whose unsigned order is the float order
__device__ __forceinline__ uint32_t cnp_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cnp_unkey(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ void cnp_camera(const MapDev &M, const MapGeom &G, const MapCreateWs &W, int s)
{
    orbg_kf_camera c = G.cams[s];
    for (int k = 0; k < 12; k++) c.Tcw[k] = M.kf_Tcw[(size_t)s * 12 + k];
    W.cams[s] = c;
}

__global__ __launch_bounds__(MAP_T) void k_cnp_neigh(MapDev M, MapAttach A, MapGeom G, MapCreateWs W,
                                                     int slot, int nn, int monocular,
                                                     const int32_t *nrecent, int32_t *neigh)
{
    __shared__ int scr[4];
    uint32_t *zk = (uint32_t *)map_smem;
    const int i = blockIdx.x;
    const bool live = cnp_live(M, slot);
    const bool pose = live && M.kf_pose[slot] != 0;
    const int cnt = pose ? min(min(M.nord[slot], nn), ORBG_CNP_MAX_NEIGH) : 0;
    if (i == 0 && threadIdx.x == 0) {
        W.hdr[CNP_HDR_NN] = cnt;
        W.hdr[CNP_HDR_NNEW] = 0;
        W.hdr[CNP_HDR_NEED] = 0;
        W.hdr[CNP_HDR_BITS] = !live ? ORBG_CNP_DEAD : !pose ? ORBG_CNP_NO_POSE : 0;
        W.hdr[CNP_HDR_ABORT] = 0;
        W.hdr[CNP_HDR_REC0] = max(nrecent[0], 0);
        if (pose) cnp_camera(M, G, W, slot);
    }
    if (i == 0)
        for (int k = threadIdx.x; k < W.acap; k += MAP_T) W.virt[k] = 0;
    const int nb = i < cnt ? (int)M.ord_slot[(size_t)slot * M.K + i] : -1;
    int st = 0;
    if (nb >= 0) {
        if (!cnp_live(M, nb) || !M.kf_pose[nb]) {
            st = 3;
        } else {
            // cv::norm(Ow2 - Ow1) on CV_32F: the squares summed in double
            double sq = 0.0;
            for (int k = 0; k < 3; k++) {
                const float d = M.kf_centre[nb * 3 + k] - M.kf_centre[slot * 3 + k];
                sq += (double)d * (double)d;
            }
            const float baseline = (float)sqrt(sq);
            if (!monocular) {
                if (baseline < G.cams[nb].mb) st = 1;
            } else {
                // KeyFrame::ComputeSceneMedianDepth(2): z of every row entry, sorted
                const int n2 = min(M.kf_n[nb], M.cap);
                const float *T = M.kf_Tcw + (size_t)nb * 12;
                const float r0 = T[8], r1 = T[9], r2 = T[10], tz = T[11];
                int carry = 0;
                for (int base = 0; base < n2; base += MAP_T) {  // uniform trip count
                    const int k = base + threadIdx.x;
                    int p = -1;
                    if (k < n2) p = M.kf_points[(size_t)nb * M.cap + k];
                    if (p >= M.P) p = -1;
                    int total;
                    const int ex = block_scan(p >= 0, scr, &total);
                    if (p >= 0) {
                        const orbg_map_point r = M.mp[p];
                        double t = (double)r0 * (double)r.x;  // Mat::dot on CV_32F: double, in order
                        t += (double)r1 * (double)r.y;
                        t += (double)r2 * (double)r.z;
                        zk[carry + ex] = cnp_key((float)(t + (double)tz));
                    }
                    carry += total;
                }
                if (carry == 0) {
                    st = 3;
                } else {
                    int n2p = 1;
                    while (n2p < carry) n2p <<= 1;
                    __syncthreads();
                    for (int k = carry + threadIdx.x; k < n2p; k += MAP_T) zk[k] = 0u;
                    lds_sort_desc(zk, n2p);
                    // ascending index (n - 1) / 2 of the n depths
                    const float median = cnp_unkey(zk[carry - 1 - (carry - 1) / 2]);
                    const float ratio = baseline / median;
                    if ((double)ratio < 0.01) st = 1;
                }
            }
            if (threadIdx.x == 0) cnp_camera(M, G, W, nb);
        }
    }
    if (threadIdx.x == 0) {
        neigh[i] = nb;
        W.nstat[i] = st;
        W.kf1[i] = slot;
        W.kf2[i] = (nb >= 0 && st == 0) ? nb : slot;
    }
}

__global__ __launch_bounds__(MAP_T) void k_cnp_pair(MapDev M, MapAttach A, MapCreateWs W, int slot,
                                                    int i, const int32_t *abort)
{
    __shared__ int skip, nbs;
    if (threadIdx.x == 0) {
        int ab = W.hdr[CNP_HDR_ABORT];
        if (i > 0 && !ab && abort && *(const volatile int32_t *)abort != 0) {
            ab = 1;
            W.hdr[CNP_HDR_ABORT] = 1;
        }
        int st = W.nstat[i];
        const bool listed = i < W.hdr[CNP_HDR_NN];
        if (listed && ab) {
            st = 2;
            W.nstat[i] = 2;
            W.kf2[i] = slot;
        }
        skip = !listed || st != 0;
        nbs = W.kf2[i];
        if (skip) {
            W.counts[slot] = 0;
            W.nfv[slot] = 0;
        }
    }
    __syncthreads();
    if (skip) return;
    const int ks[2] = {slot, nbs};
    for (int q = 0; q < 2; q++) {
        const int s = ks[q];
        const int n = cnp_count(M, A, W.acap, s);
        if (threadIdx.x == 0) {
            W.counts[s] = n;
            W.nfv[s] = min(max(A.kfs.nfv[s], 0), W.acap);
        }
        // a feature of the current keyframe whose point a cap left out stays out of the later
        // searches, so that CNP_HDR_NEED counts what a large enough cap would have created
        for (int k = threadIdx.x; k < W.acap; k += MAP_T)
            W.has_mp[(size_t)s * W.acap + k] =
                k >= n || M.kf_points[(size_t)s * M.cap + k] >= 0 || (q == 0 && W.virt[k]);
    }
}

__global__ __launch_bounds__(MAP_T) void k_cnp_insert(MapDev M, MapCreateWs W, int slot, int i,
                                                      int current_kf_id, int first_id,
                                                      int32_t *recent, int recent_cap,
                                                      int32_t *nrecent, int32_t *nmatches,
                                                      int32_t *nnew, int8_t *tri_status)
{
    __shared__ int scr[4];
    const bool skip = i >= W.hdr[CNP_HDR_NN] || W.nstat[i] != 0;
    const int nb = W.kf2[i];
    const int n1 = skip ? 0 : W.counts[slot], n2 = skip ? 0 : W.counts[nb];
    const int need0 = W.hdr[CNP_HDR_NEED], rec0 = W.hdr[CNP_HDR_REC0];
    const int room_p = max(M.P - first_id, 0), room_r = max(recent_cap - rec0, 0);
    const int room = min(room_p, room_r);
    int carry = 0;
    for (int base = 0; base < n1; base += MAP_T) {  // uniform trip count
        const int k = base + threadIdx.x;
        int j = -1;
        if (k < n1 && W.tst[k] == ORBG_TRI_NEW) j = W.match[k];
        if (j >= n2) j = -1;
        int total;
        const int ord = need0 + carry + block_scan(j >= 0, scr, &total);
        if (j >= 0 && ord < room) {
            const int id = first_id + ord;
            orbg_map_point r{};
            r.x = W.x3d[3 * k];
            r.y = W.x3d[3 * k + 1];
            r.z = W.x3d[3 * k + 2];
            r.flags = ORBG_MP_VALID;
            M.mp[id] = r;
            uint4 *md = (uint4 *)(M.mdesc + (size_t)id * 32);
            md[0] = make_uint4(0, 0, 0, 0);
            md[1] = make_uint4(0, 0, 0, 0);
            M.mp_ref[id] = slot;
            M.mp_first[id] = current_kf_id;
            M.mp_visible[id] = 1;
            M.mp_found[id] = 1;
            M.mp_replaced[id] = -1;
            M.mp_corr_kf[id] = 0;
            M.mp_corr_ref[id] = 0;
            M.mp_corr_slot[id] = 0;
            M.mp_gba[id] = 0;
            M.kf_points[(size_t)slot * M.cap + k] = id;
            // two idx1 may hold the same idx2 (vbMatched2 is never set): the later one keeps it
            atomicMax(&M.kf_points[(size_t)nb * M.cap + j], id);
            recent[rec0 + ord] = id;
        } else if (j >= 0) {
            W.virt[k] = 1;
        }
        carry += total;
    }
    if (tri_status)
        for (int k = threadIdx.x; k < M.cap; k += MAP_T)
            tri_status[(size_t)i * M.cap + k] = k < n1 ? W.tst[k] : (int8_t)ORBG_TRI_NONE;
    if (threadIdx.x == 0) {
        const int need = need0 + carry;
        const int made0 = min(need0, room), made = min(need, room);
        W.hdr[CNP_HDR_NEED] = need;
        W.hdr[CNP_HDR_NNEW] = made;
        if (need > room_p) W.hdr[CNP_HDR_BITS] |= ORBG_CNP_POINT_RANGE;
        if (need > room_r) W.hdr[CNP_HDR_BITS] |= ORBG_CNP_RECENT_RANGE;
        nmatches[i] = skip ? 0 : W.nm[0];
        nnew[i] = made - made0;
        if (!(W.hdr[CNP_HDR_BITS] & (ORBG_CNP_DEAD | ORBG_CNP_NO_POSE))) nrecent[0] = rec0 + made;
    }
}

__global__ __launch_bounds__(MAP_T) void k_cnp_finish(MapDev M, MapCreateWs W, int first_id,
                                                      int32_t *neigh_status, int32_t *out)
{
    const int made = W.hdr[CNP_HDR_NNEW];
    for (int k = threadIdx.x; k < M.cap; k += MAP_T) W.ids[k] = k < made ? first_id + k : -1;
    if (threadIdx.x < ORBG_CNP_MAX_NEIGH)
        neigh_status[threadIdx.x] = (int)threadIdx.x < W.hdr[CNP_HDR_NN] ? W.nstat[threadIdx.x] : 0;
    if (threadIdx.x == 0) {
        W.ids[M.cap] = min(made, M.cap);
        out[0] = W.hdr[CNP_HDR_NN];
        out[1] = made;
        out[2] = W.hdr[CNP_HDR_NEED];
        out[3] = W.hdr[CNP_HDR_BITS];
    }
}

// ProcessNewKeyFrame: W.row = the row with a bad or out-of-range id as -1, W.centre, the
// in_keyframe entries appended to recent, the others into W.ids (both in feature order)
__global__ __launch_bounds__(MAP_T) void k_pnk_prepare(MapDev M, MapCreateWs W, int slot,
                                                       const int32_t *point_ids, int n,
                                                       const float *Tcw, int mnid, int flags,
                                                       const uint8_t *in_keyframe, int32_t *recent,
                                                       int recent_cap, int32_t *nrecent,
                                                       int32_t *out)
{
    __shared__ int scr[4];
    const int rec0 = max(nrecent[0], 0);
    int cr = 0, cu = 0;
    for (int base = 0; base < M.cap; base += MAP_T) {  // uniform trip count
        const int k = base + threadIdx.x;
        int p = -1;
        if (k < n) p = point_ids[k];
        if (!map_point_ok(M, p)) p = -1;
        if (k < M.cap) W.row[k] = p;
        const bool inkf = p >= 0 && in_keyframe && in_keyframe[k];
        int tr, tu;
        const int er = block_scan(inkf, scr, &tr);
        const int eu = block_scan(p >= 0 && !inkf, scr, &tu);
        if (inkf && rec0 + cr + er < recent_cap) recent[rec0 + cr + er] = p;
        if (p >= 0 && !inkf) W.ids[cu + eu] = p;
        cr += tr;
        cu += tu;
    }
    __syncthreads();
    for (int k = cu + threadIdx.x; k < M.cap; k += MAP_T) W.ids[k] = -1;
    if (threadIdx.x == 0) {
        float T[12];
        for (int k = 0; k < 12; k++) T[k] = Tcw[k];
        loop_centre(T, W.centre);
        W.ids[M.cap] = cu;
        W.hdr[CNP_HDR_SLOT] = slot;
        W.hdr[CNP_HDR_N] = n;
        W.hdr[CNP_HDR_FLAGS] = flags;
        W.hdr[CNP_HDR_MNID] = mnid;
        const int made = min(cr, max(recent_cap - rec0, 0));
        nrecent[0] = rec0 + made;
        out[0] = made;
        out[1] = cu;
        out[2] = cr;
        out[3] = cr > made ? ORBG_CNP_RECENT_RANGE : 0;
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_cnp_neighbours(hipStream_t st, const MapDev &M, const MapAttach &A, const MapGeom &G,
                              const MapCreateWs &W, int slot, int monocular, const int32_t *nrecent,
                              int32_t *neigh)
{
    const size_t lds = (size_t)map_pow2(M.cap) * 4;  // kf_cap <= 8192: at most 32 KiB
    hipLaunchKernelGGL(k_cnp_neigh, dim3(ORBG_CNP_MAX_NEIGH), dim3(MAP_T), lds, st, M, A, G, W, slot,
                       monocular ? 20 : 10, monocular, nrecent, neigh);
    return last_rc();
}

int launch_map_cnp_pair(hipStream_t st, const MapDev &M, const MapAttach &A, const MapCreateWs &W,
                        int slot, int i, const int32_t *abort)
{
    hipLaunchKernelGGL(k_cnp_pair, dim3(1), dim3(MAP_T), 0, st, M, A, W, slot, i, abort);
    return last_rc();
}

int launch_map_cnp_insert(hipStream_t st, const MapDev &M, const MapCreateWs &W, int slot, int i,
                          int current_kf_id, int first_id, int32_t *recent, int recent_cap,
                          int32_t *nrecent, int32_t *nmatches, int32_t *nnew, int8_t *tri_status)
{
    hipLaunchKernelGGL(k_cnp_insert, dim3(1), dim3(MAP_T), 0, st, M, W, slot, i, current_kf_id,
                       first_id, recent, recent_cap, nrecent, nmatches, nnew, tri_status);
    return last_rc();
}

int launch_map_cnp_finish(hipStream_t st, const MapDev &M, const MapCreateWs &W, int first_id,
                          int32_t *neigh_status, int32_t *out)
{
    hipLaunchKernelGGL(k_cnp_finish, dim3(1), dim3(MAP_T), 0, st, M, W, first_id, neigh_status, out);
    return last_rc();
}

int launch_map_pnk_prepare(hipStream_t st, const MapDev &M, const MapCreateWs &W, int slot,
                           const int32_t *point_ids, int n, const float *Tcw, int mnid, int flags,
                           const uint8_t *in_keyframe, int32_t *recent, int recent_cap,
                           int32_t *nrecent, int32_t *out)
{
    hipLaunchKernelGGL(k_pnk_prepare, dim3(1), dim3(MAP_T), 0, st, M, W, slot, point_ids, n, Tcw, mnid,
                       flags, in_keyframe, recent, recent_cap, nrecent, out);
    return last_rc();
}

}  // namespace orbg
