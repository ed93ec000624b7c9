// map_cull_kernels.hip -- the functions of LocalMapping's loop that edit the covisibility Map's
// observation table on gfx950: KeyFrame::SetBadFlag (src/KeyFrame.cc:622-720, with
// MapPoint::EraseObservation / SetBadFlag, src/MapPoint.cc:159-232), LocalMapping::
// KeyFrameCulling (src/LocalMapping.cc:804-877) and MapPointCulling (:227-270).
//
// Inside one call observations only disappear, so the point -> observations index built at
// the call's start stays valid as a superset: an entry (u, j) of point p counts if and only if
// slot u is live and kf_points[u][j] == p still holds (cull_obs).  The callers mark the index
// stale when the call ends.
//
//   k_cull_score     one workgroup per entry of the culling slot's ordered list: nMPs and
//                    nRedundantObservations of that keyframe as the map stands when the call
//                    starts, a lane per feature, the point's observers walked through the index.
//   k_cull_sequence  one workgroup walks the list in order.  An entry keeps its start score
//                    unless an erasure of this call marked its row (row_touch: it held a point
//                    whose Observations() changed); only then it is scored again.  A redundant
//                    entry is erased at once by map_set_bad, so the result is the sequential one.
//   map_set_bad      SetBadFlag by one workgroup: the EraseConnection loop (as k_map_erase), a
//                    lane per feature of the row for EraseObservation (nObs, mpRefKF, the point
//                    going bad and leaving every row), the re-sort of the children's rows this
//                    call dirtied (every other dirty row waits for k_map_resort), then the
//                    spanning-tree repair: per round a max-reduction over weight + 1, inverted
//                    child position, inverted list position = the first greatest in the
//                    reference's iteration order.
//   k_point_cull / k_point_compact
//                    MapPointCulling: a thread per recent point (the points are distinct, so
//                    the chain's decisions do not depend on one another), then the ordered
//                    compaction of the list by one workgroup.
// No result depends on thread order: the atomics are integer counters and maxima.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

// LDS of the one-workgroup kernels: keys [K] u32, srt [bn] u32, child [K] i32, cand [K / 32] u32,
// best u64, scr [32] i32
static __host__ __device__ inline size_t cull_off_child(int K, int bn) { return map_off_b(K) + (size_t)bn * 4; }
static __host__ __device__ inline size_t cull_off_cand(int K, int bn) { return cull_off_child(K, bn) + (size_t)K * 4; }
static __host__ __device__ inline size_t cull_off_best(int K, int bn)
{
    return (cull_off_cand(K, bn) + (size_t)((K + 31) / 32) * 4 + 15) & ~(size_t)15;
}
static __host__ __device__ inline size_t cull_off_scr(int K, int bn) { return cull_off_best(K, bn) + 16; }
static inline size_t cull_lds(int K, int bn) { return cull_off_scr(K, bn) + 32 * 4; }

struct CullLds {
    uint32_t *keys, *srt, *cand;
    int32_t *child;
    unsigned long long *best;
    int *scr;
};

__device__ __forceinline__ CullLds cull_lds_of(int K, int bn)
{
    CullLds L;
    L.keys = (uint32_t *)map_smem;
    L.srt = (uint32_t *)(map_smem + map_off_b(K));
    L.child = (int32_t *)(map_smem + cull_off_child(K, bn));
    L.cand = (uint32_t *)(map_smem + cull_off_cand(K, bn));
    L.best = (unsigned long long *)(map_smem + cull_off_best(K, bn));
    L.scr = (int *)(map_smem + cull_off_scr(K, bn));
    return L;
}

// nMPs and nRedundantObservations of slot t into out[0], out[1] (zeroed by the caller, behind a
// barrier); the workgroup calls it, a barrier follows
__device__ void cull_score(const MapDev &M, int t, int monocular, int *out)
{
    const int n = min(M.kf_n[t], M.cap);
    int nm = 0, nr = 0;
    for (int idx = threadIdx.x; idx < n; idx += MAP_T) {
        const int p = M.kf_points[(size_t)t * M.cap + idx];
        if (!map_point_ok(M, p)) continue;
        if (!monocular && !(M.kf_feat[(size_t)t * M.cap + idx] & ORBG_MAP_FEAT_CLOSE)) continue;
        nm++;
        const int lvl = M.kf_oct[(size_t)t * M.cap + idx];
        int nobs = 0, others = 0;
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) {
            int u, j;
            if (!cull_obs(M, M.obs[e], p, &u, &j)) continue;
            nobs += cull_weight(M, u, j);
            others += u != t && (int)M.kf_oct[(size_t)u * M.cap + j] <= lvl + 1;
        }
        nr += nobs > 3 && others >= 3;
    }
    if (nm) atomicAdd(&out[0], nm);
    if (nr) atomicAdd(&out[1], nr);
}

__device__ __forceinline__ bool cull_skipped(int fl)
{
    return (fl & ORBG_MAP_KF_ROOT) || !(fl & MAP_KF_LIVE) || (fl & ORBG_MAP_KF_BAD);
}

// KeyFrame::SetBadFlag of slot s by the whole workgroup (uniform arguments); returns the status
__device__ int map_set_bad(const MapDev &M, int s, int epoch, const CullLds &L)
{
    const int fl = M.kf_flags[s], er = M.kf_erase[s];
    const int n = min(M.kf_n[s], M.cap), par = M.parent[s];
    __syncthreads();  // every thread has read the slot's state
    if (!(fl & MAP_KF_LIVE) || (fl & ORBG_MAP_KF_ROOT)) return 0;
    if (er & MAP_NOT_ERASE) {
        if (threadIdx.x == 0) M.kf_erase[s] = er | MAP_TO_BE_ERASED;
        return 2;
    }
    // EraseConnection of every connected keyframe; its re-sort is deferred
    for (int t = threadIdx.x; t < M.K; t += MAP_T) {
        if (M.W[(size_t)t * M.K + s]) {
            M.W[(size_t)t * M.K + s] = 0;
            M.dirty[t] = epoch;
        }
        M.W[(size_t)s * M.K + t] = 0;
    }
    // EraseObservation of every point of the row
    for (int idx = threadIdx.x; idx < M.cap; idx += MAP_T) {
        const int p = M.kf_points[(size_t)s * M.cap + idx];
        M.kf_points[(size_t)s * M.cap + idx] = -1;
        if (idx >= n || !map_point_ok(M, p)) continue;  // a bad point has no observations
        int nobs = 0, low = -1;
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; e < e1; e++) {
            int u, j;
            if (!cull_obs(M, M.obs[e], p, &u, &j) || u == s) continue;
            nobs += cull_weight(M, u, j);
            if (low < 0) low = u;  // the segment is in ascending slot order
            M.row_touch[u] = epoch;
        }
        if (M.mp_ref[p] == s) M.mp_ref[p] = low;
        if (nobs <= 2) cull_point_bad(M, p);
    }
    if (threadIdx.x < ORBG_MAP_NEIGH) M.neigh[s * ORBG_MAP_NEIGH + threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        M.kf_flags[s] = ORBG_MAP_KF_BAD;
        M.kf_erase[s] = 0;
        M.kf_n[s] = 0;
        M.nord[s] = 0;
        M.mark[s] = epoch;  // its own (now empty) list is not re-sorted
    }
    __syncthreads();
    // the children, ascending: parent == s and live
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += M.parent[t] == s && (M.kf_flags[t] & MAP_KF_LIVE);
    int nch;
    int pos = block_scan(c, L.scr, &nch);
    for (int t = t0; t < t1; t++)
        if (M.parent[t] == s && (M.kf_flags[t] & MAP_KF_LIVE)) L.child[pos++] = t;
    for (int i = threadIdx.x; i < (M.K + 31) / 32; i += MAP_T) L.cand[i] = 0;
    __syncthreads();
    if (nch == 0) return 1;
    // UpdateBestCovisibles of the children rows an erasure of this call changed, before the
    // repair reads their lists
    for (int i = 0; i < nch; i++) {
        const int ch = L.child[i];
        if (M.dirty[ch] != epoch) continue;  // uniform
        for (int u = threadIdx.x; u < M.K; u += MAP_T) {
            const uint32_t w = M.W[(size_t)ch * M.K + u];
            L.keys[u] = w ? w << 13 | (uint32_t)u : 0;
        }
        __syncthreads();
        map_store_order(M, ch, L.keys, L.srt, L.scr);
        __syncthreads();
        if (threadIdx.x == 0) M.dirty[ch] = 0;
    }
    if (threadIdx.x == 0 && par >= 0 && par < M.K) L.cand[par >> 5] |= 1u << (par & 31);
    __syncthreads();
    for (;;) {
        if (threadIdx.x == 0) *L.best = 0ull;
        __syncthreads();
        unsigned long long my = 0ull;
        for (int i = 0; i < nch; i++) {
            const int ch = L.child[i];
            if (ch < 0 || (M.kf_flags[ch] & ORBG_MAP_KF_BAD)) continue;
            const int no = M.nord[ch];
            for (int q = threadIdx.x; q < no; q += MAP_T) {
                const int t = M.ord_slot[(size_t)ch * M.K + q];
                if (!(L.cand[t >> 5] >> (t & 31) & 1u)) continue;
                const unsigned long long w = M.W[(size_t)ch * M.K + t];  // GetWeight
                const unsigned long long key = (w + 1ull) << 26 |
                                               (unsigned long long)(MAP_SLOT_MASK - (uint32_t)i) << 13 |
                                               (unsigned long long)(MAP_SLOT_MASK - (uint32_t)q);
                my = my > key ? my : key;
            }
        }
        if (my) atomicMax(L.best, my);
        __syncthreads();
        const unsigned long long b = *L.best;
        if (!b) break;
        const int i = (int)(MAP_SLOT_MASK - (uint32_t)(b >> 13 & MAP_SLOT_MASK));
        const int q = (int)(MAP_SLOT_MASK - (uint32_t)(b & MAP_SLOT_MASK));
        const int ch = L.child[i];
        __syncthreads();  // every thread has read best and child[i]
        if (threadIdx.x == 0) {
            M.parent[ch] = M.ord_slot[(size_t)ch * M.K + q];
            L.cand[ch >> 5] |= 1u << (ch & 31);
            L.child[i] = -1;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < nch; i += MAP_T)
        if (L.child[i] >= 0) M.parent[L.child[i]] = par;
    __syncthreads();
    return 1;
}

// ---------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------
__global__ void k_map_point_defaults(MapDev M)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M.P) return;
    M.mp_first[p] = 0;
    M.mp_visible[p] = 1;
    M.mp_found[p] = 1;
}

__global__ __launch_bounds__(MAP_T) void k_map_set_features(MapDev M, const int32_t *slots,
                                                            const uint8_t *flags, int row_cap,
                                                            const int32_t *counts)
{
    const int i = blockIdx.x;
    const int s = slots[i];
    if (s < 0 || s >= M.K || !(M.kf_flags[s] & MAP_KF_LIVE)) return;
    const int n = min(max(counts[i], 0), min(row_cap, M.cap));
    for (int k = threadIdx.x; k < M.cap; k += MAP_T)
        M.kf_feat[(size_t)s * M.cap + k] = k < n ? flags[(size_t)i * row_cap + k] : 0;
}

__global__ void k_map_set_point_stats(MapDev M, const int32_t *ids, int first, int n,
                                      const int32_t *first_kf, const int32_t *visible,
                                      const int32_t *found)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = ids ? ids[i] : first + i;
    if (p < 0 || p >= M.P) return;
    if (first_kf) M.mp_first[p] = first_kf[i];
    if (visible) M.mp_visible[p] = visible[i];
    if (found) M.mp_found[p] = found[i];
}

__global__ void k_map_point_nobs(MapDev M, int first, int n, int32_t *nobs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) nobs[i] = cull_nobs(M, first + i);
}

__global__ void k_map_increase(int32_t *counter, int P, const int32_t *ids,
                               const orbg_map_projection *proj, int n, int amount)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = ids[i];
    if (p < 0 || p >= P) return;
    if (proj && !(proj[i].flags & ORBG_MP_VALID)) return;
    atomicAdd(&counter[p], amount);
}

// ---------------------------------------------------------------------------
// KeyFrame::SetNotErase / SetErase / SetBadFlag
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_set_bad(MapDev M, int s, int on, int epoch, int bn,
                                                       int32_t *status)
{
    const CullLds L = cull_lds_of(M.K, bn);
    int st = 0;
    if (on < 0) {
        st = map_set_bad(M, s, epoch, L);
    } else {
        const int fl = M.kf_flags[s], er = M.kf_erase[s];
        __syncthreads();
        if (fl & MAP_KF_LIVE) {
            if (on) {
                if (threadIdx.x == 0) M.kf_erase[s] = er | MAP_NOT_ERASE;
            } else {
                if (threadIdx.x == 0) M.kf_erase[s] = er & ~MAP_NOT_ERASE;
                __syncthreads();
                if (er & MAP_TO_BE_ERASED) st = map_set_bad(M, s, epoch, L) == 1;
            }
        }
    }
    if (threadIdx.x == 0) status[0] = st;
}

// ---------------------------------------------------------------------------
// LocalMapping::KeyFrameCulling
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_cull_score(MapDev M, int slot, int monocular)
{
    __shared__ int out[2];
    const int i = blockIdx.x;
    if (i >= M.nord[slot]) return;
    const int t = M.ord_slot[(size_t)slot * M.K + i];
    if (threadIdx.x == 0) {
        M.cull_list[i] = t;
        out[0] = out[1] = 0;
    }
    __syncthreads();
    if (!cull_skipped(M.kf_flags[t])) cull_score(M, t, monocular, out);
    __syncthreads();
    if (threadIdx.x < 2) M.cull_score[2 * i + threadIdx.x] = out[threadIdx.x];
}

__global__ __launch_bounds__(MAP_T) void k_cull_sequence(MapDev M, int slot, int monocular,
                                                         int epoch, int bn, orbg_cull_record *rec,
                                                         int rec_cap, int32_t *nrec)
{
    const CullLds L = cull_lds_of(M.K, bn);
    const int nl = M.nord[slot];
    __syncthreads();  // read before an early re-sort of this slot's own row can change it
    if (threadIdx.x == 0) nrec[0] = nl;
    for (int i = 0; i < nl; i++) {
        const int t = M.cull_list[i];
        int st = 3, nm = 0, nr = 0;
        if (!cull_skipped(M.kf_flags[t])) {  // uniform
            nm = M.cull_score[2 * i];
            nr = M.cull_score[2 * i + 1];
            if (M.row_touch[t] == epoch) {
                if (threadIdx.x == 0) L.scr[16] = L.scr[17] = 0;
                __syncthreads();
                cull_score(M, t, monocular, L.scr + 16);
                __syncthreads();
                nm = L.scr[16];
                nr = L.scr[17];
            }
            st = 0;
            if ((double)nr > 0.9 * (double)nm) st = map_set_bad(M, t, epoch, L);
        }
        if (threadIdx.x == 0 && i < rec_cap) {
            orbg_cull_record r;
            r.slot = t;
            r.status = st;
            r.nmps = nm;
            r.nredundant = nr;
            rec[i] = r;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// LocalMapping::MapPointCulling
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_point_cull(MapDev M, int32_t *recent, int n,
                                                      int current_kf_id, int th_obs,
                                                      int32_t *status)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= n) return;
    const int p = recent[i];
    int st = 0;
    if (p < 0 || p >= M.P || !(M.mp[p].flags & ORBG_MP_VALID)) {
        st = 1;
    } else if ((float)M.mp_found[p] / (float)M.mp_visible[p] < 0.25f) {  // GetFoundRatio()
        st = 2;
    } else {
        const int age = current_kf_id - M.mp_first[p];
        if (age >= 2 && cull_nobs(M, p) <= th_obs)
            st = 3;
        else if (age >= 3)
            st = 4;
    }
    if (st == 2 || st == 3) cull_point_bad(M, p);
    recent[i] = st == 0 ? p : -1;
    if (status) status[i] = st;
}

// the kept entries (>= 0) to the front, in order, in place
__global__ __launch_bounds__(MAP_T) void k_point_compact(int32_t *recent, int n, int32_t *nout)
{
    __shared__ int scr[4];
    int carry = 0;
    for (int base = 0; base < n; base += MAP_T) {  // uniform trip count
        const int i = base + threadIdx.x;
        const int v = i < n ? recent[i] : -1;
        int total;
        const int ex = block_scan(v >= 0, scr, &total);  // its barriers: the tile is read
        if (v >= 0) recent[carry + ex] = v;               // at or before i
        carry += total;
    }
    if (threadIdx.x == 0) nout[0] = carry;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_point_defaults(hipStream_t st, const MapDev &M)
{
    hipLaunchKernelGGL(k_map_point_defaults, dim3((M.P + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M);
    return last_rc();
}

int launch_map_set_features(hipStream_t st, const MapDev &M, const int32_t *slots, int n,
                            const uint8_t *flags, int row_cap, const int32_t *counts)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_set_features, dim3(n), dim3(MAP_T), 0, st, M, slots, flags, row_cap,
                       counts);
    return last_rc();
}

int launch_map_set_point_stats(hipStream_t st, const MapDev &M, const int32_t *ids, int first, int n,
                               const int32_t *first_kf, const int32_t *visible,
                               const int32_t *found)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_set_point_stats, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                       ids, first, n, first_kf, visible, found);
    return last_rc();
}

int launch_map_point_nobs(hipStream_t st, const MapDev &M, int first, int n, int32_t *nobs)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_point_nobs, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                       first, n, nobs);
    return last_rc();
}

int launch_map_increase(hipStream_t st, int32_t *counter, int P, const int32_t *ids,
                        const orbg_map_projection *proj, int n, int amount)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_increase, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, counter,
                       P, ids, proj, n, amount);
    return last_rc();
}

int launch_map_set_bad(hipStream_t st, const MapDev &M, int slot, int on, int epoch,
                       int32_t *status, Prof *prof)
{
    const int bn = map_pow2(M.K);
    const size_t lds = cull_lds(M.K, bn);
    if (map_attr((const void *)k_map_set_bad, lds)) return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_set_bad_flag", &ev);
    hipLaunchKernelGGL(k_map_set_bad, dim3(1), dim3(MAP_T), lds, st, M, slot, on, epoch, bn, status);
    const int rc = on == 1 ? ORBG_OK : launch_map_resort(st, M, epoch);
    prof_end(prof, st, "map_set_bad_flag", ev);
    return rc ? rc : last_rc();
}

int launch_map_keyframe_culling(hipStream_t st, const MapDev &M, int slot, int monocular,
                                int epoch, orbg_cull_record *rec, int rec_cap, int32_t *nrec,
                                Prof *prof)
{
    const int bn = map_pow2(M.K);
    const size_t lds = cull_lds(M.K, bn);
    if (map_attr((const void *)k_cull_sequence, lds)) return ORBG_EIO;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_cull_score", &ev);
    hipLaunchKernelGGL(k_cull_score, dim3(M.K), dim3(MAP_T), 0, st, M, slot, monocular);
    prof_end(prof, st, "map_cull_score", ev);
    prof_begin(prof, st, "map_cull_sequence", &ev);
    hipLaunchKernelGGL(k_cull_sequence, dim3(1), dim3(MAP_T), lds, st, M, slot, monocular, epoch, bn,
                       rec, rec_cap, nrec);
    const int rc = launch_map_resort(st, M, epoch);
    prof_end(prof, st, "map_cull_sequence", ev);
    return rc ? rc : last_rc();
}

int launch_map_point_culling(hipStream_t st, const MapDev &M, int32_t *recent, int n,
                             int current_kf_id, int monocular, int32_t *nout, int32_t *status,
                             Prof *prof)
{
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "map_point_culling", &ev);
    if (n > 0)
        hipLaunchKernelGGL(k_point_cull, dim3((n + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M,
                           recent, n, current_kf_id, monocular ? 2 : 3, status);
    hipLaunchKernelGGL(k_point_compact, dim3(1), dim3(MAP_T), 0, st, recent, n, nout);
    prof_end(prof, st, "map_point_culling", ev);
    return last_rc();
}

}  // namespace orbg
