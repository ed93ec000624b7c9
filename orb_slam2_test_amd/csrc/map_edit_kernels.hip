// map_edit_kernels.hip -- the edits of LocalMapping's loop that move observations between map
// points of the covisibility Map on gfx950: MapPoint::AddObservation (src/MapPoint.cc:121-142),
// MapPoint::Replace (:253-303), MapPoint::ComputeDistinctiveDescriptors over the map's own
// observations (:342-425), the map update of ORBmatcher::Fuse (src/ORBmatcher.cc:1100-1125)
// around the existing search kernel (k_fuse, mapping_kernels.hip) and the lists of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:583-683), and LoopClosing::CorrectLoop's
// loop fusion and SearchAndFuse (src/LoopClosing.cc:848-863, 944-992).
//
// Inside one call a surviving point gains observations, so the point -> observations index
// built before the call is no superset of a survivor's observers.  The rows are the truth; the
// observers of x are found among the index segments of x and of every point merged into x
// during this call (ed_next / ed_tail: a list per survivor, concatenated on every Replace,
// stamped with the call's number so nothing is reset), each entry verified against its row
// (cull_obs).  An index entry (u, j) lies in exactly one segment and a point in at most one
// list, so no observation is met twice.  The one observation no segment holds is the one
// AddObservation wrote in this call: in Fuse it is (pKF, bestIdx), passed to the walk as `ex`.
//
//   k_map_add_obs     one workgroup, entries in order; the lanes scan the slot's row for the
//                     point (IsInKeyFrame), thread 0 writes.
//   k_map_replace     one workgroup, pairs in order (edit_replace).
//   edit_replace      the slots that observe the new point into an LDS bitmap, then a lane
//                     per observation of the old point: moved, or erased where the bit is set.
//   k_fuse_job / k_fuse_gather / k_fuse_update
//                     one Fuse call: the job header (slot, count, camera; from the host or from
//                     SearchInNeighbors' device lists), the search inputs from the map, and
//                     after k_fuse the sequential update by one workgroup: the points with a
//                     target are compacted in order, then handled one by one.
//   k_dd_count / k_dd_fill / k_dd_scatter
//                     the rows of k_distinctive (frame_kernels.hip) from a current index, and
//                     its result into the map's mdesc.
//   k_sin_targets / k_sin_candidates / k_sin_row
//                     vpTargetKFs with its duplicates, vpFuseCandidates, the row re-read.
// Nothing waits on another workgroup; every loop is bounded by a count read once, a row
// length, an index segment or the number of merges a call can make.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

#define ED_BM (ORBG_MAP_MAX_KEYFRAMES / 32)

__device__ __forceinline__ bool edit_kf_live(const MapDev &M, int s)
{
    return s >= 0 && s < M.K && (M.kf_flags[s] & MAP_KF_LIVE);
}

__device__ __forceinline__ bool edit_kf_bad(const MapDev &M, int s)
{
    const int fl = M.kf_flags[s];
    return !(fl & MAP_KF_LIVE) || (fl & ORBG_MAP_KF_BAD);
}

// f(u, j) for every standing observation of x, by the whole workgroup (uniform arguments);
// (ex_u, ex_j): an entry of this call's AddObservation that no index segment holds, or -1
template <class F>
__device__ __forceinline__ void edit_walk(const MapDev &M, int x, int epoch, int guard, int ex_u,
                                          int ex_j, F f)
{
    int q = x;
    for (int g = 0; q >= 0 && q < M.P && g <= guard; g++) {
        const int e1 = M.obs_off[q + 1];
        for (int e = M.obs_off[q] + (int)threadIdx.x; e < e1; e += MAP_T) {
            int u, j;
            if (cull_obs(M, M.obs[e], x, &u, &j) && !(u == ex_u && j == ex_j)) f(u, j);
        }
        q = M.ed_chain[q] == epoch ? M.ed_next[q] : -1;
    }
    if (threadIdx.x == 0 && ex_u >= 0 && edit_kf_live(M, ex_u) &&
        M.kf_points[(size_t)ex_u * M.cap + ex_j] == x)
        f(ex_u, ex_j);
}

__device__ __forceinline__ void edit_chain_init(const MapDev &M, int x, int epoch)
{
    if (M.ed_chain[x] != epoch) {
        M.ed_next[x] = -1;
        M.ed_tail[x] = x;
        M.ed_chain[x] = epoch;
    }
}

// o->Replace(w) by the whole workgroup; o != w, both in range, w good.  Barriers inside; the
// caller's reads of o's and w's state precede the call.
// (exw_u, exw_j) / (exo_u, exo_j): the observation of w / of o that no index segment may hold
__device__ void edit_replace2(const MapDev &M, int o, int w, int exw_u, int exw_j, int exo_u,
                              int exo_j, int epoch, int guard, uint32_t *bm, bool was_bad)
{
    if (!was_bad) {
        for (int k = threadIdx.x; k < (M.K + 31) / 32; k += MAP_T) bm[k] = 0;
        __syncthreads();
        edit_walk(M, w, epoch, guard, exw_u, exw_j,
                  [&](int u, int) { atomicOr(&bm[u >> 5], 1u << (u & 31)); });
        __syncthreads();
        edit_walk(M, o, epoch, guard, exo_u, exo_j, [&](int u, int j) {
            // pMP->IsInKeyFrame(pKF): EraseMapPointMatch, else ReplaceMapPointMatch + AddObservation
            M.kf_points[(size_t)u * M.cap + j] = (bm[u >> 5] >> (u & 31) & 1u) ? -1 : w;
        });
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!was_bad) {
            M.mp[o].flags &= ~ORBG_MP_VALID;
            edit_chain_init(M, w, epoch);
            edit_chain_init(M, o, epoch);
            M.ed_next[M.ed_tail[w]] = o;
            M.ed_tail[w] = M.ed_tail[o];
        }
        M.mp_replaced[o] = w;
        M.mp_found[w] += M.mp_found[o];
        M.mp_visible[w] += M.mp_visible[o];
    }
    __syncthreads();
}

__device__ __forceinline__ void edit_replace(const MapDev &M, int o, int w, int ex_u, int ex_j,
                                             int epoch, int guard, uint32_t *bm, bool was_bad)
{
    edit_replace2(M, o, w, ex_u, ex_j, ex_u, ex_j, epoch, guard, bm, was_bad);
}

// the feature of slot s that holds x, or -1, by the whole workgroup (barriers inside); sh: LDS
__device__ __forceinline__ int edit_find(const MapDev &M, int s, int x, int nrow, int *sh)
{
    __syncthreads();
    if (threadIdx.x == 0) *sh = -1;
    __syncthreads();
    for (int k = threadIdx.x; k < nrow; k += MAP_T)
        if (M.kf_points[(size_t)s * M.cap + k] == x) *sh = k;  // at most one
    __syncthreads();
    return *sh;
}

// old->Replace(w) with MapPoint::Replace's early returns, both possibly seen by slot s through
// an observation written in this call; true when the survivor's descriptor is to be recomputed
__device__ bool edit_replace_in(const MapDev &M, int o, int w, int s, int nrow, int epoch, int guard,
                                uint32_t *bm, int *sh)
{
    if (o == w || o < 0 || o >= M.P || w < 0 || w >= M.P) return false;
    if (!(M.mp[w].flags & ORBG_MP_VALID)) return false;
    const bool was_bad = !(M.mp[o].flags & ORBG_MP_VALID);
    const int pw = edit_find(M, s, w, nrow, sh);
    const int po = edit_find(M, s, o, nrow, sh);
    edit_replace2(M, o, w, pw >= 0 ? s : -1, pw, po >= 0 ? s : -1, po, epoch, guard, bm, was_bad);
    return true;
}

// ---------------------------------------------------------------------------
// AddObservation + AddMapPoint
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_add_obs(MapDev M, const int32_t *slots,
                                                       const int32_t *idx, const int32_t *ids,
                                                       int n, int32_t *status)
{
    __shared__ int found;
    for (int i = 0; i < n; i++) {
        const int s = slots[i], j = idx[i], p = ids[i];
        if (threadIdx.x == 0) found = 0;
        __syncthreads();
        int st = 0;
        if (!edit_kf_live(M, s)) {
            st = 1;
        } else {
            const int nrow = min(M.kf_n[s], M.cap);
            if (j < 0 || j >= nrow) {
                st = 2;
            } else if (p < 0 || p >= M.P) {
                st = 3;
            } else if (!(M.mp[p].flags & ORBG_MP_VALID)) {
                st = 4;
            } else {
                for (int k = threadIdx.x; k < nrow; k += MAP_T)
                    if (M.kf_points[(size_t)s * M.cap + k] == p) found = 1;
                __syncthreads();
                if (found)
                    st = 5;
                else if (M.kf_points[(size_t)s * M.cap + j] >= 0)
                    st = 6;
            }
        }
        __syncthreads();  // every thread has read the row and `found`
        if (threadIdx.x == 0) {
            if (st == 0) M.kf_points[(size_t)s * M.cap + j] = p;
            if (status) status[i] = st;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// ComputeDistinctiveDescriptors over the map's observations: the rows of k_distinctive
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool dd_usable(const MapDev &M, const MapAttach &A, uint32_t ob, int *row)
{
    const int u = (int)(ob >> 16), j = (int)(ob & 0xFFFFu);
    if (edit_kf_bad(M, u) || j >= A.cap || j >= A.kfs.counts[u]) return false;
    *row = u * A.cap + j;
    return true;
}

// off[i] = the start of point ids[i]'s rows, off[n_eff] = tot[0] = their number.  A bad point,
// an id out of range or one already listed (ed_mark) takes no rows.  One workgroup.
__global__ __launch_bounds__(MAP_T) void k_dd_count(MapDev M, MapAttach A, const int32_t *ids,
                                                    int n, const int32_t *dn, int epoch,
                                                    int32_t *off, int32_t *tot)
{
    __shared__ int scr[4];
    if (dn) n = min(max(dn[0], 0), n);
    int carry = 0;
    for (int base = 0; base < n; base += MAP_T) {  // uniform trip count
        const int i = base + threadIdx.x;
        int c = 0;
        if (i < n) {
            const int p = ids[i];
            if (map_point_ok(M, p) && atomicExch(&M.ed_mark[p], epoch) != epoch) {
                const int e1 = M.obs_off[p + 1];
                for (int e = M.obs_off[p]; e < e1; e++) {
                    int row;
                    c += dd_usable(M, A, M.obs[e], &row);
                }
            }
        }
        int total;
        const int ex = block_scan(c, scr, &total);
        if (i < n) off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        off[n] = carry;
        tot[0] = carry;
        tot[1] = n;
    }
}

__global__ __launch_bounds__(MAP_T) void k_dd_fill(MapDev M, MapAttach A, const int32_t *ids, int n,
                                                   int32_t *off, const int32_t *tot, int32_t *rows)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= n) return;
    if (i >= tot[1]) {  // past the device-side count: no rows
        off[i + 1] = tot[0];
        return;
    }
    int o = off[i];
    if (off[i + 1] == o) return;
    const int p = ids[i];
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        int row;
        if (dd_usable(M, A, M.obs[e], &row)) rows[o++] = row;
    }
}

__global__ __launch_bounds__(MAP_T) void k_dd_scatter(MapDev M, const int32_t *ids, int n,
                                                      const int32_t *off, const uint8_t *desc)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= n || off[i + 1] == off[i]) return;
    const int p = ids[i];
    const uint4 *src = (const uint4 *)(desc + (size_t)i * 32);
    uint4 *dst = (uint4 *)(M.mdesc + (size_t)p * 32);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---------------------------------------------------------------------------
// MapPoint::Replace
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_T) void k_map_replace(MapDev M, const int32_t *olds,
                                                       const int32_t *news, int n, int epoch,
                                                       int32_t *status, int32_t *surv)
{
    __shared__ uint32_t bm[ED_BM];
    for (int i = 0; i < n; i++) {
        const int o = olds[i], w = news[i];
        int st, sv = -1;
        if (o == w) {
            st = 1;
        } else if (w < 0 || w >= M.P || !(M.mp[w].flags & ORBG_MP_VALID)) {
            st = 2;
        } else if (o < 0 || o >= M.P) {
            st = 3;
        } else {
            const bool was_bad = !(M.mp[o].flags & ORBG_MP_VALID);
            edit_replace(M, o, w, -1, -1, epoch, n, bm, was_bad);
            st = was_bad ? 4 : 0;
            sv = w;
        }
        if (threadIdx.x == 0) {
            if (status) status[i] = st;
            surv[i] = sv;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// ORBmatcher::Fuse(pKF, vpMapPoints, th) around k_fuse
// ---------------------------------------------------------------------------
__global__ void k_fuse_job(MapDev M, MapAttach A, MapEditWs W, int slot, int n, int entry, int cur)
{
    if (blockIdx.x || threadIdx.x) return;
    int s, cnt, act;
    if (slot >= 0) {
        s = slot;
        cnt = n;
        act = 1;
    } else if (entry < ORBG_MAP_MAX_TARGETS) {
        act = entry < W.targets[ORBG_MAP_MAX_TARGETS];
        s = act ? W.targets[entry] : 0;
        cnt = W.snap[M.cap];
    } else {
        s = cur;
        cnt = W.ids[W.ncap];
        act = 1;
    }
    act = act && edit_kf_live(M, s);
    if (!act) {
        s = min(max(s, 0), M.K - 1);
        cnt = 0;
    }
    W.hdr[MAP_HDR_SLOT] = s;
    W.hdr[MAP_HDR_N] = min(max(cnt, 0), W.ncap);
    W.hdr[MAP_HDR_ACTIVE] = act;
    W.cam[0] = A.cams[s];
}

// the search inputs: the record and mDescriptor of ids[i], VALID = in range, good and not in
// the slot's row (the index is current)
__global__ __launch_bounds__(MAP_T) void k_fuse_gather(MapDev M, MapEditWs W, const int32_t *ids)
{
    const int i = blockIdx.x * MAP_T + threadIdx.x;
    if (i >= W.hdr[MAP_HDR_N]) return;
    const int s = W.hdr[MAP_HDR_SLOT], p = ids[i];
    orbg_map_point r{};
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (p >= 0 && p < M.P) {
        r = M.mp[p];
        bool ok = (r.flags & ORBG_MP_VALID) != 0;
        const int e1 = M.obs_off[p + 1];
        for (int e = M.obs_off[p]; ok && e < e1; e++) {
            int u, j;
            if (cull_obs(M, M.obs[e], p, &u, &j) && u == s) ok = false;  // IsInKeyFrame(pKF)
        }
        r.flags = ok ? ORBG_MP_VALID : 0;
        const uint4 *src = (const uint4 *)(M.mdesc + (size_t)p * 32);
        d0 = src[0];
        d1 = src[1];
    }
    W.mps[i] = r;
    uint4 *dst = (uint4 *)(W.mdesc + (size_t)i * 32);
    dst[0] = d0;
    dst[1] = d1;
}

// Observations() of x by the whole workgroup into *acc (LDS, zeroed behind a barrier by the
// caller); a barrier follows in the caller
__device__ __forceinline__ void edit_nobs(const MapDev &M, int x, int epoch, int guard, int ex_u,
                                          int ex_j, int *acc)
{
    int c = 0;
    edit_walk(M, x, epoch, guard, ex_u, ex_j, [&](int u, int j) { c += cull_weight(M, u, j); });
    if (c) atomicAdd(acc, c);
}

// The update of :1100-1125 by one workgroup.  The points with a target (bestDist <= TH_LOW, a
// feature index inside the row) are compacted in order first, so the sequential part runs over
// them alone.  nfused[at_nt ? ntargets : 0] = the count of statuses 1..4.
__global__ __launch_bounds__(MAP_T) void k_fuse_update(MapDev M, MapEditWs W, const int32_t *ids,
                                                       int nmax, int epoch, int32_t *best_idx,
                                                       int32_t *best_dist, int32_t *status,
                                                       int32_t *nfused, int at_nt)
{
    __shared__ uint32_t bm[ED_BM];
    __shared__ int scr[4];
    __shared__ int acc[2];
    const int s = W.hdr[MAP_HDR_SLOT], n = min(W.hdr[MAP_HDR_N], nmax);
    const int nrow = W.hdr[MAP_HDR_ACTIVE] ? min(M.kf_n[s], M.cap) : 0;
    int32_t *hits = W.hits;
    int nh = 0;
    const int lim = (best_idx || best_dist || status) ? nmax : n;  // the outputs cover nmax
    for (int base = 0; base < lim; base += MAP_T) {  // uniform trip count
        const int i = base + threadIdx.x;
        bool hit = false;
        if (i < lim) {
            int b = -1, d = 256;
            if (i < n) {
                b = W.bidx[i];
                d = W.bdist[i];
                const int p = ids[i];
                hit = p >= 0 && p < M.P && b >= 0 && b < nrow && d <= ORBG_MAP_TH_LOW;
            }
            if (best_idx) best_idx[i] = b;
            if (best_dist) best_dist[i] = d;
            if (status) status[i] = 0;
            if (i < n) W.surv[i] = -1;
        }
        int total;
        const int ex = block_scan(hit, scr, &total);
        if (hit) hits[nh + ex] = i;
        nh += total;
    }
    __syncthreads();
    int fused = 0;
    for (int h = 0; h < nh; h++) {
        const int i = hits[h];
        const int p = ids[i], b = W.bidx[i];
        int st, sv = -1;
        if (threadIdx.x < 2) acc[threadIdx.x] = 0;
        __syncthreads();
        if (!(M.mp[p].flags & ORBG_MP_VALID) || M.ed_inkf[p] == epoch) {
            st = 5;  // isBad() || IsInKeyFrame(pKF) by its turn
        } else {
            const int q = M.kf_points[(size_t)s * M.cap + b];
            if (q < 0) {
                st = 1;
            } else if (q >= M.P || !(M.mp[q].flags & ORBG_MP_VALID)) {
                st = 4;
            } else {
                edit_nobs(M, q, epoch, nh, s, b, &acc[0]);
                edit_nobs(M, p, epoch, nh, s, b, &acc[1]);
                __syncthreads();
                const bool keep_q = acc[0] > acc[1];  // pMPinKF->Observations() > pMP->Observations()
                __syncthreads();
                if (keep_q) {
                    edit_replace(M, p, q, s, b, epoch, nh, bm, false);
                    st = 2;
                    sv = q;
                } else {
                    edit_replace(M, q, p, s, b, epoch, nh, bm, false);
                    st = 3;
                    sv = p;
                }
            }
        }
        __syncthreads();  // every thread has read the state this entry's writes change
        if (threadIdx.x == 0) {
            if (st == 1) M.kf_points[(size_t)s * M.cap + b] = p;
            if (st == 1 || st == 3) M.ed_inkf[p] = epoch;
            if (status) status[i] = st;
            W.surv[i] = sv;
        }
        fused += st != 5;
        __syncthreads();
    }
    if (threadIdx.x == 0 && nfused) nfused[at_nt ? min(W.targets[ORBG_MAP_MAX_TARGETS], ORBG_MAP_MAX_TARGETS) : 0] = fused;
}

// ---------------------------------------------------------------------------
// LoopClosing::CorrectLoop's loop fusion (src/LoopClosing.cc:848-863) and SearchAndFuse's
// update (:944-992 with ORBmatcher.cc:1230-1250)
// ---------------------------------------------------------------------------
// matched[i] (mvpCurrentMatchedPoints as ids, -1 = none) in feature order: a held point is
// replaced by the matched one, else the matched one is added.  surv [cap]: the points whose
// descriptor is recomputed once after the call; counts: replaced, added
__global__ __launch_bounds__(MAP_T) void k_loop_fusion(MapDev M, int cur, const int32_t *matched,
                                                       int nm, int epoch, int32_t *surv,
                                                       int32_t *counts)
{
    __shared__ uint32_t bm[ED_BM];
    __shared__ int sh;
    const int nrow = edit_kf_live(M, cur) ? min(M.kf_n[cur], M.cap) : 0;
    const int n = min(nrow, nm);
    for (int k = threadIdx.x; k < M.cap; k += MAP_T) surv[k] = -1;
    __syncthreads();
    int nrep = 0, nadd = 0;
    for (int i = 0; i < n; i++) {
        const int w = matched[i];
        if (w < 0 || w >= M.P) continue;
        const int o = M.kf_points[(size_t)cur * M.cap + i];
        int sv = -1;
        if (o >= 0) {
            if (edit_replace_in(M, o, w, cur, nrow, epoch, n, bm, &sh)) {
                sv = w;
                nrep++;
            }
        } else if (M.mp[w].flags & ORBG_MP_VALID) {
            if (edit_find(M, cur, w, nrow, &sh) < 0) {  // AddObservation returns when cur has it
                if (threadIdx.x == 0) M.kf_points[(size_t)cur * M.cap + i] = w;
                sv = w;
                nadd++;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) surv[i] = sv;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = nrep;
        counts[1] = nadd;
    }
}

// the job of SearchAndFuse's member of rank `rank` in slot order: its slot, the loop points'
// count, the attached camera with the corrected Sim3's rows as Tcw ([s R | t], float)
__global__ void k_sf_job(MapDev M, MapAttach A, MapEditWs W, const int32_t *set, int set_cap,
                         const int32_t *nset, int rank, const orbg_sim3d *corrected, int n)
{
    if (blockIdx.x || threadIdx.x) return;
    const int ns = min(max(*nset, 0), set_cap);
    int s = -1;
    for (int i = 0; i < ns && s < 0; i++) {
        int r = 0;
        for (int k = 0; k < ns; k++) r += set[k] < set[i];
        if (r == rank) s = set[i];
    }
    const int act = rank < ns && edit_kf_live(M, s);
    const int sc = min(max(s, 0), M.K - 1);
    W.hdr[MAP_HDR_SLOT] = sc;
    W.hdr[MAP_HDR_N] = act ? min(max(n, 0), W.ncap) : 0;
    W.hdr[MAP_HDR_ACTIVE] = act;
    orbg_frustum_camera cam = A.cams[sc];
    if (act) {
        const orbg_sim3d S = corrected[sc];
        const double x = S.q[0], y = S.q[1], z = S.q[2], w = S.q[3];  // Quaterniond::toRotationMatrix
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
        const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
        const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz),
                             tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) cam.Tcw[r * 4 + k] = (float)(S.s * R[r * 3 + k]);
            cam.Tcw[r * 4 + 3] = (float)S.t[r];
        }
    }
    W.cam[0] = cam;
}

// Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)'s update and SearchAndFuse's Replace loop by one
// workgroup: first every point with a target in order (a free feature takes it, a good point on
// the feature is recorded), then the recorded points are replaced in order.  counts: nFused,
// replaced
__global__ __launch_bounds__(MAP_T) void k_sf_update(MapDev M, MapEditWs W, const int32_t *ids,
                                                     int nmax, int epoch, int32_t *counts)
{
    __shared__ uint32_t bm[ED_BM];
    __shared__ int scr[4];
    __shared__ int sh;
    const int s = W.hdr[MAP_HDR_SLOT], n = min(W.hdr[MAP_HDR_N], nmax);
    const int nrow = W.hdr[MAP_HDR_ACTIVE] ? min(M.kf_n[s], M.cap) : 0;
    int32_t *hits = W.hits, *rep = W.dd_best;
    int nh = 0;
    for (int base = 0; base < nmax; base += MAP_T) {  // uniform trip count
        const int i = base + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const int b = W.bidx[i], p = ids[i];
            hit = p >= 0 && p < M.P && b >= 0 && b < nrow && W.bdist[i] <= ORBG_MAP_TH_LOW;
        }
        if (i < nmax) W.surv[i] = -1;
        int total;
        const int ex = block_scan(hit, scr, &total);
        if (hit) hits[nh + ex] = i;
        nh += total;
    }
    __syncthreads();
    int fused = 0, nrep = 0;
    for (int h = 0; h < nh; h++) {
        const int p = ids[hits[h]], b = W.bidx[hits[h]];
        const int q = M.kf_points[(size_t)s * M.cap + b];
        int r = -1;
        bool add = false;
        if (q < 0)
            add = (M.mp[p].flags & ORBG_MP_VALID) && edit_find(M, s, p, nrow, &sh) < 0;
        else if (q < M.P && (M.mp[q].flags & ORBG_MP_VALID))
            r = q;
        __syncthreads();
        if (threadIdx.x == 0) {
            if (add) M.kf_points[(size_t)s * M.cap + b] = p;
            rep[h] = r;
        }
        fused++;
        __syncthreads();
    }
    for (int h = 0; h < nh; h++) {
        const int r = rep[h];
        if (r < 0) continue;
        const int p = ids[hits[h]];
        const bool done = edit_replace_in(M, r, p, s, nrow, epoch, nh, bm, &sh);
        __syncthreads();
        if (done) {
            if (threadIdx.x == 0) W.surv[hits[h]] = p;
            nrep++;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] += fused;
        counts[1] += nrep;
    }
}

// ---------------------------------------------------------------------------
// LocalMapping::SearchInNeighbors: the lists
// ---------------------------------------------------------------------------
// vpTargetKFs of `slot` into W.targets (all of it) and targets (the first target_cap), the
// slot's row into W.snap; nfused[0 .. MAX_TARGETS] = 0
__global__ __launch_bounds__(MAP_T) void k_sin_targets(MapDev M, MapEditWs W, int slot,
                                                       int current_kf_id, int nn, int32_t *targets,
                                                       int target_cap, int32_t *ntargets,
                                                       int32_t *nfused)
{
    const bool live = edit_kf_live(M, slot);
    const int nrow = live ? min(M.kf_n[slot], M.cap) : 0;
    for (int k = threadIdx.x; k < M.cap; k += MAP_T)
        W.snap[k] = k < nrow ? M.kf_points[(size_t)slot * M.cap + k] : -1;
    for (int k = threadIdx.x; k <= ORBG_MAP_MAX_TARGETS; k += MAP_T) nfused[k] = 0;
    if (threadIdx.x) return;
    W.snap[M.cap] = nrow;
    int nt = 0;
    // mnFuseTargetForKF starts at 0: with current_kf_id == 0 every keyframe counts as marked
    if (live && current_kf_id != 0) {
        int marked[20], nm = 0;
        const int n1 = min(M.nord[slot], nn);
        for (int a = 0; a < n1; a++) {
            const int t = M.ord_slot[(size_t)slot * M.K + a];
            bool skip = edit_kf_bad(M, t);
            for (int k = 0; k < nm; k++) skip |= marked[k] == t;
            if (skip) continue;
            W.targets[nt++] = t;
            marked[nm++] = t;
            const int n2 = min(M.nord[t], 5);
            for (int c = 0; c < n2; c++) {
                const int t2 = M.ord_slot[(size_t)t * M.K + c];
                bool skip2 = edit_kf_bad(M, t2) || t2 == slot;
                for (int k = 0; k < nm; k++) skip2 |= marked[k] == t2;
                if (!skip2) W.targets[nt++] = t2;  // not marked: it may be listed again
            }
        }
    }
    W.targets[ORBG_MAP_MAX_TARGETS] = nt;
    for (int k = 0; k < min(nt, target_cap); k++) targets[k] = W.targets[k];
    ntargets[0] = nt;
}

// vpFuseCandidates: the good points of the target entries' rows in list order and feature
// order, each at its first occurrence (ed_first: the least position).  One workgroup.
__global__ __launch_bounds__(MAP_T) void k_sin_candidates(MapDev M, MapEditWs W)
{
    __shared__ int scr[4];
    const int nt = min(W.targets[ORBG_MAP_MAX_TARGETS], ORBG_MAP_MAX_TARGETS);
    for (int pass = 0; pass < 2; pass++) {
        for (int a = 0; a < nt; a++) {
            const int t = W.targets[a];
            const int nrow = edit_kf_live(M, t) ? min(M.kf_n[t], M.cap) : 0;
            for (int k = threadIdx.x; k < nrow; k += MAP_T) {
                const int p = M.kf_points[(size_t)t * M.cap + k];
                if (!map_point_ok(M, p)) continue;
                if (pass == 0)
                    M.ed_first[p] = 0x7fffffff;
                else
                    atomicMin(&M.ed_first[p], a * M.cap + k);
            }
        }
        __syncthreads();
    }
    int carry = 0;
    for (int a = 0; a < nt; a++) {
        const int t = W.targets[a];
        const int nrow = edit_kf_live(M, t) ? min(M.kf_n[t], M.cap) : 0;
        for (int base = 0; base < nrow; base += MAP_T) {  // uniform trip count
            const int k = base + threadIdx.x;
            int p = -1;
            if (k < nrow) {
                p = M.kf_points[(size_t)t * M.cap + k];
                if (!map_point_ok(M, p) || M.ed_first[p] != a * M.cap + k) p = -1;
            }
            int total;
            const int ex = block_scan(p >= 0, scr, &total);
            if (p >= 0 && carry + ex < W.ncap) W.ids[carry + ex] = p;
            carry += total;
        }
    }
    if (threadIdx.x == 0) W.ids[W.ncap] = min(carry, W.ncap);
}

// the slot's row as it stands, -1 padded to kf_cap, and the slot itself for UpdateConnections
__global__ __launch_bounds__(MAP_T) void k_sin_row(MapDev M, MapEditWs W, int slot)
{
    const int nrow = edit_kf_live(M, slot) ? min(M.kf_n[slot], M.cap) : 0;
    for (int k = threadIdx.x; k < M.cap; k += MAP_T)
        W.snap[k] = k < nrow ? M.kf_points[(size_t)slot * M.cap + k] : -1;
    if (threadIdx.x == 0) W.hdr[MAP_HDR_CUR] = slot;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_map_add_observations(hipStream_t st, const MapDev &M, const int32_t *slots,
                                const int32_t *idx, const int32_t *ids, int n, int32_t *status)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_add_obs, dim3(1), dim3(MAP_T), 0, st, M, slots, idx, ids, n, status);
    return last_rc();
}

int launch_map_distinctive(hipStream_t st, const MapDev &M, const MapAttach &A, const int32_t *ids,
                           int n, const int32_t *dn, int epoch, int32_t *off, int32_t *tot,
                           int32_t *best, uint8_t *desc)
{
    if (n <= 0) return ORBG_OK;
    const int g = (n + MAP_T - 1) / MAP_T;
    int32_t *rows = (int32_t *)M.obs_tmp;  // free once the index is built
    hipLaunchKernelGGL(k_dd_count, dim3(1), dim3(MAP_T), 0, st, M, A, ids, n, dn, epoch, off, tot);
    hipLaunchKernelGGL(k_dd_fill, dim3(g), dim3(MAP_T), 0, st, M, A, ids, n, off, tot, rows);
    if (launch_distinctive(st, A.kfs.desc, rows, off, n, best, desc)) return ORBG_EIO;
    hipLaunchKernelGGL(k_dd_scatter, dim3(g), dim3(MAP_T), 0, st, M, ids, n, off, desc);
    return last_rc();
}

int launch_map_replace(hipStream_t st, const MapDev &M, const int32_t *olds, const int32_t *news,
                       int n, int epoch, int32_t *status, int32_t *surv)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_map_replace, dim3(1), dim3(MAP_T), 0, st, M, olds, news, n, epoch, status,
                       surv);
    return last_rc();
}

int launch_map_fuse_job(hipStream_t st, const MapDev &M, const MapAttach &A, const MapEditWs &W,
                        int slot, int n, int entry, int cur)
{
    hipLaunchKernelGGL(k_fuse_job, dim3(1), dim3(64), 0, st, M, A, W, slot, n, entry, cur);
    return last_rc();
}

int launch_map_fuse_gather(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                           int nmax)
{
    if (nmax <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_fuse_gather, dim3((nmax + MAP_T - 1) / MAP_T), dim3(MAP_T), 0, st, M, W,
                       ids);
    return last_rc();
}

int launch_map_fuse_update(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                           int nmax, int epoch, int32_t *best_idx, int32_t *best_dist,
                           int32_t *status, int32_t *nfused, int nfused_at_ntargets)
{
    hipLaunchKernelGGL(k_fuse_update, dim3(1), dim3(MAP_T), 0, st, M, W, ids, nmax, epoch, best_idx,
                       best_dist, status, nfused, nfused_at_ntargets);
    return last_rc();
}

int launch_map_loop_fusion(hipStream_t st, const MapDev &M, int cur, const int32_t *matched, int nm,
                           int epoch, int32_t *surv, int32_t *counts)
{
    hipLaunchKernelGGL(k_loop_fusion, dim3(1), dim3(MAP_T), 0, st, M, cur, matched, nm, epoch, surv,
                       counts);
    return last_rc();
}

int launch_map_sf_job(hipStream_t st, const MapDev &M, const MapAttach &A, const MapEditWs &W,
                      const int32_t *set, int set_cap, const int32_t *nset, int rank,
                      const orbg_sim3d *corrected, int n)
{
    hipLaunchKernelGGL(k_sf_job, dim3(1), dim3(64), 0, st, M, A, W, set, set_cap, nset, rank,
                       corrected, n);
    return last_rc();
}

int launch_map_sf_update(hipStream_t st, const MapDev &M, const MapEditWs &W, const int32_t *ids,
                         int nmax, int epoch, int32_t *counts)
{
    hipLaunchKernelGGL(k_sf_update, dim3(1), dim3(MAP_T), 0, st, M, W, ids, nmax, epoch, counts);
    return last_rc();
}

int launch_map_sin_targets(hipStream_t st, const MapDev &M, const MapEditWs &W, int slot,
                           int current_kf_id, int monocular, int32_t *targets, int target_cap,
                           int32_t *ntargets, int32_t *nfused)
{
    hipLaunchKernelGGL(k_sin_targets, dim3(1), dim3(MAP_T), 0, st, M, W, slot, current_kf_id,
                       monocular ? 20 : 10, targets, target_cap, ntargets, nfused);
    return last_rc();
}

int launch_map_sin_candidates(hipStream_t st, const MapDev &M, const MapEditWs &W)
{
    hipLaunchKernelGGL(k_sin_candidates, dim3(1), dim3(MAP_T), 0, st, M, W);
    return last_rc();
}

int launch_map_sin_row(hipStream_t st, const MapDev &M, const MapEditWs &W, int slot)
{
    hipLaunchKernelGGL(k_sin_row, dim3(1), dim3(MAP_T), 0, st, M, W, slot);
    return last_rc();
}

}  // namespace orbg
