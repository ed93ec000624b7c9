// place_kernels.hip -- place recognition on gfx950: DBoW2's L1 score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and ORB-SLAM2's KeyFrameDatabase
// (src/KeyFrameDatabase.cc: add :50, erase :58, DetectLoopCandidates :106-274,
// DetectRelocalizationCandidates :291-419).
//
//   k_place_score    one wave per (v1, v2) pair: 64 entries of v2 at a time binary-search v1's
//                    ascending word ids; the matched lanes' terms fabs(vi - wi) - fabs(vi) -
//                    fabs(wi) are then added one at a time in lane (= word) order, so the sum
//                    is the reference's sequential double sum; -score / 2.0 at the end.
//   k_place_add      copies BowVectors into their slots' rows, marks the slots live, gives
//                    them the next add-sequence numbers and pins mRelocScore to 0.
//   k_place_hist / k_place_scan_* / k_place_fill / k_place_rank
//                    the inverted file (CSR over the words, postings = slots) from the live
//                    rows: word histogram (integer atomics), exclusive scan (tile sums, a
//                    one-workgroup scan of the sums, tiles), fill (the order
//                    inside a word is arbitrary: nothing reads it), and each live slot's rank
//                    among the live slots by add-sequence number.
//   k_place_query    one workgroup per query.  Pass 1: shared-word counts per slot, packed
//                    16-bit counters in LDS (integer atomics; bit 15 marks a connected
//                    KeyFrame in loop mode).  Workgroup max -> minCommonWords; the survivors
//                    (count > minCommonWords) are compacted and each is scored by one wave
//                    against the KeyFrame's own vector with k_place_score's intersection, the
//                    query's words staged in LDS; the first matched word is the survivor's
//                    position in lKFsSharingWords' order.  The survivors are bitonic-sorted
//                    by (first shared word position, add rank) = the reference's list order;
//                    the neighbour accumulation runs one entry per thread (float adds in
//                    neighbour order), bestAccScore is a float max, and the retained entries
//                    are deduplicated (first occurrence by atomicMin of the entry index) and
//                    compacted in order.  No floating-point sum depends on thread order.
//   k_place_apply    after a relocalization call: each scored slot's mRelocScore becomes the
//                    score from the call's highest-indexed query that scored it (64-bit
//                    atomicMax of (query + 1) << 32 | float bits during the queries, which
//                    all read the scores as they were when the call started).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/orbg.h"
#include "place_args.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

#define PLACE_THREADS 256
#define PLACE_SCAN_THREADS 1024

// L1Scoring::score(v1 = a, v2 = b) by one wave (all 64 lanes active, every lane returns the
// same double).  aw may point to LDS or global memory.  *first = the index in `a` of the
// first common word (-1: none).
__device__ __forceinline__ double wave_l1_score(const int32_t *aw, const double *ax, int na,
                                                const int32_t *bw, const double *bx, int nb,
                                                int *first)
{
    const int lane = threadIdx.x & 63;
    double score = 0;
    int f = -1;
    for (int base = 0; base < nb; base += 64) {
        const int j = base + lane;
        bool hit = false;
        int pos = 0;
        double term = 0;
        if (j < nb) {
            const int32_t w = bw[j];
            int lo = 0, hi = na;  // lower_bound
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (aw[mid] < w)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < na && aw[lo] == w) {
                hit = true;
                pos = lo;
                const double vi = ax[lo], wi = bx[j];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long mask = __ballot(hit);
        if (mask && f < 0) f = __shfl(pos, __ffsll((long long)mask) - 1, 64);
        while (mask) {  // ascending word order
            const int l = __ffsll((long long)mask) - 1;
            score += __shfl(term, l, 64);
            mask &= mask - 1;
        }
    }
    *first = f;
    return -score / 2.0;
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_score(orbg_bow_vectors a,
                                                               orbg_bow_vectors b, int cap,
                                                               const int32_t *a_index,
                                                               const int32_t *b_index, int npairs,
                                                               double *score)
{
    const int p = blockIdx.x * (PLACE_THREADS / 64) + (threadIdx.x >> 6);
    if (p >= npairs) return;  // uniform per wave
    const int ia = a_index ? a_index[p] : p, ib = b_index ? b_index[p] : p;
    const int na = min(max(a.nbow[ia], 0), cap), nb = min(max(b.nbow[ib], 0), cap);
    int first;
    const double s = wave_l1_score(a.words + (size_t)ia * cap, a.weights + (size_t)ia * cap, na,
                                   b.words + (size_t)ib * cap, b.weights + (size_t)ib * cap, nb,
                                   &first);
    if ((threadIdx.x & 63) == 0) score[p] = s;
}

// ---------------------------------------------------------------------------
// database maintenance
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PLACE_THREADS) void k_place_add(PlaceDb D, const int32_t *slots,
                                                             orbg_bow_vectors v, int vcap,
                                                             const int32_t *index, int n)
{
    const int i = blockIdx.x;
    const int slot = slots[i];
    if (slot < 0 || slot >= D.K) return;
    const int src = index ? index[i] : i;
    const int nb = min(max(v.nbow[src], 0), min(vcap, D.cap));
    const int32_t *sw = v.words + (size_t)src * vcap;
    const double *sx = v.weights + (size_t)src * vcap;
    int32_t *dw = D.words + (size_t)slot * D.cap;
    double *dx = D.weights + (size_t)slot * D.cap;
    for (int k = threadIdx.x; k < nb; k += PLACE_THREADS) {
        dw[k] = sw[k];
        dx[k] = sx[k];
    }
    if (threadIdx.x == 0) {
        D.nbow[slot] = nb;
        D.live[slot] = 1;
        D.seq[slot] = D.counter[0] + i;
        D.reloc[slot] = 0.0f;  // KeyFrame.cc:39-40 leaves mRelocScore uninitialised
    }
}

__global__ void k_place_bump(PlaceDb D, int n) { D.counter[0] += n; }

__global__ void k_place_erase(PlaceDb D, int slot) { D.live[slot] = 0; }

__global__ __launch_bounds__(PLACE_THREADS) void k_place_hist(PlaceDb D)
{
    const int s = blockIdx.x;
    if (!D.live[s]) return;
    const int nb = D.nbow[s];
    const int32_t *w = D.words + (size_t)s * D.cap;
    for (int k = threadIdx.x; k < nb; k += PLACE_THREADS) {
        const int wd = w[k];
        if (wd >= 0 && wd < D.nwords) atomicAdd(&D.inv_cur[wd], 1);
    }
}

// Exclusive scan of the word histogram in three launches.  A tile = PLACE_SCAN_TILE
// consecutive words, four per thread.
//   k_place_scan_sum   part[b] = tile b's total
//   k_place_scan_top   one workgroup: part[] -> its exclusive scan, inv_off[nwords] = total
//   k_place_scan_fin   inv_off = inv_cur (the fill cursors) = part[b] + the scan inside tile b
#define PLACE_SCAN_TILE (PLACE_SCAN_THREADS * 4)

// exclusive scan of in[i0 .. i0 + 4) per thread across the workgroup, offset by `base`, written
// to out0 (and out1 when non-NULL) for indices < n; returns the tile's total (every thread)
__device__ __forceinline__ int place_scan_tile(const int32_t *in, int n, int i0, int base,
                                               int32_t *out0, int32_t *out1, int *wsum)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int v[4], t = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        v[u] = i0 + u < n ? in[i0 + u] : 0;
        t += v[u];
    }
    int inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(inc, o, 64);
        if (lane >= o) inc += x;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int k = 0; k < PLACE_SCAN_THREADS / 64; k++) {
        if (k < wv) base += wsum[k];
        tot += wsum[k];
    }
    __syncthreads();  // wsum is free again
    int run = base + inc - t;
    if (out0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (i0 + u < n) {
                out0[i0 + u] = run;
                if (out1) out1[i0 + u] = run;
            }
            run += v[u];
        }
    }
    return tot;
}

__global__ __launch_bounds__(PLACE_SCAN_THREADS) void k_place_scan_sum(PlaceDb D)
{
    __shared__ int wsum[PLACE_SCAN_THREADS / 64];
    const int tot = place_scan_tile(D.inv_cur, D.nwords, blockIdx.x * PLACE_SCAN_TILE + threadIdx.x * 4,
                                    0, nullptr, nullptr, wsum);
    if (threadIdx.x == 0) D.part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PLACE_SCAN_THREADS) void k_place_scan_top(PlaceDb D, int ntiles)
{
    __shared__ int wsum[PLACE_SCAN_THREADS / 64];
    int base = 0;  // the same in every thread
    for (int b0 = 0; b0 < ntiles; b0 += PLACE_SCAN_TILE)
        base += place_scan_tile(D.part, ntiles, b0 + threadIdx.x * 4, base, D.part, nullptr, wsum);
    if (threadIdx.x == 0) D.inv_off[D.nwords] = base;
}

__global__ __launch_bounds__(PLACE_SCAN_THREADS) void k_place_scan_fin(PlaceDb D)
{
    __shared__ int wsum[PLACE_SCAN_THREADS / 64];
    place_scan_tile(D.inv_cur, D.nwords, blockIdx.x * PLACE_SCAN_TILE + threadIdx.x * 4,
                    D.part[blockIdx.x], D.inv_off, D.inv_cur, wsum);
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_fill(PlaceDb D)
{
    const int s = blockIdx.x;
    if (!D.live[s]) return;
    const int nb = D.nbow[s];
    const int32_t *w = D.words + (size_t)s * D.cap;
    for (int k = threadIdx.x; k < nb; k += PLACE_THREADS) {
        const int wd = w[k];
        if (wd >= 0 && wd < D.nwords) D.post[atomicAdd(&D.inv_cur[wd], 1)] = (uint16_t)s;
    }
}

// rank[s] = live slots added before s.  Workgroup (x, y): slots x * 256 .., compared with the
// PLACE_RANK_CHUNK slots from y * PLACE_RANK_CHUNK on; integer atomics into the zeroed rank[].
#define PLACE_RANK_CHUNK 512
__global__ __launch_bounds__(PLACE_THREADS) void k_place_rank(PlaceDb D)
{
    const int s = blockIdx.x * PLACE_THREADS + threadIdx.x;
    if (s >= D.K || !D.live[s]) return;
    const int64_t me = D.seq[s];
    const int t0 = blockIdx.y * PLACE_RANK_CHUNK, t1 = min(t0 + PLACE_RANK_CHUNK, D.K);
    int r = 0;
    for (int t = t0; t < t1; t++) r += (D.live[t] && D.seq[t] < me) ? 1 : 0;
    if (r) atomicAdd(&D.rank[s], r);
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_count(PlaceDb D)
{
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int n = 0;
    for (int s = threadIdx.x; s < D.K; s += PLACE_THREADS) n += D.live[s] ? 1 : 0;
    atomicAdd(&tot, n);
    __syncthreads();
    if (threadIdx.x == 0) D.nlive[0] = tot;
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_apply(PlaceDb D)
{
    const int s = blockIdx.x * PLACE_THREADS + threadIdx.x;
    if (s >= D.K) return;
    const unsigned long long p = D.pending[s];
    if (p) {
        D.reloc[s] = __uint_as_float((unsigned)p);
        D.pending[s] = 0;
    }
}

// ---------------------------------------------------------------------------
// queries
// ---------------------------------------------------------------------------
static __host__ __device__ inline int place_pow2(int n)
{
    int P = 64;
    while (P < n) P <<= 1;
    return P;
}
// LDS of k_place_query: packed counters [Kp / 2] u32, scores [Kp] f32 (later the dedupe's
// first-entry indices), survivor keys [pow2 >= K] u64, the query's words [qcap] i32
static __host__ __device__ inline int place_kp(int K) { return (K + 63) & ~63; }

size_t place_query_lds(int K, int qcap)
{
    return (size_t)place_pow2(K) * 8 + (size_t)place_kp(K) * 6 + (size_t)qcap * 4;
}

template <int NT, typename T, typename F>
__device__ __forceinline__ T block_reduce(T v, T *tmp, F op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = tmp[0];
#pragma unroll
    for (int k = 1; k < NT / 64; k++) r = op(r, tmp[k]);
    return r;
}

// NT threads: 256, or 1024 when the LDS a database needs leaves one workgroup per CU anyway
template <int NT>
__global__ __launch_bounds__(NT) void k_place_query(PlaceDb D, PlaceQuery Q)
{
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ int s_itmp[NT / 64];
    __shared__ float s_ftmp[NT / 64];
    __shared__ int s_ns, s_base;
    const int K = D.K, Kp = place_kp(K), tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t *surv = (uint64_t *)lds;
    float *score = (float *)(lds + (size_t)place_pow2(K) * 8);
    int *firstidx = (int *)score;
    uint32_t *cnt = (uint32_t *)(score + Kp);
    int32_t *qw = (int32_t *)(cnt + Kp / 2);

    const int q = blockIdx.x;
    const int src = Q.qindex ? Q.qindex[q] : q;
    const int nqw = min(max(Q.q.nbow[src], 0), Q.qcap);
    const int32_t *gqw = Q.q.words + (size_t)src * Q.qcap;
    const double *gqx = Q.q.weights + (size_t)src * Q.qcap;
    const bool loop = Q.loop != 0;
    const float min_score = loop ? Q.min_score[q] : 0.0f;

    for (int i = tid; i < Kp / 2; i += NT) cnt[i] = 0;
    for (int i = tid; i < nqw; i += NT) qw[i] = gqw[i];
    if (tid == 0) s_ns = 0;
    __syncthreads();
    if (loop) {  // spConnectedKeyFrames: never in lKFsSharingWords, never a counted neighbour
        const int nc = min(max(Q.nconn[q], 0), Q.conn_cap);
        for (int i = tid; i < nc; i += NT) {
            const int s = Q.conn[(size_t)q * Q.conn_cap + i];
            if (s >= 0 && s < K) atomicOr(&cnt[s >> 1], 0x8000u << ((s & 1) * 16));
        }
        __syncthreads();
    }
#define PLACE_CNT(s) ((cnt[(s) >> 1] >> (((s) & 1) * 16)) & 0xFFFFu)

    // ---- pass 1: mnRelocWords / mnLoopWords, 16 lanes per query word ----
    for (int p = tid >> 4; p < nqw; p += NT / 16) {
        const int w = qw[p];
        if (w < 0 || w >= D.nwords) continue;
        const int e1 = D.inv_off[w + 1];
        for (int e = D.inv_off[w] + (tid & 15); e < e1; e += 16) {
            const int s = D.post[e];
            atomicAdd(&cnt[s >> 1], 1u << ((s & 1) * 16));
        }
    }
    __syncthreads();
    int m = 0;
    for (int s = tid; s < K; s += NT) {
        const unsigned c = PLACE_CNT(s);
        if (!(c & 0x8000u)) m = max(m, (int)c);
    }
    const int maxc = block_reduce<NT>(m, s_itmp, [](int a, int b) { return max(a, b); });
    const int minc = (int)((float)maxc * 0.8f);  // int minCommonWords = maxCommonWords*0.8f
    for (int s = tid; s < K; s += NT) {
        const unsigned c = PLACE_CNT(s);
        if (!(c & 0x8000u) && (int)c > minc) surv[atomicAdd(&s_ns, 1)] = (uint64_t)s;  // sorted below
    }
    __syncthreads();
    const int ns = s_ns;

    // ---- pass 2: one wave per survivor, mpVoc->score(query, pKFi->mBowVec) ----
    for (int i = wv; i < ns; i += NT / 64) {
        const int s = (int)surv[i];
        int first;
        const double sc = wave_l1_score(qw, gqx, nqw, D.words + (size_t)s * D.cap,
                                        D.weights + (size_t)s * D.cap,
                                        min(max(D.nbow[s], 0), D.cap), &first);
        if (lane == 0) {
            const float si = (float)sc;
            score[s] = si;
            surv[i] = (uint64_t)max(first, 0) << 26 | (uint64_t)D.rank[s] << 13 | (uint64_t)s;
            if (!loop)  // pKFi->mRelocScore = si, applied after the call (k_place_apply)
                atomicMax(&D.pending[s],
                          (unsigned long long)(q + 1) << 32 | (unsigned long long)__float_as_uint(si));
        }
    }
    const int P = place_pow2(ns);
    for (int i = ns + tid; i < P; i += NT) surv[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += NT) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const uint64_t a = surv[i], b = surv[l];
                if ((a > b) == ((i & k) == 0)) {
                    surv[i] = b;
                    surv[l] = a;
                }
            }
            __syncthreads();
        }

    // ---- accumulate by covisibility: entry i -> (accScore, pBestKF, in lScoreAndMatch) ----
    float best_acc = min_score;  // reloc: 0
    for (int i = tid; i < ns; i += NT) {
        const int s = (int)(surv[i] & 0x1FFFu);
        const float si = score[s];
        const bool kept = !loop || si >= min_score;
        float best = si, acc = si;
        int bk = s;
        if (kept) {
            for (int j = 0; j < ORBG_KFDB_NEIGH; j++) {
                const int s2 = Q.neigh[(size_t)s * ORBG_KFDB_NEIGH + j];
                if (s2 < 0 || s2 >= K) continue;
                const unsigned c = PLACE_CNT(s2);
                if ((c & 0x8000u) || c == 0) continue;  // mnLoopQuery / mnRelocQuery != id
                float sc2;
                if ((int)c > minc)
                    sc2 = score[s2];
                else if (loop)
                    continue;
                else
                    sc2 = D.reloc[s2];  // not scored by this query: the stored mRelocScore
                acc += sc2;
                if (sc2 > best) {
                    bk = s2;
                    best = sc2;
                }
            }
            if (acc > best_acc) best_acc = acc;
        }
        surv[i] = (uint64_t)__float_as_uint(acc) << 32 | (uint64_t)bk << 1 | (kept ? 1u : 0u);
    }
    best_acc = block_reduce<NT>(best_acc, s_ftmp, [](float a, float b) { return a > b ? a : b; });
    const float retain = 0.75f * best_acc;
    __syncthreads();  // every score[] read is done: the array becomes firstidx[]

    // ---- retain, drop duplicates (first occurrence), compact in order ----
#define PLACE_RETAINED(e) (((e) & 1u) && __uint_as_float((unsigned)((e) >> 32)) > retain)
    for (int i = tid; i < ns; i += NT) {
        const uint64_t e = surv[i];
        if (PLACE_RETAINED(e)) firstidx[(e >> 1) & 0x1FFFu] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int i = tid; i < ns; i += NT) {
        const uint64_t e = surv[i];
        if (PLACE_RETAINED(e)) atomicMin(&firstidx[(e >> 1) & 0x1FFFu], i);
    }
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < ns; i0 += NT) {
        const int i = i0 + tid;
        bool out = false;
        int bk = 0;
        if (i < ns) {
            const uint64_t e = surv[i];
            bk = (int)((e >> 1) & 0x1FFFu);
            out = PLACE_RETAINED(e) && firstidx[bk] == i;
        }
        const unsigned long long mask = __ballot(out);
        const int below = __popcll(mask & ((1ull << lane) - 1));
        if (lane == 0) s_itmp[wv] = __popcll(mask);
        __syncthreads();
        int pos = s_base + below, tot = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; k++) {
            if (k < wv) pos += s_itmp[k];
            tot += s_itmp[k];
        }
        if (out && pos < Q.cand_cap) Q.cand[(size_t)q * Q.cand_cap + pos] = bk;
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        Q.ncand[q] = s_base;
        if (Q.max_common) Q.max_common[q] = maxc;
        if (Q.nscored) Q.nscored[q] = ns;
    }
#undef PLACE_CNT
#undef PLACE_RETAINED
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
static int last_rc() { return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO; }

int launch_place_score(hipStream_t st, const orbg_bow_vectors &a, const orbg_bow_vectors &b, int cap,
                       const int32_t *a_index, const int32_t *b_index, int npairs, double *score,
                       Prof *prof)
{
    if (npairs <= 0) return ORBG_OK;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "place_score", &ev);
    hipLaunchKernelGGL(k_place_score, dim3((npairs + 3) / 4), dim3(PLACE_THREADS), 0, st, a, b,
                       cap, a_index, b_index, npairs, score);
    prof_end(prof, st, "place_score", ev);
    return last_rc();
}

int launch_place_add(hipStream_t st, const PlaceDb &D, const int32_t *slots,
                     const orbg_bow_vectors &v, int vcap, const int32_t *index, int n, Prof *prof)
{
    if (n <= 0) return ORBG_OK;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "place_add", &ev);
    hipLaunchKernelGGL(k_place_add, dim3(n), dim3(PLACE_THREADS), 0, st, D, slots, v, vcap, index, n);
    hipLaunchKernelGGL(k_place_bump, dim3(1), dim3(1), 0, st, D, n);
    prof_end(prof, st, "place_add", ev);
    return last_rc();
}

int launch_place_erase(hipStream_t st, const PlaceDb &D, int slot)
{
    hipLaunchKernelGGL(k_place_erase, dim3(1), dim3(1), 0, st, D, slot);
    return last_rc();
}

int launch_place_count(hipStream_t st, const PlaceDb &D)
{
    hipLaunchKernelGGL(k_place_count, dim3(1), dim3(PLACE_THREADS), 0, st, D);
    return last_rc();
}

int launch_place_rebuild(hipStream_t st, const PlaceDb &D, Prof *prof)
{
    hipEvent_t ev = nullptr;
    if (D.nwords > 0) {
        prof_begin(prof, st, "place_hist", &ev);
        if (hipMemsetAsync(D.inv_cur, 0, (size_t)D.nwords * 4, st) != hipSuccess) return ORBG_EIO;
        hipLaunchKernelGGL(k_place_hist, dim3(D.K), dim3(PLACE_THREADS), 0, st, D);
        prof_end(prof, st, "place_hist", ev);
    }
    const int ntiles = (D.nwords + PLACE_SCAN_TILE - 1) / PLACE_SCAN_TILE;
    prof_begin(prof, st, "place_scan", &ev);
    if (ntiles > 0)
        hipLaunchKernelGGL(k_place_scan_sum, dim3(ntiles), dim3(PLACE_SCAN_THREADS), 0, st, D);
    hipLaunchKernelGGL(k_place_scan_top, dim3(1), dim3(PLACE_SCAN_THREADS), 0, st, D, ntiles);
    if (ntiles > 0)
        hipLaunchKernelGGL(k_place_scan_fin, dim3(ntiles), dim3(PLACE_SCAN_THREADS), 0, st, D);
    prof_end(prof, st, "place_scan", ev);
    if (D.nwords > 0) {
        prof_begin(prof, st, "place_fill", &ev);
        hipLaunchKernelGGL(k_place_fill, dim3(D.K), dim3(PLACE_THREADS), 0, st, D);
        prof_end(prof, st, "place_fill", ev);
    }
    prof_begin(prof, st, "place_rank", &ev);
    if (hipMemsetAsync(D.rank, 0, (size_t)D.K * 4, st) != hipSuccess) return ORBG_EIO;
    hipLaunchKernelGGL(k_place_rank,
                       dim3((D.K + PLACE_THREADS - 1) / PLACE_THREADS,
                            (D.K + PLACE_RANK_CHUNK - 1) / PLACE_RANK_CHUNK),
                       dim3(PLACE_THREADS), 0, st, D);
    prof_end(prof, st, "place_rank", ev);
    return last_rc();
}

int launch_place_query(hipStream_t st, const PlaceDb &D, const PlaceQuery &Q, Prof *prof)
{
    if (Q.nq <= 0) return ORBG_OK;
    const size_t lds = place_query_lds(D.K, Q.qcap);
    // above 40 KiB fewer than four 256-thread workgroups fit a CU's 160 KiB: one of 1024 instead
    const bool wide = lds > 40 * 1024;
    const void *fn = wide ? (const void *)k_place_query<1024> : (const void *)k_place_query<256>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return ORBG_EIO;
    hipEvent_t ev = nullptr;
    const char *name = Q.loop ? "place_loop" : "place_reloc";
    prof_begin(prof, st, name, &ev);
    if (wide)
        hipLaunchKernelGGL(k_place_query<1024>, dim3(Q.nq), dim3(1024), lds, st, D, Q);
    else
        hipLaunchKernelGGL(k_place_query<256>, dim3(Q.nq), dim3(256), lds, st, D, Q);
    if (!Q.loop)
        hipLaunchKernelGGL(k_place_apply, dim3((D.K + PLACE_THREADS - 1) / PLACE_THREADS),
                           dim3(PLACE_THREADS), 0, st, D);
    prof_end(prof, st, name, ev);
    return last_rc();
}

}  // namespace orbg
