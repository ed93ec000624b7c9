// init_kernels.hip -- Initializer (src/Initializer.cc; Tracking::MonocularInitialization):
// Initialize() of every frame pair of a batch, from the device matcher's vnMatches12 to R21,
// t21, vP3D and vbTriangulated.
//
//   k_init_prepare      one workgroup per pair: the two Normalize reductions (fp64, 256 strided
//                       partial sums and a binary tree) and the compaction of mvMatches12 by
//                       ballot and prefix scan into (x1, y1, x2, y2) records plus `first`.
//   k_init_hypothesis   a group of ORBG_INIT_HYP_LANES lanes per (pair, iteration), the groups
//                       of a 64-thread workgroup side by side: A^T A of ComputeH21 and
//                       ComputeF21 from one gather of the eight matches, both 9x9 eigen solves
//                       at once in LDS (InitWork; the lanes split the eight rotations of a
//                       round and their 72 updates), then H21i / H12i and F21i on a lane each.
//   k_init_score        the hot loop, 2 x iterations x N evaluations per pair.  A workgroup
//                       stages its pair's match records in LDS (32 KB per 2048 matches: two
//                       workgroups fit a CU's LDS) and scores 16 (model, iteration) jobs, four
//                       per wave; lanes stride over the matches, 64 decisions make one ballot
//                       word, the per-lane fp64 partial scores combine in a butterfly.
//   k_init_reconstruct  one workgroup per pair: the first strict maxima, RH and the model; one
//                       lane decomposes; all lanes run the 4 or 8 CheckRT passes over the
//                       inliers; integer counts, the order statistic by bisection on the
//                       cosines' ordered bit patterns, the decision, and the scatter of vP3D and
//                       vbTriangulated through `first`.
//
// No atomics and no order-dependent float reduction: every output is the same on every run
// and for every batch the pair is put in.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "init_args.h"
#include "init_device.h"
#include "orbg_launch.h"

namespace orbg {

#ifndef ORBG_INIT_HYP_LANES
#define ORBG_INIT_HYP_LANES 16
#endif
#define INIT_HYP_THREADS 64
#define INIT_HYP_GROUPS (INIT_HYP_THREADS / ORBG_INIT_HYP_LANES)
#define INIT_THREADS 256
#define INIT_WAVES (INIT_THREADS / 64)
#define INIT_STAGE 2048                 // match records staged at a time
#define INIT_WAVE_JOBS 4                // (model, iteration) jobs per wave
#define INIT_WG_JOBS (INIT_WAVES * INIT_WAVE_JOBS)

// keys of frame f: none for an index outside [0, nframes); the count cut at `limit`
__device__ static inline int init_frame(const InitArgs &A, int f, int limit, const orbg_keypoint **k)
{
    *k = A.kps;
    if (f < 0 || f >= A.nframes) return 0;
    *k = A.kps + (size_t)f * A.frame_stride;
    const int n = A.counts[f];
    return n < 0 ? 0 : (n > limit ? limit : n);
}

// the sums of 256 per-thread pairs: a binary tree in LDS; every thread returns both
__device__ static inline void init_block_sum2(double a, double b, double (*red)[INIT_THREADS], int tid,
                                              double *sa, double *sb)
{
    __syncthreads();
    red[0][tid] = a;
    red[1][tid] = b;
    __syncthreads();
    for (int d = INIT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) {
            red[0][tid] += red[0][tid + d];
            red[1][tid] += red[1][tid + d];
        }
        __syncthreads();
    }
    *sa = red[0][0];
    *sb = red[1][0];
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_prepare(InitArgs A)
{
    __shared__ double red[2][INIT_THREADS];
    __shared__ int wsum[INIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int lim0 = A.cap < A.frame_stride ? A.cap : A.frame_stride;
    const int lim1 = lim0 < A.match_stride ? lim0 : A.match_stride;
    const orbg_keypoint *k1, *k2;
    const int n1 = init_frame(A, A.f1[p], lim1, &k1);
    const int n2 = init_frame(A, A.f2[p], A.frame_stride, &k2);

    for (int s = 0; s < 2; s++) {  // Normalize(mvKeys1), Normalize(mvKeys2)
        const orbg_keypoint *k = s ? k2 : k1;
        const int n = s ? n2 : n1;
        double ax = 0.0, ay = 0.0, sx, sy;
        for (int i = tid; i < n; i += INIT_THREADS) ax += (double)k[i].x, ay += (double)k[i].y;
        init_block_sum2(ax, ay, red, tid, &sx, &sy);
        const float meanX = (float)(sx / n), meanY = (float)(sy / n);
        ax = 0.0, ay = 0.0;
        for (int i = tid; i < n; i += INIT_THREADS) {
            ax += (double)fabsf(k[i].x - meanX);
            ay += (double)fabsf(k[i].y - meanY);
        }
        init_block_sum2(ax, ay, red, tid, &sx, &sy);
        const float meanDevX = (float)(sx / n), meanDevY = (float)(sy / n);
        if (tid == 0) {
            InitNorm o;
            o.mx = meanX, o.my = meanY;
            o.sx = (float)(1.0 / (double)meanDevX), o.sy = (float)(1.0 / (double)meanDevY);
            A.norms[2 * (size_t)p + s] = o;
        }
    }

    // mvMatches12 (:94-109): the pairs (i, vMatches12[i]) with a match, in i order
    const int32_t *m12 = A.matches12 + (size_t)p * A.match_stride;
    float4 *recs = A.recs + (size_t)p * A.cap;
    int32_t *first = A.first + (size_t)p * A.cap;
    int base = 0;
    for (int c0 = 0; c0 < n1; c0 += INIT_THREADS) {  // uniform trip count
        const int i = c0 + tid;
        const int m = i < n1 ? m12[i] : -1;
        const bool has = m >= 0 && m < n2;
        const unsigned long long word = __ballot(has);
        const int before = __popcll(word & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(word);
        __syncthreads();
        int off = base, total = 0;
        for (int w = 0; w < INIT_WAVES; w++) {
            if (w < wave) off += wsum[w];
            total += wsum[w];
        }
        if (has) {
            const int pos = off + before;  // < n1 <= cap
            recs[pos] = make_float4(k1[i].x, k1[i].y, k2[m].x, k2[m].y);
            first[pos] = i;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) A.nmatch[p] = base;
}

__global__ __launch_bounds__(INIT_HYP_THREADS) void k_init_hypothesis(InitArgs A)
{
    __shared__ InitWork works[INIT_HYP_GROUPS];
    constexpr int G = ORBG_INIT_HYP_LANES;
    const int g = threadIdx.x / G, lane = threadIdx.x - g * G;
    InitWork *W = &works[g];
    const int64_t row = (int64_t)blockIdx.x * INIT_HYP_GROUPS + g;
    const bool inrange = row < (int64_t)A.npairs * A.max_its;
    const int p = inrange ? (int)(row / A.max_its) : 0, it = inrange ? (int)(row - (int64_t)p * A.max_its) : 0;
    const int N = A.nmatch[p];
    const bool run = inrange && it < init_iterations(A.problems[p], N, A.max_its);
    float *H21 = A.H21 + row * 9, *H12 = A.H12 + row * 9, *F21 = A.F21 + row * 9;

    if (!__syncthreads_or(run)) {  // no group of this workgroup runs
        if (inrange && lane < 9) H21[lane] = 0.f, H12[lane] = 0.f, F21[lane] = 0.f;
        return;
    }
    // every lane of the workgroup goes through every phase: a group with nothing to run
    // computes on zeros and writes zeros
    const InitNorm n1 = A.norms[2 * (size_t)p], n2 = A.norms[2 * (size_t)p + 1];
    if (lane < 8) {
        int s = -1;
        if (run) s = A.sets[row * 8 + lane];
        const bool good = s >= 0 && s < N;
        W->idx[lane] = good ? s : -1;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (good) r = A.recs[(size_t)p * A.cap + s];
        init_normalized(r, n1, n2, W->pn[lane]);
        if (!good) W->pn[lane][0] = 0.f, W->pn[lane][1] = 0.f, W->pn[lane][2] = 0.f, W->pn[lane][3] = 0.f;
    }
    __syncthreads();
    if (lane == 0) {
        bool ok = run;
        for (int k = 0; k < 8; k++) {
            ok = ok && W->idx[k] >= 0;
            for (int j = 0; j < k; j++) ok = ok && W->idx[j] != W->idx[k];
        }
        W->ok = ok ? 1 : 0;
    }
    __syncthreads();
    init_hypothesis(W, n1, n2, inrange, H21, H12, F21, lane, G);
}

// the 64 lanes' sums in a butterfly: every lane ends with the same value
__device__ static inline double init_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_score(InitArgs A)
{
    __shared__ float4 rec[INIT_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jobs = 2 * A.max_its, per_pair = (jobs + INIT_WG_JOBS - 1) / INIT_WG_JOBS;
    const int p = blockIdx.x / per_pair;
    const int j0 = (blockIdx.x - p * per_pair) * INIT_WG_JOBS + wave * INIT_WAVE_JOBS;
    const orbg_init_problem P = A.problems[p];
    const int N = A.nmatch[p], its = init_iterations(P, N, A.max_its), words = A.cap >> 6;
    const float invSigmaSquare = init_inv_sigma2(P.sigma);
    const float4 *recs = A.recs + (size_t)p * A.cap;

    // job j: model j & 1 (0: H, 1: F) of iteration j >> 1; live: it scores
    bool live[INIT_WAVE_JOBS];
    double acc[INIT_WAVE_JOBS];
#pragma unroll
    for (int jj = 0; jj < INIT_WAVE_JOBS; jj++) {
        const int j = j0 + jj, it = j >> 1;
        acc[jj] = 0.0;
        live[jj] = false;
        if (j < jobs && it < its) {
            const size_t row = (size_t)p * A.max_its + it;
            live[jj] = !init_is_zero9(((j & 1) ? A.F21 : A.H21) + row * 9);
        }
    }
    for (int c0 = 0; c0 < N; c0 += INIT_STAGE) {  // uniform over the workgroup
        const int cn = N - c0 < INIT_STAGE ? N - c0 : INIT_STAGE;
        __syncthreads();
        for (int i = tid; i < cn; i += INIT_THREADS) rec[i] = recs[c0 + i];
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < INIT_WAVE_JOBS; jj++) {
            if (!live[jj]) continue;  // uniform per wave
            const int j = j0 + jj, it = j >> 1;
            const size_t row = (size_t)p * A.max_its + it;
            unsigned long long *mask = ((j & 1) ? A.masks_f : A.masks_h) + row * words + (c0 >> 6);
            float M[18];
            if (j & 1) {
#pragma unroll
                for (int k = 0; k < 9; k++) M[k] = A.F21[row * 9 + k], M[9 + k] = 0.f;
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) M[k] = A.H21[row * 9 + k], M[9 + k] = A.H12[row * 9 + k];
            }
            for (int w = 0; (w << 6) < cn; w++) {  // uniform trip count: every lane reaches the ballot
                const int i = (w << 6) + lane;
                bool in = false;
                float t1 = 0.f, t2 = 0.f;
                if (i < cn)
                    in = (j & 1) ? init_check_f(M, rec[i], invSigmaSquare, &t1, &t2)
                                 : init_check_h(M, M + 9, rec[i], invSigmaSquare, &t1, &t2);
                const unsigned long long word = __ballot(in);
                if (lane == 0) mask[w] = word;
                acc[jj] += (double)t1;
                acc[jj] += (double)t2;
            }
        }
    }
    const int nw = (N + 63) >> 6;
#pragma unroll
    for (int jj = 0; jj < INIT_WAVE_JOBS; jj++) {
        const int j = j0 + jj, it = j >> 1;
        if (j >= jobs) continue;  // uniform per wave
        const size_t row = (size_t)p * A.max_its + it;
        unsigned long long *mask = ((j & 1) ? A.masks_f : A.masks_h) + row * words;
        const double total = init_wave_sum(acc[jj]);
        for (int w = (live[jj] ? nw : 0) + lane; w < words; w += 64) mask[w] = 0ull;
        if (lane == 0) ((j & 1) ? A.scores_f : A.scores_h)[row] = live[jj] ? (float)total : 0.f;
    }
}

struct InitRec {  // k_init_reconstruct's shared state
    InitHyp hyp[8];
    int red[INIT_THREADS];
    float redf[INIT_THREADS];
    int ng[8];
    float par[8];
    int best[2];
    float S[2], RH;
    int model, nhyp, which, success;
};

__device__ static inline int init_block_sum(int v, int *red, int tid)
{
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int d = INIT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_reconstruct(InitArgs A)
{
    __shared__ InitRec S;
    __shared__ uint32_t keys[ORBG_INIT_MAX_N];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const orbg_init_problem P = A.problems[p];
    const int N = A.nmatch[p], its = init_iterations(P, N, A.max_its), words = A.cap >> 6;
    const size_t row0 = (size_t)p * A.max_its;
    const float4 *recs = A.recs + (size_t)p * A.cap;
    const int32_t *first = A.first + (size_t)p * A.cap;
    float *p3d = A.p3d + (size_t)p * A.cap * 3;
    uint8_t *tri = A.triangulated + (size_t)p * A.cap;
    orbg_init_result *R = A.results + p;

    for (int i = tid; i < A.cap * 3; i += INIT_THREADS) p3d[i] = 0.f;
    for (int i = tid; i < A.cap; i += INIT_THREADS) tri[i] = 0;

    // FindHomography / FindFundamental's `currentScore > score` from 0: the first maximum
    for (int m = 0; m < 2; m++) {
        const float *sc = (m ? A.scores_f : A.scores_h) + row0;
        float bs = 0.f;
        int bi = -1;
        for (int i = tid; i < its; i += INIT_THREADS)
            if (sc[i] > bs) bs = sc[i], bi = i;
        __syncthreads();
        S.redf[tid] = bs;
        S.red[tid] = bi;
        __syncthreads();
        for (int d = INIT_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) {
                const float os = S.redf[tid + d];
                const int oi = S.red[tid + d];
                if (oi >= 0 && (os > S.redf[tid] || (os == S.redf[tid] && (S.red[tid] < 0 || oi < S.red[tid]))))
                    S.redf[tid] = os, S.red[tid] = oi;
            }
            __syncthreads();
        }
        if (tid == 0) S.S[m] = S.redf[0], S.best[m] = S.red[0];
    }
    __syncthreads();
    if (tid == 0) {
        S.model = init_model(S.S[0], S.S[1], &S.RH);
        if (S.best[S.model == 1 ? 0 : 1] < 0) S.model = 0;  // no matrix to decompose
        S.nhyp = 0;
        if (S.model == 1)
            S.nhyp = init_decompose_h(A.H21 + (row0 + S.best[0]) * 9, P, S.hyp) ? 8 : 0;
        else if (S.model == 2)
            init_decompose_f(A.F21 + (row0 + S.best[1]) * 9, P, S.hyp), S.nhyp = 4;
        for (int k = 0; k < 8; k++) S.ng[k] = 0, S.par[k] = 0.f;
    }
    __syncthreads();
    const int model = S.model, nhyp = S.nhyp;
    const unsigned long long *mask = nullptr;
    if (model == 1) mask = A.masks_h + (row0 + S.best[0]) * words;
    if (model == 2) mask = A.masks_f + (row0 + S.best[1]) * words;
    int ninl = 0;
    if (mask)
        for (int w = tid; w < ((N + 63) >> 6); w += INIT_THREADS) ninl += __popcll(mask[w]);
    ninl = init_block_sum(ninl, S.red, tid);
    const float th2 = init_th2(P.sigma);

    for (int h = 0; h < nhyp; h++) {  // CheckRT
        int cnt = 0;
        for (int i = tid; i < N; i += INIT_THREADS) {
            uint32_t key = INIT_NO_KEY;
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                float x3d[3], cosp;
                if (init_check_point(S.hyp[h], P, th2, recs[i], x3d, &cosp) & 1) {
                    cnt++;
                    key = init_order_key(cosp);
                }
            }
            keys[i] = key;
        }
        const int ngood = init_block_sum(cnt, S.red, tid);
        float par = 0.f;
        if (ngood > 0) {  // uniform
            // the k-th smallest key: the largest value with at most k keys below it
            const int k = ngood - 1 < 50 ? ngood - 1 : 50;
            uint32_t res = 0;
            for (int b = 31; b >= 0; b--) {
                const uint32_t cand = res | (1u << b);
                int below = 0;
                for (int i = tid; i < N; i += INIT_THREADS) below += keys[i] < cand ? 1 : 0;
                if (init_block_sum(below, S.red, tid) <= k) res = cand;
            }
            par = init_parallax(init_key_value(res));
        }
        if (tid == 0) S.ng[h] = ngood, S.par[h] = par;
        __syncthreads();
    }
    if (tid == 0) {
        S.which = -1;
        S.success = 0;
        if (model == 1 && nhyp) S.success = init_decide_h(S.ng, S.par, ninl, P, &S.which);
        if (model == 2) S.success = init_decide_f(S.ng, S.par, ninl, P, &S.which);
    }
    __syncthreads();
    const int which = S.which, success = S.success;
    int ntri = 0;
    if (success) {  // uniform: vP3D and vbTriangulated of the chosen hypothesis
        for (int i = tid; i < N; i += INIT_THREADS)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                float x3d[3], cosp;
                const int f = init_check_point(S.hyp[which], P, th2, recs[i], x3d, &cosp);
                const int i1 = first[i];  // < n1 <= cap, distinct per match
                if (f & 1) p3d[3 * i1] = x3d[0], p3d[3 * i1 + 1] = x3d[1], p3d[3 * i1 + 2] = x3d[2];
                if (f & 2) tri[i1] = 1, ntri++;
            }
    }
    ntri = init_block_sum(ntri, S.red, tid);
    if (tid == 0) {
        R->n = N;
        R->best_h = S.best[0];
        R->best_f = S.best[1];
        R->SH = S.S[0], R->SF = S.S[1], R->RH = S.RH;
        R->model = model;
        R->success = success;
        R->hyp = which;
        R->ntriangulated = ntri;
        R->ninliers = ninl;
        R->nhyp = nhyp;
    }
    if (tid < 8) R->ngood[tid] = S.ng[tid], R->parallax[tid] = S.par[tid];
    if (tid < 12) {
        const float v = success ? (tid < 9 ? S.hyp[which].R[tid] : S.hyp[which].t[tid - 9]) : 0.f;
        if (tid < 9) R->R21[tid] = v; else R->t21[tid - 9] = v;
    }
    if (tid < 96) {
        const int h = tid / 12, k = tid - 12 * h;
        const float v = h < nhyp ? (k < 9 ? S.hyp[h].R[k] : S.hyp[h].t[k - 9]) : 0.f;
        if (k < 9) R->hyp_R[h][k] = v; else R->hyp_t[h][k - 9] = v;
    }
}

size_t init_scratch_bytes(int npairs, int cap, int max_its)
{
    const size_t pc = (size_t)npairs * cap, rows = (size_t)npairs * max_its;
    return (pc * sizeof(float4) + 255) / 256 * 256 + (pc * 4 + 255) / 256 * 256 +
           ((size_t)npairs * 4 + 255) / 256 * 256 + ((size_t)npairs * 2 * sizeof(InitNorm) + 255) / 256 * 256 +
           (rows * 9 * 4 + 255) / 256 * 256;
}

void init_scratch_at(uint8_t *b, int npairs, int cap, int max_its, InitArgs *A)
{
    const size_t pc = (size_t)npairs * cap, rows = (size_t)npairs * max_its;
    auto take = [&](size_t bytes) {
        uint8_t *o = b;
        b += (bytes + 255) / 256 * 256;
        return o;
    };
    A->recs = (float4 *)take(pc * sizeof(float4));
    A->first = (int32_t *)take(pc * 4);
    A->nmatch = (int32_t *)take((size_t)npairs * 4);
    A->norms = (InitNorm *)take((size_t)npairs * 2 * sizeof(InitNorm));
    A->H12 = (float *)take(rows * 9 * 4);
}

int launch_init(hipStream_t st, const InitArgs &A, Prof *prof)
{
    hipEvent_t ev;
    const size_t rows = (size_t)A.npairs * A.max_its;
    prof_begin(prof, st, "init_prepare", &ev);
    hipLaunchKernelGGL(k_init_prepare, dim3((unsigned)A.npairs), dim3(INIT_THREADS), 0, st, A);
    prof_end(prof, st, "init_prepare", ev);
    prof_begin(prof, st, "init_hypothesis", &ev);
    hipLaunchKernelGGL(k_init_hypothesis, dim3((unsigned)((rows + INIT_HYP_GROUPS - 1) / INIT_HYP_GROUPS)),
                       dim3(INIT_HYP_THREADS), 0, st, A);
    prof_end(prof, st, "init_hypothesis", ev);
    const int per_pair = (2 * A.max_its + INIT_WG_JOBS - 1) / INIT_WG_JOBS;
    prof_begin(prof, st, "init_score", &ev);
    hipLaunchKernelGGL(k_init_score, dim3((unsigned)A.npairs * per_pair), dim3(INIT_THREADS), 0, st, A);
    prof_end(prof, st, "init_score", ev);
    prof_begin(prof, st, "init_reconstruct", &ev);
    hipLaunchKernelGGL(k_init_reconstruct, dim3((unsigned)A.npairs), dim3(INIT_THREADS), 0, st, A);
    prof_end(prof, st, "init_reconstruct", ev);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

}  // namespace orbg
