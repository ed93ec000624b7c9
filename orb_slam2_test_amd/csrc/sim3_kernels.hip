// sim3_kernels.hip -- Sim3Solver (src/Sim3Solver.cc; LoopClosing::ComputeSim3,
// LoopClosing.cc:530-594): every RANSAC iteration of every candidate pair in one batch.
//
//   k_sim3_prepare  one thread per (pair, correspondence): the constructor's arithmetic
//                   (:81-109): camera-frame points, own-image projections and the truncated
//                   thresholds, into three float4 arrays.
//   k_sim3_hypothesis
//                   one thread per (pair, iteration): Horn's closed form on the three
//                   sampled correspondences (sim3_args.h; a fixed number of Jacobi sweeps),
//                   the hypothesis {R, t, s} written out; all zero (s = 0) for an iteration
//                   that does not run, a bad triple or a degenerate sample.  A wave holds 64
//                   different iterations, so no lane repeats another's solve.
//   k_sim3_ransac   one wave per (pair, iteration), four waves per workgroup: the wave reads
//                   its hypothesis, and its lanes stride over the pair's correspondences; 64
//                   decisions make one ballot word, stored by lane 0, and the popcounts add
//                   up to the count.
//   k_sim3_select   one wave per pair: the sequential acceptance rule (:183-200) over the
//                   pair's counts by a prefix maximum, then the result record and the scatter
//                   of the returned iteration's mask through index1.
//
// No atomics, no LDS, no float reduction: counts are integer popcounts, so every output is
// the same on every run and for every batch the pair is put in.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "sim3_args.h"
#include "orbg_launch.h"

namespace orbg {

#define SIM3_THREADS 256
#define SIM3_WAVES (SIM3_THREADS / 64)

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_prepare(Sim3Args A)
{
    const int64_t gid = (int64_t)blockIdx.x * SIM3_THREADS + threadIdx.x;
    if (gid >= (int64_t)A.npairs * A.cap) return;
    const int p = (int)(gid / A.cap), i = (int)(gid - (int64_t)p * A.cap);
    const orbg_sim3_problem &P = A.problems[p];
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
    if (i < sim3_n(P, A.cap)) {
        const orbg_sim3_corr &K = A.corrs[gid];
        float X1[3], X2[3];
        sim3_transform(P.T1w, K.Xw1, X1);
        sim3_transform(P.T2w, K.Xw2, X2);
        sim3_project(X1, P.fx1, P.fy1, P.cx1, P.cy1, &c.x, &c.y);
        sim3_project(X2, P.fx2, P.fy2, P.cx2, P.cy2, &c.z, &c.w);
        a = make_float4(X1[0], X1[1], X1[2], sim3_threshold(K.sigma2_1));
        b = make_float4(X2[0], X2[1], X2[2], sim3_threshold(K.sigma2_2));
    }
    A.prep.a[gid] = a;
    A.prep.b[gid] = b;
    A.prep.c[gid] = c;
}

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_hypothesis(Sim3Args A)
{
    const int64_t gid = (int64_t)blockIdx.x * SIM3_THREADS + threadIdx.x;
    if (gid >= (int64_t)A.npairs * A.max_its) return;
    const int p = (int)(gid / A.max_its), it = (int)(gid - (int64_t)p * A.max_its);
    const orbg_sim3_problem &P = A.problems[p];
    const int n = sim3_n(P, A.cap);
    const size_t base = (size_t)p * A.cap;
    orbg_sim3_hyp H = {};
    bool ok = it < sim3_iterations(P, A.cap, A.max_its);
    if (ok) {
        const int32_t *S = A.samples + gid * 3;
        const int s0 = S[0], s1 = S[1], s2 = S[2];
        ok = s0 >= 0 && s0 < n && s1 >= 0 && s1 < n && s2 >= 0 && s2 < n && s0 != s1 &&
             s0 != s2 && s1 != s2;
        if (ok) {
            const int s[3] = {s0, s1, s2};
            float p1[3][3], p2[3][3];
            for (int k = 0; k < 3; k++) {
                const float4 a = A.prep.a[base + s[k]], b = A.prep.b[base + s[k]];
                p1[k][0] = a.x, p1[k][1] = a.y, p1[k][2] = a.z;
                p2[k][0] = b.x, p2[k][1] = b.y, p2[k][2] = b.z;
            }
            ok = sim3_horn(p1, p2, P.fix_scale != 0, &H);
        }
    }
    float *o = (float *)(A.hyps + gid);
    const float *h = (const float *)&H;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(orbg_sim3_hyp) / 4); k++) o[k] = ok ? h[k] : 0.0f;
}

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_ransac(Sim3Args A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (A.max_its + SIM3_WAVES - 1) / SIM3_WAVES;
    const int p = blockIdx.x / groups, it = (blockIdx.x - p * groups) * SIM3_WAVES + wave;
    if (p >= A.npairs || it >= A.max_its) return;  // uniform per wave
    const orbg_sim3_problem P = A.problems[p];  // a copy: not re-read after the mask stores
    const int n = sim3_n(P, A.cap), words = A.cap >> 6;
    const size_t row = (size_t)p * A.max_its + it, base = (size_t)p * A.cap;
    unsigned long long *mask = A.masks + row * words;

    const orbg_sim3_hyp H = A.hyps[row];
    if (H.s == 0.0f) {  // uniform: not run, a bad triple or a degenerate sample (all zero)
        for (int w = lane; w < words; w += 64) mask[w] = 0ull;
        if (lane == 0) A.counts[row] = 0;
        return;
    }
    float T12[12], T21[12];
    sim3_transforms(H, T12, T21);
    int count = 0;
    for (int w = 0; w < words; w++) {  // uniform trip count: every lane reaches the ballot
        const int i = (w << 6) + lane;
        bool in = false;
        if (i < n) in = sim3_inlier(T12, T21, P, A.prep.a[base + i], A.prep.b[base + i], A.prep.c[base + i]);
        const unsigned long long word = __ballot(in);
        if (lane == 0) mask[w] = word;
        count += __popcll(word);
    }
    if (lane == 0) A.counts[row] = count;
}

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_select(Sim3Args A)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * SIM3_WAVES + (threadIdx.x >> 6);
    if (p >= A.npairs) return;  // uniform per wave
    const orbg_sim3_problem &P = A.problems[p];
    const int n = sim3_n(P, A.cap), its = sim3_iterations(P, A.cap, A.max_its);
    const int32_t *counts = A.counts + (size_t)p * A.max_its;
    // mnBestInliers before iteration i = max(0, counts[0 .. i - 1]); i replaces the best when
    // counts[i] >= that, and is the hit when counts[i] > min_inliers as well
    int best = 0, best_iter = -1, hit_iter = -1;
    for (int c0 = 0; c0 < its && hit_iter < 0; c0 += 64) {
        const int i = c0 + lane;
        const int c = i < its ? counts[i] : -1;
        int incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl = max(incl, o);
        }
        int before = __shfl_up(incl, 1);
        before = lane == 0 ? best : max(best, before);
        const bool take = c >= before;  // false past `its` (c = -1, before >= 0)
        unsigned long long takes = __ballot(take);
        const unsigned long long hits = __ballot(take && c > P.min_inliers);
        if (hits) {
            const int l = __ffsll((long long)hits) - 1;
            hit_iter = c0 + l;
            takes &= l == 63 ? ~0ull : ((1ull << (l + 1)) - 1);
        }
        if (takes) best_iter = c0 + 63 - __clzll((long long)takes);
        best = max(best, __shfl(incl, 63));
    }
    const int ret = hit_iter >= 0 ? hit_iter : best_iter;
    const int words = A.cap >> 6;
    int ninl = 0;
    if (ret >= 0) {
        const size_t row = (size_t)p * A.max_its + ret;
        ninl = A.counts[row];
        const unsigned long long *mask = A.masks + row * words;
        const orbg_sim3_corr *K = A.corrs + (size_t)p * A.cap;
        uint8_t *out = A.inliers12 + (size_t)p * A.n1cap;  // zeroed before this kernel
        for (int i = lane; i < n; i += 64)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                const int i1 = K[i].index1;
                if (i1 >= 0 && i1 < A.n1cap) out[i1] = 1;
            }
    }
    if (lane == 0) {
        orbg_sim3_result *R = A.results + p;
        R->hit_iter = hit_iter;
        R->best_iter = best_iter;
        R->ninliers = ninl;
        // bNoMore: N < mRansacMinInliers (:146), or mnIterations >= mRansacMaxIts without a return
        R->nomore = (n < P.min_inliers || hit_iter < 0) ? 1 : 0;
        const float *h = ret >= 0 ? (const float *)(A.hyps + (size_t)p * A.max_its + ret) : nullptr;
        float *o = (float *)&R->hyp;
        for (int k = 0; k < (int)(sizeof(orbg_sim3_hyp) / 4); k++) o[k] = h ? h[k] : 0.0f;
    }
}

int launch_sim3(hipStream_t st, const Sim3Args &A, Prof *prof)
{
    hipEvent_t ev;
    if (hipMemsetAsync(A.inliers12, 0, (size_t)A.npairs * A.n1cap, st) != hipSuccess) return ORBG_EIO;
    const int64_t nprep = (int64_t)A.npairs * A.cap;
    prof_begin(prof, st, "sim3_prepare", &ev);
    hipLaunchKernelGGL(k_sim3_prepare, dim3((unsigned)((nprep + SIM3_THREADS - 1) / SIM3_THREADS)),
                       dim3(SIM3_THREADS), 0, st, A);
    prof_end(prof, st, "sim3_prepare", ev);
    const int64_t nhyp = (int64_t)A.npairs * A.max_its;
    prof_begin(prof, st, "sim3_hypothesis", &ev);
    hipLaunchKernelGGL(k_sim3_hypothesis, dim3((unsigned)((nhyp + SIM3_THREADS - 1) / SIM3_THREADS)),
                       dim3(SIM3_THREADS), 0, st, A);
    prof_end(prof, st, "sim3_hypothesis", ev);
    const int groups = (A.max_its + SIM3_WAVES - 1) / SIM3_WAVES;
    prof_begin(prof, st, "sim3_ransac", &ev);
    hipLaunchKernelGGL(k_sim3_ransac, dim3((unsigned)A.npairs * groups), dim3(SIM3_THREADS), 0, st, A);
    prof_end(prof, st, "sim3_ransac", ev);
    prof_begin(prof, st, "sim3_select", &ev);
    hipLaunchKernelGGL(k_sim3_select, dim3((A.npairs + SIM3_WAVES - 1) / SIM3_WAVES),
                       dim3(SIM3_THREADS), 0, st, A);
    prof_end(prof, st, "sim3_select", ev);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

}  // namespace orbg
