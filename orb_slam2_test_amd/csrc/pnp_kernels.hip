// pnp_kernels.hip -- PnPsolver (src/PnPsolver.cc; Tracking::Relocalization, Tracking.cc:
// 1958-2180): every EPnP RANSAC iteration of every candidate KeyFrame in one batch.
//
//   k_pnp_hypothesis  a group of ORBG_PNP_HYP_LANES lanes per (candidate, iteration), the
//                     groups of a 64-thread workgroup side by side: compute_pose on the
//                     min_set sampled correspondences (pnp_device.h).  The matrices live in
//                     LDS (PnpWork); the lanes split the 94 sums, the six rotations of a
//                     Jacobi round, the entries of L_6x10 and the three candidates.  All zero
//                     for an iteration that does not run, a bad sample or a hypothesis that
//                     is not finite.
//   k_pnp_ransac      one wave per (candidate, iteration), four waves per workgroup:
//                     CheckInliers; 64 decisions make one ballot word, stored by lane 0, and
//                     the popcounts add up to the count.
//   k_pnp_refine      one workgroup per (candidate, iteration) that exits unless the
//                     iteration is a record (count >= min_inliers and above every earlier
//                     count): Refine() on its mask.  The masked points are staged through
//                     LDS in chunks, in index order; one thread per sum adds them in that
//                     order (centroid, second moments, then the 94 sums of compute_pose);
//                     the same EPnP tail as the hypothesis kernel; CheckInliers over all n.
//   k_pnp_select      one wave per candidate: the sequential acceptance rule (:209-255) over
//                     the counts and refine records, then the result and the scatter of the
//                     returned mask through `index`.
//
// No atomics and no order-dependent float reduction: every output is the same on every run
// and for every batch the candidate is put in.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "pnp_args.h"
#include "pnp_device.h"
#include "orbg_launch.h"

namespace orbg {

#ifndef ORBG_PNP_HYP_LANES
#define ORBG_PNP_HYP_LANES 16
#endif
#define PNP_HYP_THREADS 64
#define PNP_HYP_GROUPS (PNP_HYP_THREADS / ORBG_PNP_HYP_LANES)
#define PNP_THREADS 256
#define PNP_WAVES (PNP_THREADS / 64)
#define PNP_REF_THREADS 128

struct PnpSample {
    double pw[ORBG_PNP_MAX_SET][3], uv[ORBG_PNP_MAX_SET][2];
    double rec[ORBG_PNP_MAX_SET][PNP_REC];
    double err[3];
    int idx[ORBG_PNP_MAX_SET];
    int ok;
};

__global__ __launch_bounds__(PNP_HYP_THREADS) void k_pnp_hypothesis(PnpArgs A)
{
    __shared__ PnpWork works[PNP_HYP_GROUPS];
    __shared__ PnpSample samples[PNP_HYP_GROUPS];
    constexpr int G = ORBG_PNP_HYP_LANES;
    const int g = threadIdx.x / G, lane = threadIdx.x - g * G;
    PnpWork *W = &works[g];
    PnpSample *S = &samples[g];
    const int64_t row = (int64_t)blockIdx.x * PNP_HYP_GROUPS + g;
    const bool inrange = row < (int64_t)A.ncand * A.max_its;
    const int p = inrange ? (int)(row / A.max_its) : 0, it = inrange ? (int)(row - (int64_t)p * A.max_its) : 0;
    const orbg_pnp_problem P = A.problems[p];
    const int n = pnp_n(P, A.cap);
    const int m = P.min_set < 4 ? 4 : (P.min_set > ORBG_PNP_MAX_SET ? ORBG_PNP_MAX_SET : P.min_set);
    const bool run = inrange && it < pnp_iterations(P, A.cap, A.max_its);
    const double fu = P.fx, fv = P.fy, uc = P.cx, vc = P.cy;

    if (!__syncthreads_or(run)) {  // no group of this workgroup runs (iterations past a candidate's own)
        if (inrange && lane < 12) ((double *)(A.hyps + row))[lane] = 0.0;
        return;
    }
    // every lane of the workgroup goes through every phase: a group with nothing to run
    // computes on zeros and writes zeros
    if (lane < ORBG_PNP_MAX_SET) {
        int s = -1;
        if (run && lane < m) s = A.samples[row * ORBG_PNP_MAX_SET + lane];
        const bool good = s >= 0 && s < n;
        S->idx[lane] = good ? s : -1;
        float X = 0.f, Y = 0.f, Z = 0.f, u = 0.f, v = 0.f;
        if (good) {
            const orbg_pnp_corr &K = A.corrs[(size_t)p * A.cap + s];
            X = K.Xw[0], Y = K.Xw[1], Z = K.Xw[2], u = K.uv[0], v = K.uv[1];
        }
        S->pw[lane][0] = X, S->pw[lane][1] = Y, S->pw[lane][2] = Z;
        S->uv[lane][0] = u, S->uv[lane][1] = v;
    }
    __syncthreads();
    if (lane == 0) {
        bool ok = run;
        for (int k = 0; k < m; k++) {
            ok = ok && S->idx[k] >= 0;
            for (int j = 0; j < k; j++) ok = ok && S->idx[j] != S->idx[k];
        }
        S->ok = ok ? 1 : 0;
        double c0[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < m; k++) {
            c0[0] += S->pw[k][0];
            c0[1] += S->pw[k][1];
            c0[2] += S->pw[k][2];
        }
        c0[0] /= m, c0[1] /= m, c0[2] /= m;
        for (int k = 0; k < m; k++) {
            const double d0 = S->pw[k][0] - c0[0], d1 = S->pw[k][1] - c0[1], d2 = S->pw[k][2] - c0[2];
            cov[0] += d0 * d0, cov[1] += d0 * d1, cov[2] += d0 * d2;
            cov[3] += d1 * d1, cov[4] += d1 * d2, cov[5] += d2 * d2;
        }
        pnp_control_points(W, c0, cov, (double)m);
    }
    __syncthreads();
    if (lane < m)
        pnp_point_rec(W, S->pw[lane][0], S->pw[lane][1], S->pw[lane][2], S->uv[lane][0],
                      S->uv[lane][1], uc, vc, S->rec[lane]);
    __syncthreads();
    if (lane < 4) W->afirst[lane] = S->rec[0][lane];
    for (int e = lane; e < PNP_SUMS; e += G) {
        double s = 0.0;
        for (int k = 0; k < m; k++) s += pnp_sum_term(e, S->rec[k], fu, fv);
        pnp_sum_store(W, e, s);
    }
    __syncthreads();
    pnp_tail(W, lane, G);
    if (lane < 3) {
        double s = 0.0;
        for (int k = 0; k < m; k++)
            s += pnp_reproj(W->c[lane].R, W->c[lane].t, S->pw[k][0], S->pw[k][1], S->pw[k][2],
                            S->uv[k][0], S->uv[k][1], fu, fv, uc, vc);
        S->err[lane] = s / m;
    }
    __syncthreads();
    const PnpCand *C = &W->c[pnp_choose(S->err[0], S->err[1], S->err[2])];
    const bool ok = S->ok && pnp_finite(C->R, C->t);
    if (inrange && lane < 12) {
        double *o = (double *)(A.hyps + row);
        o[lane] = ok ? (lane < 9 ? C->R[lane] : C->t[lane - 9]) : 0.0;
    }
}

__device__ static inline bool pnp_hyp_is_zero(const orbg_pnp_hyp &H)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += H.R[k] * H.R[k];
    return !(s > 0.0);
}

// CheckInliers of hypothesis H over the candidate's correspondences by one wave; returns the
// count (the same in every lane)
__device__ static inline int pnp_check_wave(const orbg_pnp_hyp &H, const orbg_pnp_problem &P,
                                            const orbg_pnp_corr *K, int n, int w0, int wstep,
                                            int words, unsigned long long *mask, int lane)
{
    const double fu = P.fx, fv = P.fy, uc = P.cx, vc = P.cy;
    int count = 0;
    for (int w = w0; w < words; w += wstep) {  // uniform trip count: every lane reaches the ballot
        const int i = (w << 6) + lane;
        bool in = false;
        if (i < n) {
            const orbg_pnp_corr k = K[i];
            in = pnp_inlier(H.R, H.t, k.Xw[0], k.Xw[1], k.Xw[2], k.uv[0], k.uv[1], k.sigma2 * P.th2,
                            fu, fv, uc, vc);
        }
        const unsigned long long word = __ballot(in);
        if (lane == 0) mask[w] = word;
        count += __popcll(word);
    }
    return count;
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_ransac(PnpArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (A.max_its + PNP_WAVES - 1) / PNP_WAVES;
    const int p = blockIdx.x / groups, it = (blockIdx.x - p * groups) * PNP_WAVES + wave;
    if (p >= A.ncand || it >= A.max_its) return;  // uniform per wave
    const orbg_pnp_problem P = A.problems[p];
    const int n = pnp_n(P, A.cap), words = A.cap >> 6;
    const size_t row = (size_t)p * A.max_its + it;
    unsigned long long *mask = A.masks + row * words;
    const orbg_pnp_hyp H = A.hyps[row];
    if (pnp_hyp_is_zero(H)) {  // uniform: not run, a bad sample or not finite (all zero)
        for (int w = lane; w < words; w += 64) mask[w] = 0ull;
        if (lane == 0) A.counts[row] = 0;
        return;
    }
    const int count = pnp_check_wave(H, P, A.corrs + (size_t)p * A.cap, n, 0, 1, words, mask, lane);
    if (lane == 0) A.counts[row] = count;
}

__global__ __launch_bounds__(PNP_REF_THREADS) void k_pnp_refine(PnpArgs A)
{
    constexpr int T = PNP_REF_THREADS;
    __shared__ PnpWork W;
    __shared__ double rec[T][PNP_REC];
    __shared__ float pts[T][5];
    __shared__ int flag[T];
    __shared__ int red[T];
    __shared__ double c0s[3], covs[6], errs[3];
    const int tid = threadIdx.x;
    const int p = blockIdx.x / A.max_its, it = blockIdx.x - p * A.max_its;
    const orbg_pnp_problem P = A.problems[p];
    if (it >= pnp_iterations(P, A.cap, A.max_its)) return;
    const size_t row0 = (size_t)p * A.max_its, row = row0 + it;
    const int cnt = A.counts[row];
    if (cnt < P.min_inliers || cnt < 1) return;
    // a record iteration: above every earlier count (mnBestInliers starts at 0)
    int mx = 0;
    for (int j = tid; j < it; j += T) mx = max(mx, A.counts[row0 + j]);
    red[tid] = mx;
    __syncthreads();
    for (int d = T / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] = max(red[tid], red[tid + d]);
        __syncthreads();
    }
    if (cnt <= red[0]) return;  // uniform

    const int n = pnp_n(P, A.cap), words = A.cap >> 6;
    const orbg_pnp_corr *K = A.corrs + (size_t)p * A.cap;
    const unsigned long long *best = A.masks + row * words;
    const double fu = P.fx, fv = P.fy, uc = P.cx, vc = P.cy;

    // stage chunk `base` of the correspondences: the point and whether the best set holds it
#define PNP_STAGE(base)                                                      \
    {                                                                        \
        const int i_ = (base) + tid;                                         \
        int f_ = 0;                                                          \
        if (i_ < n) {                                                        \
            f_ = (int)((best[i_ >> 6] >> (i_ & 63)) & 1ull);                 \
            const orbg_pnp_corr k_ = K[i_];                                  \
            pts[tid][0] = k_.Xw[0], pts[tid][1] = k_.Xw[1], pts[tid][2] = k_.Xw[2]; \
            pts[tid][3] = k_.uv[0], pts[tid][4] = k_.uv[1];                  \
        }                                                                    \
        flag[tid] = f_;                                                      \
    }

    double acc = 0.0;  // this thread's sum of the pass
    for (int base = 0; base < n; base += T) {  // choose_control_points: the centroid
        PNP_STAGE(base)
        __syncthreads();
        if (tid < 3)
            for (int k = 0; k < T; k++)
                if (flag[k]) acc += (double)pts[k][tid];
        __syncthreads();
    }
    if (tid < 3) c0s[tid] = acc / cnt;
    __syncthreads();
    acc = 0.0;
    // (a, b) of the six second moments: 00 01 02 11 12 22
    const int ca = tid < 3 ? 0 : (tid < 5 ? 1 : 2), cb = tid < 3 ? tid : (tid < 5 ? tid - 2 : 2);
    for (int base = 0; base < n; base += T) {
        PNP_STAGE(base)
        __syncthreads();
        if (tid < 6)
            for (int k = 0; k < T; k++)
                if (flag[k]) acc += ((double)pts[k][ca] - c0s[ca]) * ((double)pts[k][cb] - c0s[cb]);
        __syncthreads();
    }
    if (tid < 6) covs[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        const double c0[3] = {c0s[0], c0s[1], c0s[2]};
        const double cov[6] = {covs[0], covs[1], covs[2], covs[3], covs[4], covs[5]};
        pnp_control_points(&W, c0, cov, (double)cnt);
    }
    __syncthreads();
    acc = 0.0;
    int have_first = 0;  // thread T - 1 keeps the first point's alphas
    for (int base = 0; base < n; base += T) {
        PNP_STAGE(base)
        if (flag[tid])
            pnp_point_rec(&W, pts[tid][0], pts[tid][1], pts[tid][2], pts[tid][3], pts[tid][4], uc, vc,
                          rec[tid]);
        __syncthreads();
        if (tid < PNP_SUMS) {
            for (int k = 0; k < T; k++)
                if (flag[k]) acc += pnp_sum_term(tid, rec[k], fu, fv);
        } else if (tid == T - 1 && !have_first) {
            for (int k = 0; k < T && !have_first; k++)
                if (flag[k]) {
                    for (int j = 0; j < 4; j++) W.afirst[j] = rec[k][j];
                    have_first = 1;
                }
        }
        __syncthreads();
    }
    if (tid < PNP_SUMS) pnp_sum_store(&W, tid, acc);
    __syncthreads();
    pnp_tail(&W, tid, T);
    acc = 0.0;
    for (int base = 0; base < n; base += T) {  // reprojection_error of the three candidates
        PNP_STAGE(base)
        __syncthreads();
        if (tid < 3)
            for (int k = 0; k < T; k++)
                if (flag[k])
                    acc += pnp_reproj(W.c[tid].R, W.c[tid].t, pts[k][0], pts[k][1], pts[k][2], pts[k][3],
                                      pts[k][4], fu, fv, uc, vc);
        __syncthreads();
    }
#undef PNP_STAGE
    if (tid < 3) errs[tid] = acc / cnt;
    __syncthreads();
    const PnpCand *C = &W.c[pnp_choose(errs[0], errs[1], errs[2])];
    orbg_pnp_hyp H;
#pragma unroll
    for (int k = 0; k < 9; k++) H.R[k] = C->R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) H.t[k] = C->t[k];
    const bool finite = pnp_finite(H.R, H.t);
    int count = 0;
    if (finite) {  // uniform; the refined mask is zero otherwise (cleared before the launch)
        const int c = pnp_check_wave(H, P, K, n, tid >> 6, T / 64, words, A.refined_masks + row * words,
                                     tid & 63);
        if ((tid & 63) == 0) red[tid >> 6] = c;
        __syncthreads();
        for (int w = 0; w < T / 64; w++) count += red[w];
    }
    if (tid == 0) {
        orbg_pnp_refine *o = A.refines + row;
        o->valid = 1;
        o->count = count;
        o->ok = count > P.min_inliers ? 1 : 0;
        o->pad = 0;
    }
    if (tid < 12) {
        double *o = (double *)&A.refines[row].hyp;
        o[tid] = finite ? (tid < 9 ? C->R[tid] : C->t[tid - 9]) : 0.0;
    }
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_select(PnpArgs A)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * PNP_WAVES + (threadIdx.x >> 6);
    if (p >= A.ncand) return;  // uniform per wave
    const orbg_pnp_problem &P = A.problems[p];
    const int n = pnp_n(P, A.cap), its = pnp_iterations(P, A.cap, A.max_its);
    const size_t row0 = (size_t)p * A.max_its;
    // mvbBestInliers at iteration i is the latest record at or before i; the hit is the first
    // iteration with count >= min_inliers whose current best refined to more than min_inliers
    int best_iter = -1, best_ok = 0, hit_iter = -1;
    for (int c0 = 0; c0 < its && hit_iter < 0; c0 += 64) {
        const int i = c0 + lane;
        int valid = 0, ok = 0, c = -1;
        if (i < its) {
            c = A.counts[row0 + i];
            valid = A.refines[row0 + i].valid;
            ok = A.refines[row0 + i].ok;
        }
        unsigned long long recs = __ballot(valid != 0);
        const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
        const unsigned long long below = recs & upto;
        const int src = below ? 63 - __clzll((long long)below) : 0;
        const int okv = __shfl(ok, src);
        const int cur_ok = below ? okv : best_ok;
        const unsigned long long hits = __ballot(i < its && c >= P.min_inliers && cur_ok != 0);
        if (hits) {
            const int l = __ffsll((long long)hits) - 1;
            hit_iter = c0 + l;
            recs &= l == 63 ? ~0ull : ((1ull << (l + 1)) - 1);
        }
        const int last = recs ? 63 - __clzll((long long)recs) : 0;
        const int ok_last = __shfl(ok, last);
        if (recs) {
            best_iter = c0 + last;
            best_ok = ok_last;
        }
    }
    const int words = A.cap >> 6;
    const bool hit = hit_iter >= 0;
    int ninl = 0;
    if (best_iter >= 0) {
        const size_t row = row0 + best_iter;
        ninl = hit ? A.refines[row].count : A.counts[row];
        const unsigned long long *mask = (hit ? A.refined_masks : A.masks) + row * words;
        const orbg_pnp_corr *K = A.corrs + (size_t)p * A.cap;
        uint8_t *out = A.inliers + (size_t)p * A.n1cap;  // zeroed before this kernel
        for (int i = lane; i < n; i += 64)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                const int i1 = K[i].index;
                if (i1 >= 0 && i1 < A.n1cap) out[i1] = 1;
            }
    }
    orbg_pnp_result *R = A.results + p;
    if (lane == 0) {
        R->hit_iter = hit_iter;
        R->best_iter = best_iter;
        R->ninliers = ninl;
        // bNoMore: N < mRansacMinInliers (:173), or mnIterations >= mRansacMaxIts without a return
        R->nomore = (n < P.min_inliers || !hit) ? 1 : 0;
        R->refined = hit ? 1 : 0;
    }
    if (lane < 12) {
        float v = 0.0f;
        if (best_iter >= 0) {
            const orbg_pnp_hyp *h = hit ? &A.refines[row0 + best_iter].hyp : A.hyps + row0 + best_iter;
            const int r = lane >> 2, c = lane & 3;
            v = (float)(c < 3 ? h->R[3 * r + c] : h->t[r]);
        }
        R->Tcw[lane] = v;
    }
}

int launch_pnp(hipStream_t st, const PnpArgs &A, Prof *prof)
{
    hipEvent_t ev;
    const size_t rows = (size_t)A.ncand * A.max_its, words = (size_t)(A.cap >> 6);
    if (hipMemsetAsync(A.inliers, 0, (size_t)A.ncand * A.n1cap, st) != hipSuccess ||
        hipMemsetAsync(A.refines, 0, rows * sizeof(orbg_pnp_refine), st) != hipSuccess ||
        hipMemsetAsync(A.refined_masks, 0, rows * words * 8, st) != hipSuccess)
        return ORBG_EIO;
    prof_begin(prof, st, "pnp_hypothesis", &ev);
    hipLaunchKernelGGL(k_pnp_hypothesis, dim3((unsigned)((rows + PNP_HYP_GROUPS - 1) / PNP_HYP_GROUPS)),
                       dim3(PNP_HYP_THREADS), 0, st, A);
    prof_end(prof, st, "pnp_hypothesis", ev);
    const int groups = (A.max_its + PNP_WAVES - 1) / PNP_WAVES;
    prof_begin(prof, st, "pnp_ransac", &ev);
    hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)A.ncand * groups), dim3(PNP_THREADS), 0, st, A);
    prof_end(prof, st, "pnp_ransac", ev);
    prof_begin(prof, st, "pnp_refine", &ev);
    hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)rows), dim3(PNP_REF_THREADS), 0, st, A);
    prof_end(prof, st, "pnp_refine", ev);
    prof_begin(prof, st, "pnp_select", &ev);
    hipLaunchKernelGGL(k_pnp_select, dim3((A.ncand + PNP_WAVES - 1) / PNP_WAVES), dim3(PNP_THREADS), 0,
                       st, A);
    prof_end(prof, st, "pnp_select", ev);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

}  // namespace orbg
