// sim3opt_kernels.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1366-1578) for gfx950.
//
// One 256-thread workgroup per loop candidate runs the whole refinement of its Sim3, in
// k_pose_opt's structure: g2o's Levenberg-Marquardt on one VertexSim3Expmap with an
// EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ per correspondence (Huber on both),
// optimize(5), the drop test, optimize(nBad > 0 ? 10 : 5) on the kept pairs, the final test.
//
// g2o's split is kept: an iteration linearises once at the estimate (computeActiveErrors +
// buildSystem) and every trial is an error pass alone.  The Jacobian is g2o's numeric one
// (central differences, delta 1e-9, through Sim3(update) * estimate), so a linearisation
// costs 15 error evaluations per edge and a trial one; fusing the two as k_pose_opt does
// would make every rejected trial 15 times dearer for nothing.  The 14 perturbed estimates
// and their inverses depend on the candidate alone: 14 lanes compute them into LDS once per
// linearisation.
//
// Thread t takes pairs t, t + 256, ... and accumulates the robust chi2, the lower triangle of
// the 7x7 H and b in registers (36 doubles); the workgroup reduces them in a fixed order
// (butterfly within a wave, (w0 + w1) + (w2 + w3) across waves): no atomics on doubles, the
// same bits run to run and for any batch position.  Lane 0 owns the LM scalars, the 7x7
// LDLT and the Sim3 exp update (state in LDS); barriers hand estimates out and sums back.
// The dropped-pair flags live in LDS too, so the kernel needs no scratch buffer.
//
// The arithmetic is sim3opt_args.h's and g2o_math.h's __host__ __device__ functions.  fp64 throughout; no FMA
// contraction; sin / cos / exp pinned.
#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "orbg_internal.h"
#include "orbg_device.h"
#include "sim3opt_args.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

#define SO_T 256

struct SoShared {
    double red[SO_NV];
    double wred[4 * SO_NV];
    Sim3d est, est_inv;      // the vertex's estimate
    Sim3d trial, trial_inv;  // the trial estimate
    Sim3d last, last_inv;    // where the edges' errors were last computed
    Sim3d init;              // the input (the return-0 path gives it back)
    Sim3d P[SO_NP], Pinv[SO_NP];
    double H[49], b[7], x[7];
    double Hd[7][7];         // lane 0's damped copy, factorised in place
    int go, count;
    uint8_t dead[ORBG_SIM3OPT_MAX_N];
};

__global__ __launch_bounds__(SO_T) void k_sim3_opt(Sim3OptArgs A)
{
    __shared__ SoShared S;
    const int f = blockIdx.x, tid = threadIdx.x;
    const orbg_sim3opt_problem P = A.problems[f];
    const int n = sim3opt_n(P, A.cap);
    const orbg_sim3opt_corr *corrs = A.corrs + (size_t)f * A.cap;
    uint8_t *keep = A.keep + (size_t)f * A.n1cap;
    const bool fix_scale = P.fix_scale != 0;
    const double delta = so_huber_delta(P.th2);
    for (int i = tid; i < A.n1cap; i += SO_T) keep[i] = 0;
    for (int i = tid; i < n; i += SO_T) S.dead[i] = 0;
    if (tid == 0) {
        so_init(A.init[f], &S.init);
        S.est = S.init;
        S.count = 0;
    }
    __syncthreads();
    int nBad = 0, nIn = 0, its[2] = {0, 0};
    bool give_input = true;  // g2oS12 is written back only after the second optimize
    LmState lm = {0, 2, 0, 0, 0, 0};  // lane 0's
    for (int round = 0; round < 2 && n > 0; round++) {
        // ---- optimize(iters): OptimizationAlgorithmLevenberg::solve per iteration ----
        const int iters = round == 0 ? 5 : (nBad > 0 ? 10 : 5);
        for (int it = 0; it < iters; it++) {
            // computeActiveErrors + buildSystem at the estimate
            if (tid < SO_NP) so_perturbed(S.est, tid, fix_scale, &S.P[tid], &S.Pinv[tid]);
            if (tid == 64) so_inverse(S.est, &S.est_inv);
            __syncthreads();
            double p[SO_NV];
#pragma unroll
            for (int j = 0; j < SO_NV; j++) p[j] = 0;
            for (int e = tid; e < n; e += SO_T) {
                if (S.dead[e]) continue;
                SoPair E;
                so_pair(P, corrs[e], &E);
                so_add_pair(S.est, S.est_inv, S.P, S.Pinv, P, E, delta, p);
            }
            wg_reduce<SO_NV>(p, S.wred, S.red);
            if (tid == 0) {
                S.last = S.est;
                S.last_inv = S.est_inv;
                unpack_sys<7>(S.red, S.H, S.b);
                lm.currentChi = S.red[0];
                lm_begin(&lm, it, it == 0 ? lm_max_diag<7>(S.H) : 0.0);
            }
            for (;;) {
                bool ok = false;
                if (tid == 0) {
                    ok = so_lm_trial(&lm, S.H, S.b, S.est, fix_scale, S.x, &S.trial, S.Hd);
                    so_inverse(S.trial, &S.trial_inv);
                    S.last = S.trial;
                    S.last_inv = S.trial_inv;
                }
                __syncthreads();
                double chi = 0;
                for (int e = tid; e < n; e += SO_T) {
                    if (S.dead[e]) continue;
                    SoPair E;
                    so_pair(P, corrs[e], &E);
                    chi += so_pair_chi(S.trial, S.trial_inv, P, E, delta);
                }
                wg_reduce<1>(&chi, S.wred, S.red);
                if (tid == 0) {
                    double rho;
                    if (lm_trial(&lm, ok, S.red[0], lm_scale<7>(&lm, S.x, S.b), &rho)) S.est = S.trial;
                    // 1 another trial, 2 Terminate, 0 next iteration
                    S.go = lm_retry(&lm, rho) ? 1 : (lm_end(&lm, rho) ? 2 : 0);
                }
                __syncthreads();
                if (S.go != 1) break;
            }
            its[round]++;
            if (S.go == 2) break;
        }
        // ---- the drop test on the stored errors: those of the last trial evaluated ----
        int bad = 0;
        for (int e = tid; e < n; e += SO_T) {
            if (S.dead[e]) continue;
            SoPair E;
            so_pair(P, corrs[e], &E);
            if (so_is_bad(S.last, S.last_inv, P, E)) {
                S.dead[e] = 1;
                bad++;
            }
        }
        if (bad) atomicAdd(&S.count, bad);  // integers: exact in any order
        __syncthreads();
        const int total = S.count;
        __syncthreads();
        if (tid == 0) S.count = 0;
        if (round == 0) {
            nBad = total;
            if (n - nBad < 10) break;  // return 0
        } else {
            nIn = (n - nBad) - total;
            give_input = false;
        }
    }
    __syncthreads();
    if (tid == 0)
        so_result(give_input ? S.init : S.est, nIn, nBad, n, its[0], its[1], &A.results[f]);
    for (int e = tid; e < n; e += SO_T) {
        const int j = corrs[e].index1;
        if (!S.dead[e] && j >= 0 && j < A.n1cap) keep[j] = 1;
    }
}

int launch_sim3opt(hipStream_t st, const Sim3OptArgs &A, Prof *prof)
{
    if (A.npairs <= 0) return ORBG_OK;
    hipEvent_t ev = nullptr;
    prof_begin(prof, st, "sim3_opt", &ev);
    hipLaunchKernelGGL(k_sim3_opt, dim3(A.npairs), dim3(SO_T), 0, st, A);
    prof_end(prof, st, "sim3_opt", ev);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

}  // namespace orbg
