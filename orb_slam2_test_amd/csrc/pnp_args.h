// pnp_args.h -- launch arguments of PnPsolver (pnp_kernels.hip), shared with the host entry
// points (api_solvers.hip).  The EPnP arithmetic itself is in pnp_device.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbg.h"

namespace orbg {

#define ORBG_PNP_MAX_N 8192  // correspondences per candidate (as the matchers' keypoint limit)

struct PnpArgs {
    const orbg_pnp_problem *problems;  // [ncand]
    const orbg_pnp_corr *corrs;        // [ncand][cap]
    const int32_t *samples;            // [ncand][max_its][ORBG_PNP_MAX_SET]
    int32_t ncand, cap, max_its, n1cap;
    int32_t *counts;                   // [ncand][max_its]
    orbg_pnp_hyp *hyps;                // [ncand][max_its]
    unsigned long long *masks;         // [ncand][max_its][cap / 64]
    orbg_pnp_refine *refines;          // [ncand][max_its]
    unsigned long long *refined_masks; // [ncand][max_its][cap / 64]
    orbg_pnp_result *results;          // [ncand]
    uint8_t *inliers;                  // [ncand][n1cap]
};

// Correspondences the candidate really has (a count outside [0, cap] reads nothing) and the
// iterations it really runs: none when N < mRansacMinInliers (PnPsolver.cc:173), when the
// minimal set is outside 4 .. 8 or larger than N.
__host__ __device__ static inline int pnp_n(const orbg_pnp_problem &P, int cap)
{
    return (P.n < 0 || P.n > cap) ? 0 : P.n;
}
__host__ __device__ static inline int pnp_iterations(const orbg_pnp_problem &P, int cap, int max_its)
{
    const int n = pnp_n(P, cap);
    if (P.min_set < 4 || P.min_set > ORBG_PNP_MAX_SET || n < P.min_set || n < P.min_inliers) return 0;
    return P.iterations < 0 ? 0 : (P.iterations > max_its ? max_its : P.iterations);
}

struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_pnp(hipStream_t st, const PnpArgs &A, Prof *prof);

}  // namespace orbg
