// init_args.h -- launch arguments of Initializer (init_kernels.hip), shared with the host
// entry points (api_init.hip) and the one-core host program (init_host.hip).  The arithmetic
// itself is in init_device.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbg.h"

namespace orbg {

// Normalize (:984-1037) of one frame: T = [sx 0 -mx*sx; 0 sy -my*sy; 0 0 1]
struct InitNorm {
    float mx, my, sx, sy;
};

struct InitArgs {
    const orbg_init_problem *problems;  // [npairs]
    const orbg_keypoint *kps;           // frame f at kps + f * frame_stride
    const int32_t *counts;              // [nframes]
    const int32_t *f1, *f2;             // [npairs]
    const int32_t *matches12;           // [npairs][match_stride]
    const int32_t *sets;                // [npairs][max_its][8]
    int32_t frame_stride, nframes, npairs, cap, max_its, match_stride;
    // context scratch
    float4 *recs;                       // [npairs][cap]: (x1, y1, x2, y2) of mvMatches12
    int32_t *first;                     // [npairs][cap]: mvMatches12[i].first
    int32_t *nmatch;                    // [npairs]: N
    InitNorm *norms;                    // [npairs][2]
    float *H12;                         // [npairs][max_its][9]
    // outputs (the caller's, or context scratch where the caller passed NULL)
    float *scores_h, *scores_f;         // [npairs][max_its]
    float *H21, *F21;                   // [npairs][max_its][9]
    unsigned long long *masks_h, *masks_f;  // [npairs][max_its][cap / 64]
    orbg_init_result *results;          // [npairs]
    float *p3d;                         // [npairs][cap][3]
    uint8_t *triangulated;              // [npairs][cap]
};

// Iterations a pair really runs: none when N < 8 (the reference's draw is undefined there).
__host__ __device__ static inline int init_iterations(const orbg_init_problem &P, int N, int max_its)
{
    if (N < 8) return 0;
    return P.iterations < 0 ? 0 : (P.iterations > max_its ? max_its : P.iterations);
}

// bytes of the context scratch the kernels need beside the outputs
size_t init_scratch_bytes(int npairs, int cap, int max_its);
void init_scratch_at(uint8_t *b, int npairs, int cap, int max_its, InitArgs *A);

struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_init(hipStream_t st, const InitArgs &A, Prof *prof);

}  // namespace orbg
