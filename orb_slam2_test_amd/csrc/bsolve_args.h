// bsolve_args.h -- the block-sparse form of the Schur solve's reduced camera system
// (bsolve_kernels.hip): S x = b_schur by a multi-workgroup LDL^T in 6x6 blocks, for graphs
// whose free poses are too many for schur_kernels.hip's dense per-segment system
// (GlobalBundleAdjustment: every keyframe but one is free).  bsolve_kernels.hip holds the
// kernels, the host symbolic factorisation (build_bsolve_plan) and the host-only entry
// orbg_ba_sparse_symbolic over it; orbg_api.hip, which owns the orbg_ba_graph, includes this
// header for orbg_ba_graph_schur_plan_sparse (the plan's device layout and upload).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/orbg.h"
#include "schur_args.h"

namespace orbg {

// The symbolic factorisation, built on the host from a SchurPlanHost's block pattern (the
// upper blocks i1 <= i2 of S in free-pose indices):
//   order: minimum degree over the free poses' coupling graph, the smallest free index among
//     those of least degree (eg_plan's rule); perm[p] = free index eliminated p-th;
//   L by columns in elimination positions, rows ascending, the diagonal first (colptr /
//     rowidx): the pattern of S plus fill;
//   per block (r, j) its updates L(r, k) D(k) L(j, k)^T, k ascending: up[u] = (slot of
//     (r, k), slot of (j, k), k, 0) in upoff[s] .. upoff[s + 1];
//   per column j its row of L, k ascending: row[u] = (slot of (j, k), k) (the forward
//     substitution's terms);
//   level[j] = 1 + max level[k] over its row (0 without one): columns of one level share no
//     data.  lvl_cols lists the columns by level (ascending column within one), lvl_off
//     [nlevel + 1] its ranges.  The longest run of single-column levels at the top is the
//     tail (ntail columns, levels npar .. nlevel - 1): one workgroup walks it.
//   blk_dst[b]: where upper block b of the SchurPlanHost goes: 2 * slot + 1 if it is stored
//     transposed (the order puts i2 before i1), 2 * slot else.
struct BsPlanHost {
    int n = 0, nlevel = 0, npar = 0, ntail = 0;
    int64_t sblocks = 0;
    std::vector<int32_t> perm, iperm, colptr, rowidx, upoff, rowoff, level, lvl_off, lvl_cols,
        blk_dst;
    std::vector<int4> up;
    std::vector<int2> row;
};

// ORBG_OK, or ORBG_ENOTSUP past ORBG_GBA_MAX_L_BLOCKS / ORBG_GBA_MAX_UPDATES (set_err names
// the count); P: a plan of build_schur_plan
int build_bsolve_plan(const SchurPlanHost &P, BsPlanHost &B);

struct BsArgs {
    int n;                           // free poses = block columns
    const int32_t *perm;             // [n] free index of elimination position p
    const int32_t *colptr, *rowidx;  // L by columns, positions
    const int32_t *upoff;            // [nl + 1]
    const int4 *up;
    const int32_t *rowoff;           // [n + 1]
    const int2 *row;
    const int32_t *lvl_cols;         // [n] columns by level
    double *L;                       // [nl][36] S in (k_schur_blocks*<true>), L out; row-major blocks
    double *D, *y, *xs;              // [n][6] pivots, L y = b, x by position
    double *x;                       // [6 nfree] SchurArgs.x: b_schur in, x_p out, by free index
    int32_t *ok;
};

// what the launcher needs on the host: the device arguments and the schedule
struct BsLaunch {
    BsArgs a{};
    std::vector<int32_t> lvl_off;
    int npar = 0, ntail = 0;
    int64_t nl = 0;
};

struct Prof;
int launch_bsolve(hipStream_t st, const BsLaunch &B, Prof *prof);
int launch_gba_correct_points(hipStream_t st, const float *Tcw, const float *Twc, int nkf,
                              const int32_t *ref, const float *pts, int n, float *out);

}  // namespace orbg
