// bsolve_kernels.hip -- the reduced camera system of a global bundle adjustment, S x = b_schur,
// by a block-sparse LDL^T in 6x6 blocks over several workgroups, on gfx950, fp64.
// schur_kernels.hip's dense per-segment system is (6 nfree)^2 doubles and one workgroup's
// O(n^3): right for an LBA window's ~20 free poses, not for a map's every keyframe.  Here S is
// written by k_schur_blocks*<true> straight into the block pattern of its factor L
// (bsolve_args.h: minimum-degree order, fill by symbolic elimination), and factorised
// left-looking, column by column, with k_eg_solve's arithmetic (essential_kernels.hip) in 6x6:
// L D L^T with unit lower L in scalar terms, no pivoting, a pivot that is not positive and
// finite clears ok (k_schur_backsub then writes zero increments).
//
// Schedule: the columns of one elimination-tree level share no data, so a level is one launch
// with a workgroup per column, and the launch boundary is the only dependency between
// workgroups (no flag, counter or grid barrier is waited on).  The single-column levels at the
// top of the tree are one workgroup's walk (k_bs_tail), which also starts the backward
// substitution; the remaining levels then run in reverse, a wave per column.
//
//   k_bs_level       workgroup per column j, wave per block (r, j): the block minus its
//                    updates L(r,k) D(k) L(j,k)^T, k ascending; one more wave b_j minus row j of
//                    L times y; then the diagonal block's own L D L^T and its part of L y = b
//                    by one thread in registers, the blocks below it row by row
//   k_bs_tail        the same per column for the tail's columns in order, then their backward
//                    substitution in reverse order
//   k_bs_level_back  wave per column: x_j = Ljj^-T (y_j / d_j - sum L(r,j)^T x_r), r ascending
// A wave takes its list BS_BATCH entries at a time: the entries by one load, then the blocks
// and vectors they name as 16-byte pieces by all 64 lanes into the wave's LDS region, and the
// arithmetic reads LDS -- no lane follows entry -> block -> value through dependent global
// loads.  Every sum runs in list order and nothing is accumulated atomically: two solves of
// one system give the same bytes.  The 6x6 products stay on the VALU (36 lanes, 6 dependent
// multiply-subtract pairs per entry): an MFMA form was not written -- the column's cost is the
// latency of its staged loads and of the diagonal block's scalar chain, not its flops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <set>

#include "../../include/orbg.h"
#include "bsolve_args.h"
#include "orbg_ctx.h"
#include "orbg_device.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

#define BS_WAVES 4
#define BS_TAIL_WAVES 12  // the tail's columns are the widest (up to 64 blocks with lists of 60 at 1500
                          // keyframes): 12 waves = 59 KB of staging; with 4 the tail was 3.96 ms per solve
#define BS_BATCH 8    // list entries per staging step (clique14's lists reach 12: a full and a partial step)
#define BS_PIECES 39  // 16-byte pieces per entry: two 6x6 blocks (18 each) and a 6-vector (3)
#define BS_LOADS ((BS_BATCH * BS_PIECES + 63) / 64)

template <int W>
struct BsLds {
    double2 stage[W][BS_BATCH * BS_PIECES];
    double Ld[36], dd[6], tmp[6];
};

// m (1 .. BS_BATCH) entries from `entry(u0 ..)` into `stage`: entry q's pieces at
// stage[BS_PIECES q ..]: block .x (36 doubles), block .y (36; not fetched unless TWO: the
// substitutions' entries name one block), vec[6 .z ..] (6)
template <bool TWO, class Entry>
__device__ __forceinline__ void bs_stage(Entry entry, int u0, int m, int lane, const double *L,
                                         const double *vec, double2 *stage)
{
    const int4 ent = entry(u0 + min(lane, m - 1));
    const double2 *Lp = (const double2 *)L, *vp = (const double2 *)vec;
#pragma unroll
    for (int i = 0; i < BS_LOADS; i++) {
        const int pc = lane + 64 * i, qq = pc / BS_PIECES, part = pc - BS_PIECES * qq;
        const int q = min(qq, BS_BATCH - 1);
        const int s1 = __shfl(ent.x, q, 64), s2 = __shfl(ent.y, q, 64), k = __shfl(ent.z, q, 64);
        if (qq < m && (TWO || part < 18 || part >= 36)) {
            const double2 *src = part < 18   ? Lp + (size_t)s1 * 18 + part
                                 : part < 36 ? Lp + (size_t)s2 * 18 + (part - 18)
                                             : vp + (size_t)k * 3 + (part - 36);
            stage[pc] = *src;
        }
    }
}

// kind 0: v (lane = 6 a + b < 36) -= (L1[a][c] d[c]) L2[b][c]; 1: v (lane = a < 6) -=
// L1[a][c] vec[c]; 2: v (lane = a < 6) -= L1[c][a] vec[c]; over the list's entries in order
template <int KIND, class Entry>
__device__ __forceinline__ double bs_accumulate(double v, Entry entry, int n, int lane,
                                                const double *L, const double *vec, double2 *stage)
{
    const double *sd = (const double *)stage;
    const int a = KIND == 0 ? lane / 6 : lane, b = lane - 6 * (lane / 6);
    const bool on = KIND == 0 ? lane < 36 : lane < 6;
    for (int u0 = 0; u0 < n; u0 += BS_BATCH) {
        const int m = min(BS_BATCH, n - u0);
        bs_stage<KIND == 0>(entry, u0, m, lane, L, vec, stage);
        wave_sync_lds();
        if (on)
            for (int q = 0; q < m; q++) {
                const double *e = sd + 2 * BS_PIECES * q;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    if (KIND == 0) v -= (e[6 * a + c] * e[72 + c]) * e[36 + 6 * b + c];
                    if (KIND == 1) v -= e[6 * a + c] * e[72 + c];
                    if (KIND == 2) v -= e[6 * c + a] * e[72 + c];
                }
            }
        wave_sync_lds();  // every lane's reads before the next step's writes
    }
    return v;
}

// column j of the factorisation and its part of L y = b, by a workgroup of W waves (uniform)
template <int W>
__device__ __forceinline__ void bs_column_forward(const BsArgs &B, int j, BsLds<W> &S)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c0 = B.colptr[j], nb = B.colptr[j + 1] - c0;
    for (int t = w; t <= nb; t += W) {
        if (t < nb) {  // block c0 + t minus the columns to its left
            const int s = c0 + t, u0 = B.upoff[s];
            double v = lane < 36 ? B.L[(size_t)s * 36 + lane] : 0.0;
            v = bs_accumulate<0>(v, [&](int u) { return B.up[u0 + u]; }, B.upoff[s + 1] - u0, lane,
                                 B.L, B.D, S.stage[w]);
            if (lane < 36) B.L[(size_t)s * 36 + lane] = v;
        } else {  // b's segment minus row j of L times y
            const int u0 = B.rowoff[j];
            double v = lane < 6 ? B.x[6 * (size_t)B.perm[j] + lane] : 0.0;
            v = bs_accumulate<1>(v, [&](int u) {
                    const int2 r = B.row[u0 + u];
                    return make_int4(r.x, r.x, r.y, 0);
                }, B.rowoff[j + 1] - u0, lane, B.L, B.y, S.stage[w]);
            if (lane < 6) S.tmp[lane] = v;
        }
    }
    __syncthreads();
    if (tid < 36) S.Ld[tid] = B.L[(size_t)c0 * 36 + tid];
    __syncthreads();
    if (tid == 0) {  // the diagonal block's own L D L^T, then its part of L y = b, in registers
        double M[36], d[6], yv[6];
#pragma unroll
        for (int k = 0; k < 36; k++) M[k] = S.Ld[k];
#pragma unroll
        for (int k = 0; k < 6; k++) yv[k] = S.tmp[k];
        bool neg = false;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double dk = M[k * 6 + k];
#pragma unroll
            for (int c = 0; c < k; c++) dk -= (M[k * 6 + c] * d[c]) * M[k * 6 + c];
            d[k] = dk;
            neg = neg || !(dk > 0.0) || !(dk <= DBL_MAX);
#pragma unroll
            for (int i = k + 1; i < 6; i++) {
                double v = M[i * 6 + k];
#pragma unroll
                for (int c = 0; c < k; c++) v -= (M[i * 6 + c] * d[c]) * M[k * 6 + c];
                M[i * 6 + k] = v / dk;
            }
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double v = yv[a];
#pragma unroll
            for (int c = 0; c < a; c++) v -= M[a * 6 + c] * yv[c];
            yv[a] = v;
        }
#pragma unroll
        for (int k = 0; k < 36; k++) S.Ld[k] = M[k];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            S.dd[k] = d[k];
            S.tmp[k] = yv[k];
        }
        if (neg) *B.ok = 0;  // the other columns go on (no index depends on a value); x is not used
    }
    __syncthreads();
    if (tid < 36) B.L[(size_t)c0 * 36 + tid] = S.Ld[tid];
    if (tid >= 64 && tid < 70) {
        B.D[(size_t)j * 6 + tid - 64] = S.dd[tid - 64];
        B.y[(size_t)j * 6 + tid - 64] = S.tmp[tid - 64];
    }
    // the blocks below the diagonal: (L D) Ljj^T = the updated block, row by row
    for (int t = tid; t < (nb - 1) * 6; t += 64 * W) {
        double *row = B.L + (size_t)(c0 + 1 + t / 6) * 36 + (t % 6) * 6;
        double Y[6];
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double v = row[b];
#pragma unroll
            for (int c = 0; c < b; c++) v -= Y[c] * S.Ld[b * 6 + c];
            Y[b] = v;
        }
#pragma unroll
        for (int b = 0; b < 6; b++) row[b] = Y[b] / S.dd[b];
    }
    __syncthreads();  // the tail's next column reads this one's blocks, D and y
}

// x_j = Ljj^-T (y_j / d_j - sum over the blocks below the diagonal L(r, j)^T x_r), by one wave
__device__ __forceinline__ void bs_column_backward(const BsArgs &B, int j, int lane, double2 *stage)
{
    const int c0 = B.colptr[j], nb = B.colptr[j + 1] - c0;
    double v = lane < 6 ? B.y[(size_t)j * 6 + lane] / B.D[(size_t)j * 6 + lane] : 0.0;
    v = bs_accumulate<2>(v, [&](int u) { return make_int4(c0 + 1 + u, c0 + 1 + u, B.rowidx[c0 + 1 + u], 0); },
                         nb - 1, lane, B.L, B.xs, stage);
    double *sd = (double *)stage;
    if (lane < 36) sd[lane] = B.L[(size_t)c0 * 36 + lane];
    if (lane < 6) sd[40 + lane] = v;
    wave_sync_lds();
    if (lane == 0) {
        double xv[6];
#pragma unroll
        for (int k = 0; k < 6; k++) xv[k] = sd[40 + k];
#pragma unroll
        for (int a = 5; a >= 0; a--) {
            double t = xv[a];
#pragma unroll
            for (int c = a + 1; c < 6; c++) t -= sd[c * 6 + a] * xv[c];
            xv[a] = t;
        }
#pragma unroll
        for (int k = 0; k < 6; k++) sd[40 + k] = xv[k];
    }
    wave_sync_lds();
    if (lane < 6) {
        const double r = sd[40 + lane];
        B.xs[(size_t)j * 6 + lane] = r;
        B.x[6 * (size_t)B.perm[j] + lane] = r;
    }
    wave_sync_lds();  // the region is staged into again by the wave's next column
}

__global__ __launch_bounds__(64 * BS_WAVES) void k_bs_level(BsArgs B, int first)
{
    __shared__ BsLds<BS_WAVES> S;
    bs_column_forward(B, B.lvl_cols[first + blockIdx.x], S);
}

__global__ __launch_bounds__(64 * BS_TAIL_WAVES) void k_bs_tail(BsArgs B, int first, int count)
{
    __shared__ BsLds<BS_TAIL_WAVES> S;
    for (int i = 0; i < count; i++) bs_column_forward(B, B.lvl_cols[first + i], S);
    for (int i = count - 1; i >= 0; i--) {
        if (threadIdx.x < 64) bs_column_backward(B, B.lvl_cols[first + i], threadIdx.x, S.stage[0]);
        __syncthreads();  // x of this column before the next one's wave reads it (uniform loop)
    }
}

__global__ __launch_bounds__(64 * BS_WAVES) void k_bs_level_back(BsArgs B, int first, int count)
{
    __shared__ double2 stage[BS_WAVES][BS_BATCH * BS_PIECES];
    const int w = threadIdx.x >> 6, i = blockIdx.x * BS_WAVES + w;
    if (i >= count) return;  // wave-uniform; no workgroup barrier below
    bs_column_backward(B, B.lvl_cols[first + i], threadIdx.x & 63, stage[w]);
}

// LoopClosing.cc:1101-1113 for the points global BA did not optimise: Xc = Rcw X + tcw
// (mTcwBefGBA), X' = Rwc Xc + twc (GetPoseInverse()); each a cv::gemm of float matrices: the
// three products and the translation summed in double, one rounding (tri_gemm3's rule)
__global__ __launch_bounds__(256) void k_gba_correct_points(const float *__restrict__ Tcw,
                                                            const float *__restrict__ Twc, int nkf,
                                                            const int32_t *__restrict__ ref,
                                                            const float *__restrict__ pts, int n,
                                                            float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = ref[i];
    float x[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    if (r >= 0 && r < nkf) {
        const float *T[2] = {Tcw + 12 * (size_t)r, Twc + 12 * (size_t)r};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            float y[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 3; k++) t += (double)T[h][4 * a + k] * (double)x[k];
                t += (double)T[h][4 * a + 3];
                y[a] = (float)t;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) x[a] = y[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * (size_t)i + a] = x[a];
}

int launch_gba_correct_points(hipStream_t st, const float *Tcw, const float *Twc, int nkf,
                              const int32_t *ref, const float *pts, int n, float *out)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_gba_correct_points, dim3((n + 255) / 256), dim3(256), 0, st, Tcw, Twc, nkf,
                       ref, pts, n, out);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

int launch_bsolve(hipStream_t st, const BsLaunch &B, Prof *prof)
{
    if (B.a.n <= 0) return ORBG_OK;
    hipEvent_t ev = nullptr;
    const dim3 T(64 * BS_WAVES);
    prof_begin(prof, st, "bsolve_levels", &ev);
    for (int l = 0; l < B.npar; l++)
        hipLaunchKernelGGL(k_bs_level, dim3(B.lvl_off[l + 1] - B.lvl_off[l]), T, 0, st, B.a, B.lvl_off[l]);
    prof_end(prof, st, "bsolve_levels", ev);
    if (B.ntail > 0) {
        prof_begin(prof, st, "bsolve_tail", &ev);
        hipLaunchKernelGGL(k_bs_tail, dim3(1), dim3(64 * BS_TAIL_WAVES), 0, st, B.a, B.lvl_off[B.npar],
                           B.ntail);
        prof_end(prof, st, "bsolve_tail", ev);
    }
    prof_begin(prof, st, "bsolve_back", &ev);
    for (int l = B.npar - 1; l >= 0; l--) {
        const int cnt = B.lvl_off[l + 1] - B.lvl_off[l];
        hipLaunchKernelGGL(k_bs_level_back, dim3((cnt + BS_WAVES - 1) / BS_WAVES), T, 0, st, B.a,
                           B.lvl_off[l], cnt);
    }
    prof_end(prof, st, "bsolve_back", ev);
    return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO;
}

// ---------------------------------------------------------------------------
// host: the symbolic factorisation (bsolve_args.h)
// ---------------------------------------------------------------------------
int build_bsolve_plan(const SchurPlanHost &P, BsPlanHost &B)
{
    B = BsPlanHost{};
    const int n = B.n = P.nfree;
    B.sblocks = P.nblk;
    std::vector<std::set<int>> adj(std::max(n, 1));
    for (int b = 0; b < P.nblk; b++)
        if (P.blk_i1[b] != P.blk_i2[b]) {
            adj[P.blk_i1[b]].insert(P.blk_i2[b]);
            adj[P.blk_i2[b]].insert(P.blk_i1[b]);
        }
    // minimum degree, the smallest index among those of least degree (api_essential.hip eg_plan)
    std::set<std::pair<int, int>> queue;  // (degree, free index)
    for (int v = 0; v < n; v++) queue.insert({(int)adj[v].size(), v});
    std::vector<std::vector<int>> below(std::max(n, 1));
    B.iperm.assign(std::max(n, 1), 0);
    int64_t lblocks = 0;
    while (!queue.empty()) {
        const int v = queue.begin()->second;
        queue.erase(queue.begin());
        B.iperm[v] = (int)B.perm.size();
        B.perm.push_back(v);
        std::vector<int> nb(adj[v].begin(), adj[v].end());
        lblocks += 1 + (int64_t)nb.size();
        if (lblocks > ORBG_GBA_MAX_L_BLOCKS)
            return set_err(ORBG_ENOTSUP, "more than %d blocks of L", ORBG_GBA_MAX_L_BLOCKS);
        for (int a : nb) {
            queue.erase({(int)adj[a].size(), a});
            adj[a].erase(v);
        }
        for (size_t x = 0; x < nb.size(); x++)
            for (size_t y = x + 1; y < nb.size(); y++)
                if (adj[nb[x]].insert(nb[y]).second) adj[nb[y]].insert(nb[x]);
        for (int a : nb) queue.insert({(int)adj[a].size(), a});
        below[v] = std::move(nb);
        adj[v].clear();
    }
    if (B.perm.empty()) B.perm.push_back(0);
    // L by columns (rows ascending, the diagonal first) and by rows (columns ascending)
    B.colptr.assign(n + 1, 0);
    std::vector<std::vector<int2>> rows(std::max(n, 1));
    for (int p = 0; p < n; p++) {
        std::vector<int> r;
        for (int a : below[B.perm[p]]) r.push_back(B.iperm[a]);
        std::sort(r.begin(), r.end());
        B.rowidx.push_back(p);
        for (int q : r) {
            rows[q].push_back(make_int2((int)B.rowidx.size(), p));
            B.rowidx.push_back(q);
        }
        B.colptr[p + 1] = (int)B.rowidx.size();
    }
    const int64_t nl = (int64_t)B.rowidx.size();
    B.rowoff.assign(n + 1, 0);
    B.level.assign(std::max(n, 1), 0);
    for (int p = 0; p < n; p++) {
        int lv = 0;
        for (const int2 &e : rows[p]) lv = std::max(lv, B.level[e.y] + 1);  // e.y < p: known
        B.level[p] = lv;
        B.nlevel = std::max(B.nlevel, lv + 1);
        B.row.insert(B.row.end(), rows[p].begin(), rows[p].end());
        B.rowoff[p + 1] = (int)B.row.size();
    }
    // block (r, j) -= L(r, k) D(k) L(j, k)^T over the columns k < j both rows have
    B.upoff.assign((size_t)nl + 1, 0);
    for (int j = 0; j < n; j++)
        for (int s = B.colptr[j]; s < B.colptr[j + 1]; s++) {
            const std::vector<int2> &a = rows[B.rowidx[s]], &b = rows[j];
            size_t x = 0, y = 0;
            while (x < a.size() && y < b.size()) {
                if (a[x].y < b[y].y) x++;
                else if (a[x].y > b[y].y) y++;
                else {
                    B.up.push_back(make_int4(a[x].x, b[y].x, a[x].y, 0));
                    x++;
                    y++;
                }
            }
            if ((int64_t)B.up.size() > ORBG_GBA_MAX_UPDATES)
                return set_err(ORBG_ENOTSUP, "more than %d block updates in the factorisation",
                               ORBG_GBA_MAX_UPDATES);
            B.upoff[s + 1] = (int)B.up.size();
        }
    // the schedule: columns by level; the run of single-column levels at the top is the tail
    B.lvl_off.assign(B.nlevel + 1, 0);
    for (int p = 0; p < n; p++) B.lvl_off[B.level[p] + 1]++;
    for (int l = 0; l < B.nlevel; l++) B.lvl_off[l + 1] += B.lvl_off[l];
    B.lvl_cols.assign(std::max(n, 1), 0);
    {
        std::vector<int32_t> fill(B.lvl_off.begin(), B.lvl_off.end() - 1);
        for (int p = 0; p < n; p++) B.lvl_cols[fill[B.level[p]]++] = p;
    }
    B.npar = B.nlevel;
    while (B.npar > 0 && B.lvl_off[B.npar] - B.lvl_off[B.npar - 1] == 1) B.npar--;
    B.ntail = B.nlevel - B.npar;
    // the Schur blocks' places
    B.blk_dst.assign(std::max(P.nblk, 1), 0);
    for (int b = 0; b < P.nblk; b++) {
        const int p1 = B.iperm[P.blk_i1[b]], p2 = B.iperm[P.blk_i2[b]];
        const int r = std::max(p1, p2), c = std::min(p1, p2);
        const int32_t *lo = B.rowidx.data() + B.colptr[c], *hi = B.rowidx.data() + B.colptr[c + 1];
        const int slot = (int)(std::lower_bound(lo, hi, r) - B.rowidx.data());
        B.blk_dst[b] = 2 * slot + (p2 > p1 ? 1 : 0);
    }
    if (B.up.empty()) B.up.push_back(make_int4(0, 0, 0, 0));
    if (B.row.empty()) B.row.push_back(make_int2(0, 0));
    if (B.rowidx.empty()) B.rowidx.push_back(0);
    return ORBG_OK;
}

}  // namespace orbg

using namespace orbg;

extern "C" int orbg_ba_sparse_symbolic(const int32_t *epose, const int32_t *epoint,
                                       const uint8_t *eactive, int nedge, int npose, int npoint,
                                       const uint8_t *fixed, int32_t *order_out,
                                       int32_t *colptr_out, int32_t *rowidx_out, int cap,
                                       int32_t *level_out, orbg_ba_sparse_info *info)
{
    if (nedge < 0 || npose < 0 || npoint < 0 || cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((nedge && (!epose || !epoint || !eactive)) || (npose && !fixed) || !info)
        return set_err(ORBG_EINVAL, "NULL array");
    for (int e = 0; e < nedge; e++)
        if (epose[e] < 0 || epose[e] >= npose || epoint[e] < 0 || epoint[e] >= npoint)
            return set_err(ORBG_EINVAL, "edge %d references a missing vertex", e);
    const uint8_t none = 0;
    SchurPlanHost P;
    build_schur_plan(npose, npoint, nedge, epose, epoint, eactive, npose ? fixed : &none, P);
    BsPlanHost B;
    if (int rc = build_bsolve_plan(P, B)) return rc;
    const int n = B.n, nl = n ? B.colptr[n] : 0;
    *info = orbg_ba_sparse_info{n, (int32_t)B.sblocks, nl, B.nlevel, B.ntail, 0,
                                n ? (int64_t)B.upoff[nl] : 0};
    for (int p = 0; p < n; p++) {
        if (order_out) order_out[p] = P.free_pose[B.perm[p]];
        if (level_out) level_out[p] = B.level[p];
    }
    if (colptr_out)
        for (int p = 0; p <= n; p++) colptr_out[p] = B.colptr[p];
    if (rowidx_out) {
        if (cap < nl) return set_err(ORBG_EINVAL, "%d blocks of L, room for %d", nl, cap);
        for (int s = 0; s < nl; s++) rowidx_out[s] = B.rowidx[s];
    }
    return ORBG_OK;
}
