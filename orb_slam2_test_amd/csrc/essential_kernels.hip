// essential_kernels.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1021-1324) on
// device-resident state: the Sim3 pose graph of LoopClosing::CorrectLoop, g2o's EdgeSim3 with
// its numeric Jacobian, a block-sparse LDL^T for BlockSolver_7_3's system, and the write-back.
// The Levenberg-Marquardt loop is the host's (api_essential.hip); it reads three scalars per
// trial.  All fp64, no FMA contraction, no atomics on doubles: every sum runs in a fixed order,
// so two runs give identical bytes.
//   k_eg_measure      thread per edge: the measurement Sjw * Swi from Scw (kind 0) or Snc (kind 1)
//   k_eg_perturb      thread per (vertex, k): the 14 oplus(+-delta e_d) estimates of a vertex and
//                     their inverses, and the estimate's inverse -- once per vertex and
//                     linearisation, not once per edge
//   k_eg_linearize    16 lanes per edge: lanes 0..13 one column of Ji or Jj each (two
//                     Sim3::log), lane 14 the error; then the edge's Ji^T Ji, Ji^T Jj, Jj^T Jj,
//                     -Ji^T e, -Jj^T e spread over the workgroup
//   k_eg_assemble     thread per element of H's blocks and of b: the plan's list of
//                     contributing edges, summed in edge order
//   k_eg_errors       an LM trial's error pass: chi2 = sum e^T e, EG_RG workgroups walking the
//   k_eg_scale        edges grid-stride in index order, a tree per workgroup; k_eg_final: one
//   k_eg_final        tree over the workgroups (computeScale = sum x (lambda x + b) likewise)
//   k_eg_solve        (H + lambda I) x = b: one workgroup walks the block columns of L in
//                     elimination order (left-looking LDL^T without pivoting, a column's block
//                     updates spread over the lanes, __syncthreads() between the steps; the
//                     forward substitution rides along), then the backward substitution
//   k_eg_update       oplus of every free vertex
//   k_eg_poses        Tiw = [R(q) | t * (1 / s)] in float (:1266-1286)
//   k_eg_correct_points  thread per map point: correctedSwr.map(Srw.map(P)) (:1288-1323)
#include <hip/hip_runtime.h>

#include "essential_args.h"
#include "orbg_launch.h"

#pragma clang fp contract(off)

namespace orbg {

__global__ __launch_bounds__(256) void k_eg_measure(const orbg_eg_edge *__restrict__ edges, int nedge,
                                                    const Sim3d *__restrict__ Scw,
                                                    const Sim3d *__restrict__ Snc,
                                                    Sim3d *__restrict__ meas)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedge) return;
    const orbg_eg_edge ed = edges[e];
    const Sim3d *src = ed.kind == 0 ? Scw : Snc;
    Sim3d m;
    eg_measurement(src[ed.i], src[ed.j], &m);
    meas[e] = m;
}

__global__ __launch_bounds__(256) void k_eg_perturb(const Sim3d *__restrict__ est, int nvert,
                                                    int fix_scale, Sim3d *__restrict__ estinv,
                                                    Sim3d *__restrict__ Pp, Sim3d *__restrict__ Pi)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = t / (EG_NP + 1), k = t % (EG_NP + 1);
    if (v >= nvert) return;
    const Sim3d S = est[v];
    Sim3d a, b;
    if (k == EG_NP) {
        so_inverse(S, &a);
        estinv[v] = a;
        return;
    }
    double u[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int d = 0; d < 7; d++)
        if (d == (k >> 1)) u[d] = (k & 1) ? -EG_DELTA : EG_DELTA;
    so_oplus(S, u, fix_scale != 0, &a);
    so_inverse(a, &b);
    Pp[(size_t)v * EG_NP + k] = a;
    Pi[(size_t)v * EG_NP + k] = b;
}

#define EG_LE 16  // edges per k_eg_linearize workgroup (16 lanes each)

__global__ __launch_bounds__(256) void k_eg_linearize(EgPlan P, const Sim3d *__restrict__ est,
                                                      const Sim3d *__restrict__ estinv,
                                                      const Sim3d *__restrict__ Pp,
                                                      const Sim3d *__restrict__ Pi,
                                                      const Sim3d *__restrict__ meas,
                                                      double *__restrict__ eo)
{
    __shared__ double J[EG_LE][2][49];  // J[side][row * 7 + column]
    __shared__ double E[EG_LE][7];
    const int le = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int e = blockIdx.x * EG_LE + le;
    if (e < P.nedge && l < 15) {
        const orbg_eg_edge ed = P.edges[e];
        const Sim3d C = meas[e];
        const int side = l >= 7 ? 1 : 0, d = l - 7 * side;
        const int v = side ? ed.j : ed.i;
        if (l == 14) {
            double err[7];
            eg_error(C, est[ed.i], estinv[ed.j], err);
#pragma unroll
            for (int r = 0; r < 7; r++) E[le][r] = err[r];
        } else if (P.vfree[v] < 0) {  // the fixed vertex has no Jacobian
#pragma unroll
            for (int r = 0; r < 7; r++) J[le][side][r * 7 + d] = 0.0;
        } else {
            // column d: (e(oplus(+delta e_d)) - e(oplus(-delta e_d))) * (1 / (2 delta))
            const size_t pk = (size_t)v * EG_NP + 2 * d;
            const Sim3d Sia = side ? est[ed.i] : Pp[pk], Sib = side ? Sia : Pp[pk + 1];
            const Sim3d Sja = side ? Pi[pk] : estinv[ed.j], Sjb = side ? Pi[pk + 1] : Sja;
            const double scalar = 1.0 / (2 * EG_DELTA);
            double a[7], b[7];
            eg_error(C, Sia, Sja, a);
            eg_error(C, Sib, Sjb, b);
#pragma unroll
            for (int r = 0; r < 7; r++) J[le][side][r * 7 + d] = scalar * (a[r] - b[r]);
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < EG_LE * EG_EO; idx += 256) {
        const int q = idx / EG_EO, o = idx - q * EG_EO;
        const int e2 = blockIdx.x * EG_LE + q;
        if (e2 >= P.nedge) break;
        double v = 0.0;
        if (o < EG_EO_BI) {
            const int blk = o / 49, el = o - 49 * blk, a = el / 7, b = el - 7 * a;
            const double *Ja = J[q][blk == 2 ? 1 : 0], *Jb = J[q][blk == 0 ? 0 : 1];
#pragma unroll
            for (int r = 0; r < 7; r++) v += Ja[r * 7 + a] * Jb[r * 7 + b];
        } else {
            const int side = (o - EG_EO_BI) / 7, a = (o - EG_EO_BI) - 7 * side;
#pragma unroll
            for (int r = 0; r < 7; r++) v += J[q][side][r * 7 + a] * (-E[q][r]);
        }
        eo[(size_t)e2 * EG_EO + o] = v;
    }
}

__global__ __launch_bounds__(256) void k_eg_assemble(EgPlan P, const double *__restrict__ eo,
                                                     double *__restrict__ A, double *__restrict__ bv)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nA = (int64_t)P.lblocks * 49;
    if (t < nA) {
        const int s = (int)(t / 49), el = (int)(t - (int64_t)s * 49), a = el / 7, b = el - 7 * a;
        double acc = 0.0;
        for (int u = P.coff[s]; u < P.coff[s + 1]; u++) {
            const int code = P.clist[u], which = code & 3;
            const double *o = eo + (size_t)(code >> 2) * EG_EO;
            acc += which == 0 ? o[el] : which == 1 ? o[98 + el] : which == 2 ? o[49 + el] : o[49 + b * 7 + a];
        }
        A[t] = acc;
    } else if (t < nA + (int64_t)P.nfree * 7) {
        const int i = (int)(t - nA), p = i / 7, a = i - 7 * p;
        double acc = 0.0;
        for (int u = P.boff[p]; u < P.boff[p + 1]; u++) {
            const int code = P.blist[u];
            acc += eo[(size_t)(code >> 1) * EG_EO + EG_EO_BI + 7 * (code & 1) + a];
        }
        bv[i] = acc;
    }
}

// the workgroup's tree over its threads' partial sums (lm_kernels.hip's order)
__device__ __forceinline__ void eg_tree(double acc, double *v, double *out)
{
    const int tid = threadIdx.x;
    v[tid] = acc;
    __syncthreads();
    for (int s = EG_RT / 2; s > 0; s >>= 1) {
        if (tid < s) v[tid] = v[tid] + v[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = v[0];
}

__global__ __launch_bounds__(EG_RT) void k_eg_errors(EgPlan P, const Sim3d *__restrict__ est,
                                                     const Sim3d *__restrict__ meas,
                                                     double *__restrict__ part)
{
    __shared__ double v[EG_RT];
    double acc = 0.0;
    for (int e = blockIdx.x * EG_RT + threadIdx.x; e < P.nedge; e += EG_RG * EG_RT) {
        const orbg_eg_edge ed = P.edges[e];
        Sim3d Sjinv;
        so_inverse(est[ed.j], &Sjinv);
        double err[7], chi = 0.0;
        eg_error(meas[e], est[ed.i], Sjinv, err);
#pragma unroll
        for (int r = 0; r < 7; r++) chi += err[r] * err[r];  // information = I, no robust kernel
        acc += chi;
    }
    eg_tree(acc, v, part + blockIdx.x);
}

__global__ __launch_bounds__(EG_RT) void k_eg_scale(int n, double lambda, const double *__restrict__ x,
                                                    const double *__restrict__ b,
                                                    double *__restrict__ part)
{
    __shared__ double v[EG_RT];
    double acc = 0.0;
    for (int i = blockIdx.x * EG_RT + threadIdx.x; i < n; i += EG_RG * EG_RT)
        acc += x[i] * (lambda * x[i] + b[i]);
    eg_tree(acc, v, part + blockIdx.x);
}

__global__ __launch_bounds__(EG_RG) void k_eg_final(const double *__restrict__ part,
                                                    double *__restrict__ out)
{
    __shared__ double v[EG_RG];
    const int tid = threadIdx.x;
    v[tid] = part[tid];
    __syncthreads();
    for (int s = EG_RG / 2; s > 0; s >>= 1) {
        if (tid < s) v[tid] = v[tid] + v[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = v[0];
}

// (H + lambda I) x = b.  L D L^T with unit lower L in scalar terms: an off-diagonal block of L
// is a full 7x7, a diagonal block holds its unit lower triangle (the strict lower part is
// read) and D its seven pivots.  No pivoting: under fix_scale the scale rows are zero off the
// diagonal and their pivot is lambda.  A pivot that is not positive and finite ends the
// factorisation with ok = 0 and x = 0.
__global__ __launch_bounds__(256) void k_eg_solve(EgPlan P, EgWork W, double lambda,
                                                  int32_t *__restrict__ ok_out)
{
    __shared__ double Ld[49], dd[7], tmp[7];
    __shared__ int bad;
    const int tid = threadIdx.x, n = P.nfree;
    if (tid == 0) bad = 0;
    __syncthreads();
    int j = 0;
    for (; j < n; j++) {
        const int c0 = P.colptr[j], nb = P.colptr[j + 1] - c0;
        // column j's blocks minus the columns to its left; b's segment minus row j of L times y
        for (int w = tid; w < nb * 49 + 7; w += 256) {
            if (w < nb * 49) {
                const int s = c0 + w / 49, el = w % 49, a = el / 7, b = el - 7 * a;
                double v = W.A[(size_t)s * 49 + el];
                if (s == c0 && a == b) v += lambda;
                for (int u = P.upoff[s]; u < P.upoff[s + 1]; u++) {
                    const int4 t = P.up[u];
                    const double *L1 = W.L + (size_t)t.x * 49 + a * 7;
                    const double *L2 = W.L + (size_t)t.y * 49 + b * 7;
                    const double *dk = W.D + (size_t)t.z * 7;
#pragma unroll
                    for (int c = 0; c < 7; c++) v -= (L1[c] * dk[c]) * L2[c];
                }
                W.L[(size_t)s * 49 + el] = v;
            } else {
                const int a = w - nb * 49;
                double v = W.b[(size_t)j * 7 + a];
                for (int u = P.rowoff[j]; u < P.rowoff[j + 1]; u++) {
                    const int2 t = P.row[u];
                    const double *Lr = W.L + (size_t)t.x * 49 + a * 7;
                    const double *yk = W.y + (size_t)t.y * 7;
#pragma unroll
                    for (int c = 0; c < 7; c++) v -= Lr[c] * yk[c];
                }
                tmp[a] = v;
            }
        }
        __syncthreads();
        if (tid < 49) Ld[tid] = W.L[(size_t)c0 * 49 + tid];
        __syncthreads();
        if (tid == 0) {  // the diagonal block's own L D L^T, then its part of L y = b
            // in registers (every index is a constant once unrolled): the chain of dependent
            // operations is what a column costs
            double M[49], d[7], yv[7];
#pragma unroll
            for (int k = 0; k < 49; k++) M[k] = Ld[k];
#pragma unroll
            for (int k = 0; k < 7; k++) yv[k] = tmp[k];
            bool neg = false;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                double dk = M[k * 7 + k];
#pragma unroll
                for (int c = 0; c < k; c++) dk -= (M[k * 7 + c] * d[c]) * M[k * 7 + c];
                d[k] = dk;
                neg = neg || !(dk > 0.0) || !(dk <= DBL_MAX);
#pragma unroll
                for (int i = k + 1; i < 7; i++) {
                    double v = M[i * 7 + k];
#pragma unroll
                    for (int c = 0; c < k; c++) v -= (M[i * 7 + c] * d[c]) * M[k * 7 + c];
                    M[i * 7 + k] = v / dk;
                }
            }
#pragma unroll
            for (int a = 0; a < 7; a++) {
                double v = yv[a];
#pragma unroll
                for (int c = 0; c < a; c++) v -= M[a * 7 + c] * yv[c];
                yv[a] = v;
            }
#pragma unroll
            for (int k = 0; k < 49; k++) Ld[k] = M[k];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                dd[k] = d[k];
                tmp[k] = yv[k];
            }
            if (neg) bad = 1;
        }
        __syncthreads();
        if (bad) break;
        if (tid < 49) W.L[(size_t)c0 * 49 + tid] = Ld[tid];
        if (tid >= 64 && tid < 71) {
            W.D[(size_t)j * 7 + tid - 64] = dd[tid - 64];
            W.y[(size_t)j * 7 + tid - 64] = tmp[tid - 64];
        }
        // the blocks below the diagonal: S = (L D) Ljj^T, row by row
        for (int w = tid; w < (nb - 1) * 7; w += 256) {
            double *row = W.L + (size_t)(c0 + 1 + w / 7) * 49 + (w % 7) * 7;
            double Y[7];
#pragma unroll
            for (int b = 0; b < 7; b++) {
                double v = row[b];
#pragma unroll
                for (int c = 0; c < b; c++) v -= Y[c] * Ld[b * 7 + c];
                Y[b] = v;
            }
#pragma unroll
            for (int b = 0; b < 7; b++) row[b] = Y[b] / dd[b];
        }
        __syncthreads();
    }
    if (j < n) {  // a bad pivot (the break is uniform: `bad` is read behind a barrier)
        for (int i = tid; i < n * 7; i += 256) W.x[i] = 0.0;
        if (tid == 0) *ok_out = 0;
        return;
    }
    // D w = y, L^T x = w
    for (j = n - 1; j >= 0; j--) {
        const int c0 = P.colptr[j], nb = P.colptr[j + 1] - c0;
        if (tid < 7) {
            const int a = tid;
            double v = W.y[(size_t)j * 7 + a] / W.D[(size_t)j * 7 + a];
            for (int s = c0 + 1; s < c0 + nb; s++) {
                const double *Ls = W.L + (size_t)s * 49 + a;
                const double *xr = W.x + (size_t)P.rowidx[s] * 7;
#pragma unroll
                for (int c = 0; c < 7; c++) v -= Ls[c * 7] * xr[c];
            }
            tmp[a] = v;
        }
        __syncthreads();
        if (tid == 0) {
            const double *Ljj = W.L + (size_t)c0 * 49;
            double M[49], xv[7];
#pragma unroll
            for (int k = 0; k < 49; k++) M[k] = Ljj[k];
#pragma unroll
            for (int k = 0; k < 7; k++) xv[k] = tmp[k];
#pragma unroll
            for (int a = 6; a >= 0; a--) {
                double v = xv[a];
#pragma unroll
                for (int c = a + 1; c < 7; c++) v -= M[c * 7 + a] * xv[c];
                xv[a] = v;
            }
#pragma unroll
            for (int k = 0; k < 7; k++) tmp[k] = xv[k];
        }
        __syncthreads();
        if (tid < 7) W.x[(size_t)j * 7 + tid] = tmp[tid];
        __syncthreads();
    }
    if (tid == 0) *ok_out = 1;
}

// est may be updated in place: each thread reads its element before writing it
__global__ __launch_bounds__(256) void k_eg_update(const int32_t *__restrict__ vfree, int nvert,
                                                   const double *__restrict__ x, int fix_scale,
                                                   Sim3d *est)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvert) return;
    const int p = vfree[v];
    if (p < 0) return;
    const Sim3d S = est[v];
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = x[(size_t)p * 7 + k];
    Sim3d o;
    so_oplus(S, u, fix_scale != 0, &o);
    est[v] = o;
}

__global__ __launch_bounds__(256) void k_eg_poses(const Sim3d *__restrict__ est, int nvert,
                                                  float *__restrict__ Tiw)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvert) return;
    const Sim3d S = est[v];
    double R[3][3];
    q_to_rot(S.q, R);
    const double k = 1. / S.s;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Tiw[(size_t)v * 12 + 4 * r + c] = (float)R[r][c];
        Tiw[(size_t)v * 12 + 4 * r + 3] = (float)(S.t[r] * k);
    }
}

// a reference index outside [0, nvert) leaves its point as it is
__global__ __launch_bounds__(256) void k_eg_correct_points(const Sim3d *__restrict__ Scw,
                                                           const Sim3d *__restrict__ Siw, int nvert,
                                                           const int32_t *__restrict__ ref,
                                                           const float *__restrict__ pts, int n,
                                                           float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = ref[i];
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    if (r < 0 || r >= nvert) {
        out[3 * (size_t)i] = px;
        out[3 * (size_t)i + 1] = py;
        out[3 * (size_t)i + 2] = pz;
        return;
    }
    Sim3d Swr;
    so_inverse(Siw[r], &Swr);
    const double p[3] = {px, py, pz};
    double y[3], z[3];
    so_map(Scw[r], p, y);
    so_map(Swr, y, z);
    out[3 * (size_t)i] = (float)z[0];
    out[3 * (size_t)i + 1] = (float)z[1];
    out[3 * (size_t)i + 2] = (float)z[2];
}

// ---- launchers ----
#define EG_LAUNCH(prof, name, ...)            \
    do {                                      \
        hipEvent_t ev_ = nullptr;             \
        prof_begin(prof, st, name, &ev_);     \
        hipLaunchKernelGGL(__VA_ARGS__);      \
        prof_end(prof, st, name, ev_);        \
    } while (0)

static inline int eg_rc() { return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO; }

int launch_eg_measure(hipStream_t st, const EgPlan &P, const Sim3d *Scw, const Sim3d *Snc, Sim3d *meas)
{
    if (P.nedge <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_eg_measure, dim3((P.nedge + 255) / 256), dim3(256), 0, st, P.edges, P.nedge,
                       Scw, Snc, meas);
    return eg_rc();
}

int launch_eg_build(hipStream_t st, const EgPlan &P, const EgWork &W, const Sim3d *est, int fix_scale,
                    Prof *prof)
{
    const int64_t np = (int64_t)P.nvert * (EG_NP + 1);
    EG_LAUNCH(prof, "eg_perturb", k_eg_perturb, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st,
              est, P.nvert, fix_scale, W.estinv, W.P, W.Pinv);
    EG_LAUNCH(prof, "eg_linearize", k_eg_linearize, dim3((P.nedge + EG_LE - 1) / EG_LE), dim3(256), 0,
              st, P, est, W.estinv, W.P, W.Pinv, W.meas, W.eo);
    const int64_t na = (int64_t)P.lblocks * 49 + (int64_t)P.nfree * 7;
    EG_LAUNCH(prof, "eg_assemble", k_eg_assemble, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st,
              P, W.eo, W.A, W.b);
    return eg_rc();
}

int launch_eg_errors(hipStream_t st, const EgPlan &P, const EgWork &W, const Sim3d *est, double *out,
                     Prof *prof)
{
    EG_LAUNCH(prof, "eg_errors", k_eg_errors, dim3(EG_RG), dim3(EG_RT), 0, st, P, est, W.meas, W.part);
    hipLaunchKernelGGL(k_eg_final, dim3(1), dim3(EG_RG), 0, st, W.part, out);
    return eg_rc();
}

int launch_eg_solve(hipStream_t st, const EgPlan &P, const EgWork &W, double lambda, int32_t *ok,
                    Prof *prof)
{
    EG_LAUNCH(prof, "eg_solve", k_eg_solve, dim3(1), dim3(256), 0, st, P, W, lambda, ok);
    return eg_rc();
}

int launch_eg_update(hipStream_t st, const EgPlan &P, const EgWork &W, double lambda, Sim3d *est,
                     int fix_scale, double *scale_out, Prof *prof)
{
    hipLaunchKernelGGL(k_eg_scale, dim3(EG_RG), dim3(EG_RT), 0, st, P.nfree * 7, lambda, W.x, W.b, W.part);
    hipLaunchKernelGGL(k_eg_final, dim3(1), dim3(EG_RG), 0, st, W.part, scale_out);
    EG_LAUNCH(prof, "eg_update", k_eg_update, dim3((P.nvert + 255) / 256), dim3(256), 0, st, P.vfree,
              P.nvert, W.x, fix_scale, est);
    return eg_rc();
}

int launch_eg_poses(hipStream_t st, const Sim3d *est, int nvert, float *Tiw)
{
    if (nvert <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_eg_poses, dim3((nvert + 255) / 256), dim3(256), 0, st, est, nvert, Tiw);
    return eg_rc();
}

int launch_eg_correct_points(hipStream_t st, const Sim3d *Scw, const Sim3d *Siw, int nvert,
                             const int32_t *ref, const float *points, int n, float *out)
{
    if (n <= 0) return ORBG_OK;
    hipLaunchKernelGGL(k_eg_correct_points, dim3((n + 255) / 256), dim3(256), 0, st, Scw, Siw, nvert,
                       ref, points, n, out);
    return eg_rc();
}

}  // namespace orbg
