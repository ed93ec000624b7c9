// g2o_math.h -- the fp64 arithmetic every g2o-style optimizer here restates, once: the LM's
// cube, Eigen's quaternion formulas (q = x, y, z, w), VertexSE3Expmap::oplusImpl, Eigen's
// pivoted LDLT, the unpacking of reduced sums into H and b, the pinned workgroup sum and the
// step control of OptimizationAlgorithmLevenberg::solve.  Used by PoseOptimization
// (pose_kernels.hip), LocalBundleAdjustment (ba_kernels.hip, lm_kernels.hip and the host loop
// of orbg_api.hip), OptimizeSim3 (sim3opt_args.h, sim3opt_kernels.hip, sim3opt_host.hip) and
// OptimizeEssentialGraph (essential_args.h, essential_kernels.hip, api_essential.hip).
//
// Everything but wg_reduce is __host__ __device__ with a fixed operation order (no FMA
// contraction), so a host program runs the very same statements as a kernel.  The oracles
// (oracle/pose_oracle.c, oracle/ba_oracle.c) restate all of it independently on purpose.
#pragma once

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>

#include "orbg_device.h"

#pragma clang fp contract(off)

namespace orbg {

// g2o's pow(2 rho - 1, 3) (optimization_algorithm_levenberg.cpp:135, libm pow): the exact
// cube as a double-double, rounded once (oracle/pose_oracle.c orc_lm_cube, same expression)
__host__ __device__ __forceinline__ double lm_cube(double t)
{
    const double h = t * t;
    const double l = __builtin_fma(t, t, -h);
    const double ph = h * t;
    const double pl = __builtin_fma(h, t, -ph);
    return ph + (pl + l * t);
}

// ---- Eigen's quaternion formulas ----
__host__ __device__ __forceinline__ void q_rotate(const double q[4], const double v[3], double out[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2],
                    q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0];
    uv[1] += uv[1];
    uv[2] += uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2],
                         q[0] * uv[1] - q[1] * uv[0]};
    out[0] = v[0] + q[3] * uv[0] + c[0];
    out[1] = v[1] + q[3] * uv[1] + c[1];
    out[2] = v[2] + q[3] * uv[2] + c[2];
}

__host__ __device__ __forceinline__ void q_mul(const double a[4], const double b[4], double o[4])
{
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// SE3Quat::normalizeRotation
__host__ __device__ __forceinline__ void q_normalize(double q[4])
{
    if (q[3] < 0) {
        q[0] = -q[0];
        q[1] = -q[1];
        q[2] = -q[2];
        q[3] = -q[3];
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n;
    q[1] /= n;
    q[2] /= n;
    q[3] /= n;
}

// Quaterniond(Matrix3d): no normalisation
__host__ __device__ inline void q_from_rot(const double R[3][3], double q[4])
{
    const double t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0) {
        double s = sqrt(t + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[1][0] - R[0][1]) * s;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
        q[i] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[k][j] - R[j][k]) * s;
        q[j] = (R[j][i] + R[i][j]) * s;
        q[k] = (R[k][i] + R[i][k]) * s;
    }
}

// Quaterniond::toRotationMatrix
__host__ __device__ __forceinline__ void q_to_rot(const double q[4], double R[3][3])
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0][0] = 1 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1 - (txx + tyy);
}

// VertexSE3Expmap::oplusImpl: estimate = SE3Quat::exp(update) * estimate
__host__ __device__ inline void se3_oplus(double q[4], double t[3], const double upd[6])
{
    const double w[3] = {upd[0], upd[1], upd[2]}, u[3] = {upd[3], upd[4], upd[5]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double O[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    double O2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
                V[i][j] = R[i][j];
            }
    } else {
        double s, c;
        pinned_sincos(theta, &s, &c);
        const double a = s / theta, b = (1 - c) / (theta * theta);
        const double cc = (theta - s) / (theta * theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double I = i == j ? 1.0 : 0.0;
                R[i][j] = (I + a * O[i][j]) + b * O2[i][j];
                V[i][j] = (I + b * O[i][j]) + cc * O2[i][j];
            }
    }
    double dq[4], dt[3];
    q_from_rot(R, dq);
    for (int i = 0; i < 3; i++) dt[i] = V[i][0] * u[0] + V[i][1] * u[1] + V[i][2] * u[2];
    q_normalize(dq);
    double rt[3], nq[4];
    q_rotate(dq, t, rt);
    for (int i = 0; i < 3; i++) t[i] = dt[i] + rt[i];
    q_mul(dq, q, nq);
    q_normalize(nq);
    for (int i = 0; i < 4; i++) q[i] = nq[i];
}

// ---- the N x N system of one free vertex ----
// Eigen LDLT (lower, diagonal pivoting) + solve, m factorised in place; returns isPositive()
template <int N>
__host__ __device__ bool ldlt_solve(double m[N][N], const double b[N], double x[N])
{
    int tr[N];
    int sign = 0;  // 0 zero, 1 positive semidef, 2 negative semidef, 3 indefinite
    double temp[N];
    for (int k = 0; k < N; k++) {
        int big = k;
        double bv = fabs(m[k][k]);
        for (int i = k + 1; i < N; i++)
            if (fabs(m[i][i]) > bv) {
                bv = fabs(m[i][i]);
                big = i;
            }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) {
                const double s = m[k][j];
                m[k][j] = m[big][j];
                m[big][j] = s;
            }
            for (int i = big + 1; i < N; i++) {
                const double s = m[i][k];
                m[i][k] = m[i][big];
                m[i][big] = s;
            }
            {
                const double s = m[k][k];
                m[k][k] = m[big][big];
                m[big][big] = s;
            }
            for (int i = k + 1; i < big; i++) {
                const double s = m[i][k];
                m[i][k] = m[big][i];
                m[big][i] = s;
            }
        }
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = m[j][j] * m[k][j];
            double dot = 0;
            for (int j = 0; j < k; j++) dot += m[k][j] * temp[j];
            m[k][k] -= dot;
            for (int i = k + 1; i < N; i++) {
                double s = 0;
                for (int j = 0; j < k; j++) s += m[i][j] * temp[j];
                m[i][k] -= s;
            }
        }
        const double akk = m[k][k];
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            sign = 0;
            for (int j = 0; j < N; j++) tr[j] = j;
            break;
        }
        if (k < N - 1 && valid)
            for (int i = k + 1; i < N; i++) m[i][k] /= akk;
        if (sign == 0 || sign == 1) {
            if (akk > 0) sign = 1;
            else if (akk < 0) sign = sign == 0 ? 2 : 3;
        } else if (sign == 2 && akk > 0) {
            sign = 3;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double d[N];
    for (int i = 0; i < N; i++) d[i] = b[i];
    for (int k = 0; k < N; k++) {
        const double s = d[k];
        d[k] = d[tr[k]];
        d[tr[k]] = s;
    }
    for (int i = 0; i < N; i++) {
        double s = 0;
        for (int j = 0; j < i; j++) s += m[i][j] * d[j];
        d[i] -= s;
    }
    for (int i = 0; i < N; i++) d[i] = fabs(m[i][i]) > DBL_MIN ? d[i] / m[i][i] : 0.0;
    for (int i = N - 1; i >= 0; i--) {
        double s = 0;
        for (int j = i + 1; j < N; j++) s += m[j][i] * d[j];
        d[i] -= s;
    }
    for (int k = N - 1; k >= 0; k--) {
        const double s = d[k];
        d[k] = d[tr[k]];
        d[tr[k]] = s;
    }
    for (int i = 0; i < N; i++) x[i] = d[i];
    return true;
}

// red = [chi2, lower triangle of H row by row, b] into the symmetric H[N * N] and b[N]
template <int N>
__host__ __device__ __forceinline__ void unpack_sys(const double *red, double *H, double *b)
{
    int hi = 1;
    for (int r = 0; r < N; r++)
        for (int c = 0; c <= r; c++) {
            H[r * N + c] = red[hi];
            H[c * N + r] = red[hi];
            hi++;
        }
    for (int r = 0; r < N; r++) b[r] = red[hi + r];
}

// pinned sum of NV per-thread values over a 256-thread workgroup into red[0 .. NV): butterfly
// within each wave, (w0 + w1) + (w2 + w3) across waves (wred: 4 * NV doubles of LDS).  No
// atomics on doubles: the same bits run to run, and the oracles sum in this order.
template <int NV>
__device__ void wg_reduce(const double *p, double *wred, double *red)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        double v = p[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
        if (lane == 0) wred[wv * NV + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int j = threadIdx.x;
        red[j] = (wred[j] + wred[NV + j]) + (wred[2 * NV + j] + wred[3 * NV + j]);
    }
    __syncthreads();
}

// ---- OptimizationAlgorithmLevenberg::solve's step control
// (optimization_algorithm_levenberg.cpp:61-164); one owner: lane 0, or the host ----
struct LmState {
    double lambda, ni, currentChi, iniChi;
    int nBad, qmax;
};

// the start of an iteration, currentChi being activeRobustChi2 at the estimate; maxdiag =
// max |H_jj| of the system just built (computeLambdaInit; read in iteration 0 only)
__host__ __device__ inline void lm_begin(LmState *L, int it, double maxdiag)
{
    L->iniChi = L->currentChi;
    if (it == 0) {
        L->lambda = 1e-5 * maxdiag;
        L->ni = 2;
        L->nBad = 0;
    }
    L->qmax = 0;
}

// ... under setUserLambdaInit(user_lambda): computeLambdaInit returns a positive user value
// as it is and never looks at the diagonal
__host__ __device__ inline void lm_begin(LmState *L, int it, double maxdiag, double user_lambda)
{
    lm_begin(L, it, maxdiag);
    if (it == 0 && user_lambda > 0) L->lambda = user_lambda;
}

template <int N>
__host__ __device__ __forceinline__ double lm_max_diag(const double *H)
{
    double maxd = 0;
    for (int j = 0; j < N; j++) maxd = fmax(fabs(H[j * (N + 1)]), maxd);
    return maxd;
}

// computeScale: sum x (lambda x + b)
template <int N>
__host__ __device__ __forceinline__ double lm_scale(const LmState *L, const double *x, const double *b)
{
    double scale = 0;
    for (int j = 0; j < N; j++) scale += x[j] * (L->lambda * x[j] + b[j]);
    return scale;
}

// one trial's verdict from the solver's ok, activeRobustChi2 at the trial estimate and
// computeScale: updates lambda, ni, currentChi and qmax; returns whether the step is taken
// (else the caller restores the estimate) and *rho
__host__ __device__ inline bool lm_trial(LmState *L, bool ok, double tempChi, double scale, double *rho)
{
    if (!ok) tempChi = DBL_MAX;
    double r = L->currentChi - tempChi;
    scale += 1e-3;
    r /= scale;
    const bool accepted = r > 0 && tempChi == tempChi && fabs(tempChi) <= DBL_MAX;  // isfinite
    if (accepted) {
        double alpha = 1. - lm_cube(2 * r - 1);
        alpha = fmin(alpha, 2. / 3.);
        L->lambda *= fmax(1. / 3., alpha);
        L->ni = 2;
        L->currentChi = tempChi;
    } else {
        L->lambda *= L->ni;
        L->ni *= 2;
    }
    L->qmax++;
    *rho = r;
    return accepted;
}

// the trial loop's condition (the host LM adds its force-stop flag)
__host__ __device__ inline bool lm_retry(const LmState *L, double rho) { return rho < 0 && L->qmax < 10; }

// the iteration's verdict once the trials are over: 0 go on, 1 Terminate for qmax == 10 or
// rho == 0, 2 Terminate for three iterations in a row that gained less than 1e-3 of chi2
__host__ __device__ inline int lm_end(LmState *L, double rho)
{
    if (L->qmax == 10 || rho == 0) return 1;
    if ((L->iniChi - L->currentChi) * 1e3 < L->iniChi)
        L->nBad++;
    else
        L->nBad = 0;
    return L->nBad >= 3 ? 2 : 0;
}

}  // namespace orbg
