// sim3_args.h -- launch arguments and the per-hypothesis arithmetic of Sim3Solver
// (sim3_kernels.hip), shared with the host entry points (api_solvers.hip).
//
// The arithmetic is plain fp32 in a fixed operation order (the build has -ffp-contract=off),
// written as __host__ __device__ functions so that a host program can run the very same
// statements.  The 4x4 eigen solve is jacobi.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbg.h"
#include "jacobi.h"

namespace orbg {

#define ORBG_SIM3_MAX_N 8192      // correspondences per pair (as the matchers' keypoint limit)
#define ORBG_SIM3_JACOBI_SWEEPS 8 // cyclic sweeps of the 4x4 eigen solve (fixed trip count)

// One prepared correspondence (k_sim3_prepare's output, three float4 arrays [npairs][cap]):
//   a = X3Dc1.xyz, mvnMaxError1    b = X3Dc2.xyz, mvnMaxError2    c = P1im1.uv, P2im2.uv
struct Sim3Prep {
    float4 *a, *b, *c;
};

struct Sim3Args {
    const orbg_sim3_problem *problems;  // [npairs]
    const orbg_sim3_corr *corrs;        // [npairs][cap]
    const int32_t *samples;             // [npairs][max_its][3]
    int32_t npairs, cap, max_its, n1cap;
    Sim3Prep prep;
    int32_t *counts;                    // [npairs][max_its]
    orbg_sim3_hyp *hyps;                // [npairs][max_its]
    unsigned long long *masks;          // [npairs][max_its][cap / 64]
    orbg_sim3_result *results;          // [npairs]
    uint8_t *inliers12;                 // [npairs][n1cap]
};

// Correspondences the pair really has (a count outside [0, cap] reads nothing) and the
// iterations it really runs: none when N < mRansacMinInliers (Sim3Solver.cc:146) or when no
// three distinct indices exist.
__host__ __device__ static inline int sim3_n(const orbg_sim3_problem &P, int cap)
{
    return (P.n < 0 || P.n > cap) ? 0 : P.n;
}
__host__ __device__ static inline int sim3_iterations(const orbg_sim3_problem &P, int cap, int max_its)
{
    const int n = sim3_n(P, cap);
    if (n < 3 || n < P.min_inliers) return 0;
    return P.iterations < 0 ? 0 : (P.iterations > max_its ? max_its : P.iterations);
}

// mvnMaxError (Sim3Solver.cc:87-88) is a vector<size_t>: 9.210 * sigma2 in double, truncated.
__host__ __device__ static inline float sim3_threshold(float sigma2)
{
    const double v = 9.210 * (double)sigma2;
    return v >= 1.0 ? (float)(unsigned long long)v : 0.0f;
}

// Rcw * X + tcw on a 3x4 row-major pose
__host__ __device__ static inline void sim3_transform(const float *T, const float *X, float *o)
{
    for (int r = 0; r < 3; r++)
        o[r] = ((T[4 * r] * X[0] + T[4 * r + 1] * X[1]) + T[4 * r + 2] * X[2]) + T[4 * r + 3];
}

// Sim3Solver::Project / FromCameraToImage (:382-423)
__host__ __device__ static inline void sim3_project(const float *P, float fx, float fy, float cx,
                                                    float cy, float *u, float *v)
{
    const float invz = 1.0f / P[2];
    *u = fx * (P[0] * invz) + cx;
    *v = fy * (P[1] * invz) + cy;
}

// Sim3Solver::ComputeSim3 (:226-337), Horn 1987 on three point pairs: p1[k] / p2[k] = the
// camera-1 / camera-2 coordinates of sample k.  Writes R12, t12, s12; returns false for a
// degenerate sample (no positive largest eigenvalue, or a scale that is zero or not finite), where
// the reference ends with NaN or infinite poses and no inlier.
__host__ __device__ static inline bool sim3_horn(const float p1[3][3], const float p2[3][3],
                                                 bool fix_scale, orbg_sim3_hyp *H)
{
    float O1[3], O2[3], r1[3][3], r2[3][3];
    for (int d = 0; d < 3; d++) {
        O1[d] = ((p1[0][d] + p1[1][d]) + p1[2][d]) / 3.0f;
        O2[d] = ((p2[0][d] + p2[1][d]) + p2[2][d]) / 3.0f;
        for (int k = 0; k < 3; k++) {
            r1[k][d] = p1[k][d] - O1[d];
            r2[k][d] = p2[k][d] - O2[d];
        }
    }
    float M[3][3];  // Pr2 * Pr1^T
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            M[i][j] = (r2[0][i] * r1[0][j] + r2[1][i] * r1[1][j]) + r2[2][i] * r1[2][j];
    float a[4][4], v[4][4];
    a[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    a[0][1] = M[1][2] - M[2][1];
    a[0][2] = M[2][0] - M[0][2];
    a[0][3] = M[0][1] - M[1][0];
    a[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    a[1][2] = M[0][1] + M[1][0];
    a[1][3] = M[2][0] + M[0][2];
    a[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    a[2][3] = M[1][2] + M[2][1];
    a[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    for (int i = 1; i < 4; i++)
        for (int j = 0; j < i; j++) a[i][j] = a[j][i];
    jacobi_eig_sym<4, ORBG_SIM3_JACOBI_SWEEPS>(a, v);
    float lam = a[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; k++)  // static indices only: everything stays in registers
        if (a[k][k] > lam) {
            lam = a[k][k];
            qw = v[0][k];
            qx = v[1][k];
            qy = v[2][k];
            qz = v[3][k];
        }
    const float qn = 1.0f / sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw *= qn;
    qx *= qn;
    qy *= qn;
    qz *= qn;
    float *R = H->R;
    R[0] = 1.0f - 2.0f * (qy * qy + qz * qz);
    R[1] = 2.0f * (qx * qy - qw * qz);
    R[2] = 2.0f * (qx * qz + qw * qy);
    R[3] = 2.0f * (qx * qy + qw * qz);
    R[4] = 1.0f - 2.0f * (qx * qx + qz * qz);
    R[5] = 2.0f * (qy * qz - qw * qx);
    R[6] = 2.0f * (qx * qz - qw * qy);
    R[7] = 2.0f * (qy * qz + qw * qx);
    R[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
    float s = 1.0f;
    if (!fix_scale) {
        float nom = 0.0f, den = 0.0f;
        for (int k = 0; k < 3; k++)
            for (int d = 0; d < 3; d++) {
                const float p3 = (R[3 * d] * r2[k][0] + R[3 * d + 1] * r2[k][1]) + R[3 * d + 2] * r2[k][2];
                nom += r1[k][d] * p3;
                den += p3 * p3;
            }
        s = nom / den;
    }
    H->s = s;
    for (int d = 0; d < 3; d++)
        H->t[d] = O1[d] - s * ((R[3 * d] * O2[0] + R[3 * d + 1] * O2[1]) + R[3 * d + 2] * O2[2]);
    return lam > 0.0f && fabsf(s) <= 3.0e38f && s != 0.0f;  // false for NaN too
}

// T12 = [s R | t] and T21 = [(1 / s) R^T | -(1 / s) R^T t] as 3x4 row-major (:318-336)
__host__ __device__ static inline void sim3_transforms(const orbg_sim3_hyp &H, float T12[12], float T21[12])
{
    const float is = 1.0f / H.s;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            T12[4 * r + c] = H.s * H.R[3 * r + c];
            T21[4 * r + c] = is * H.R[3 * c + r];
        }
        T12[4 * r + 3] = H.t[r];
    }
    for (int r = 0; r < 3; r++)
        T21[4 * r + 3] = -((T21[4 * r] * H.t[0] + T21[4 * r + 1] * H.t[1]) + T21[4 * r + 2] * H.t[2]);
}

// Sim3Solver::CheckInliers (:340-364) for one prepared correspondence: strict <, NaN fails
__host__ __device__ static inline bool sim3_inlier(const float T12[12], const float T21[12],
                                                   const orbg_sim3_problem &P, const float4 &a,
                                                   const float4 &b, const float4 &c)
{
    const float X1[3] = {a.x, a.y, a.z}, X2[3] = {b.x, b.y, b.z};
    float q[3], u, v;
    sim3_transform(T12, X2, q);
    sim3_project(q, P.fx1, P.fy1, P.cx1, P.cy1, &u, &v);
    const float dx1 = c.x - u, dy1 = c.y - v;
    sim3_transform(T21, X1, q);
    sim3_project(q, P.fx2, P.fy2, P.cx2, P.cy2, &u, &v);
    const float dx2 = u - c.z, dy2 = v - c.w;
    const float e1 = dx1 * dx1 + dy1 * dy1, e2 = dx2 * dx2 + dy2 * dy2;
    return e1 < a.w && e2 < b.w;
}

struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_sim3(hipStream_t st, const Sim3Args &A, Prof *prof);

}  // namespace orbg
