// essential_args.h -- launch arguments and the arithmetic of Optimizer::OptimizeEssentialGraph
// (essential_kernels.hip), shared with the host entry points and the plan (api_essential.hip).
//
// What g2o evaluates per EdgeSim3 that sim3opt_args.h does not already state: Sim3::log
// (Thirdparty/g2o/g2o/types/sim3.h:148-230, with deltaR of se3_ops.hpp and Eigen's 3x3
// PartialPivLU) and EdgeSim3::computeError (types_seven_dof_expmap.h:106-114), as
// __host__ __device__ functions in fp64 with a fixed operation order.  exp, product, inverse,
// map and oplus are sim3opt_args.h's, the step control is g2o_math.h's.
#pragma once

#include "sim3opt_args.h"

#pragma clang fp contract(off)

namespace orbg {

// blocks (7x7) of H, of its factor L including fill, and entries of the factor's update lists
// one graph may have; past either the plan returns ORBG_ENOTSUP
#define ORBG_EG_MAX_BLOCKS 262144
#define ORBG_EG_MAX_UPDATES (1 << 24)
#define ORBG_EG_MAX_EDGES (1 << 26)
#define EG_DELTA 1e-9  // base_binary_edge.hpp:147
#define EG_NP 14       // perturbed estimates of a vertex: +-delta per column
// one edge's linearisation: Ji^T Ji, Ji^T Jj, Jj^T Jj (7x7, row-major), -Ji^T e, -Jj^T e
#define EG_EO 161
#define EG_EO_BI 147
#define EG_RG 64   // reduction workgroups (as lm_kernels.hip)
#define EG_RT 256

// W.lu().solve(t): Eigen's PartialPivLU of a 3x3 (largest |entry| of the column at or below
// the diagonal, first on ties), W factorised in place
__host__ __device__ static inline void eg_lu_solve3(double W[3][3], const double t[3], double x[3])
{
    double b[3] = {t[0], t[1], t[2]};
    for (int k = 0; k < 3; k++) {
        int big = k;
        double bv = fabs(W[k][k]);
        for (int i = k + 1; i < 3; i++)
            if (fabs(W[i][k]) > bv) {
                bv = fabs(W[i][k]);
                big = i;
            }
        if (big != k) {
            for (int c = 0; c < 3; c++) {
                const double s = W[k][c];
                W[k][c] = W[big][c];
                W[big][c] = s;
            }
            const double s = b[k];
            b[k] = b[big];
            b[big] = s;
        }
        for (int i = k + 1; i < 3; i++) {
            W[i][k] /= W[k][k];
            for (int c = k + 1; c < 3; c++) W[i][c] -= W[i][k] * W[k][c];
        }
    }
    for (int i = 1; i < 3; i++)
        for (int c = 0; c < i; c++) b[i] -= W[i][c] * b[c];
    for (int i = 2; i >= 0; i--) {
        for (int c = i + 1; c < 3; c++) b[i] -= W[i][c] * b[c];
        b[i] /= W[i][i];
    }
    x[0] = b[0];
    x[1] = b[1];
    x[2] = b[2];
}

// Sim3::log, sim3.h:148-230: (omega, upsilon, sigma), four branches on |sigma| < 1e-5 and
// d > 1 - 1e-5 (d = (trace R - 1) / 2)
__host__ __device__ static inline void eg_log(const Sim3d &S, double res[7])
{
    const double sigma = log(S.s);
    double R[3][3];
    q_to_rot(S.q, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const double eps = 0.00001;
    double A, B, C, k;
    double sn = 0, cs = 1, theta = 0;
    const bool small = d > 1 - eps;
    if (!small) {
        theta = acos(d);
        pinned_sincos(theta, &sn, &cs);
        k = theta / (2 * sqrt(1 - d * d));
    } else {
        k = 0.5;
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta;
            const double a = S.s * sn, b = S.s * cs;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double w[3] = {k * dR[0], k * dR[1], k * dR[2]};
    const double O[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    double W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double O2 = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
            W[i][j] = (A * O[i][j] + B * O2) + (i == j ? C : 0.0);
        }
    eg_lu_solve3(W, S.t, res + 3);
    res[0] = w[0];
    res[1] = w[1];
    res[2] = w[2];
    res[6] = sigma;
}

// EdgeSim3::computeError: (C * v1->estimate() * v2->estimate().inverse()).log(), vertex 0 of
// the edge being i and vertex 1 j; Sjinv = est[j]^-1
__host__ __device__ static inline void eg_error(const Sim3d &C, const Sim3d &Si, const Sim3d &Sjinv,
                                                double e[7])
{
    Sim3d a, b;
    so_mul(C, Si, &a);
    so_mul(a, Sjinv, &b);
    eg_log(b, e);
}

// the measurement of Optimizer.cc:1121 / :1175: Sjw * Swi
__host__ __device__ static inline void eg_measurement(const Sim3d &Siw, const Sim3d &Sjw, Sim3d *o)
{
    Sim3d Swi;
    so_inverse(Siw, &Swi);
    so_mul(Sjw, Swi, o);
}

// The host plan of one graph as the kernels read it (api_essential.hip builds it once).  Free
// vertices are numbered in elimination order (vfree[v], -1 for the fixed one).  L's block
// pattern is stored by columns: column p owns slots colptr[p] .. colptr[p + 1] - 1, rows
// ascending, the first being the diagonal block; H uses the same slots (fill blocks are 0).
struct EgPlan {
    int32_t nvert, nedge, nfree, lblocks;
    const orbg_eg_edge *edges;  // [nedge]
    const int32_t *vfree;       // [nvert]
    const int32_t *colptr;      // [nfree + 1]
    const int32_t *rowidx;      // [lblocks]
    // contributions to H's block of slot s, in edge order: edge * 4 + (0 Ji^T Ji, 1 Jj^T Jj,
    // 2 Ji^T Jj, 3 its transpose); to b's segment p: edge * 2 + (0 -Ji^T e, 1 -Jj^T e)
    const int32_t *coff, *clist, *boff, *blist;
    // slot s = (r, j) of L is updated by L(r, k) D(k) L(j, k)^T for the entries upoff[s] ..
    // upoff[s + 1] - 1 of up (x: slot of (r, k), y: slot of (j, k), z: k), k ascending
    const int32_t *upoff;
    const int4 *up;
    // row p of L left of the diagonal: entries rowoff[p] .. of row (x: slot, y: column)
    const int32_t *rowoff;
    const int2 *row;
};

// device workspace of one graph
struct EgWork {
    Sim3d *meas;          // [nedge]
    Sim3d *estinv;        // [nvert]
    Sim3d *P, *Pinv;      // [nvert][EG_NP]
    double *eo;           // [nedge][EG_EO]
    double *A, *L;        // [lblocks][49]
    double *D, *b, *y, *x;  // [nfree][7]
    double *part;         // [EG_RG]
    double *sc;           // chi2, computeScale, -, ok (int32)
};

struct Prof;
int launch_eg_measure(hipStream_t st, const EgPlan &P, const Sim3d *Scw, const Sim3d *Snc, Sim3d *meas);
int launch_eg_build(hipStream_t st, const EgPlan &P, const EgWork &W, const Sim3d *est, int fix_scale,
                    Prof *prof);
int launch_eg_errors(hipStream_t st, const EgPlan &P, const EgWork &W, const Sim3d *est, double *out,
                     Prof *prof);
int launch_eg_solve(hipStream_t st, const EgPlan &P, const EgWork &W, double lambda, int32_t *ok,
                    Prof *prof);
int launch_eg_update(hipStream_t st, const EgPlan &P, const EgWork &W, double lambda, Sim3d *est,
                     int fix_scale, double *scale_out, Prof *prof);
int launch_eg_poses(hipStream_t st, const Sim3d *est, int nvert, float *Tiw);
int launch_eg_correct_points(hipStream_t st, const Sim3d *Scw, const Sim3d *Siw, int nvert,
                             const int32_t *ref, const float *points, int n, float *out);

}  // namespace orbg
