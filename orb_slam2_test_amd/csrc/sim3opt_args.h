// sim3opt_args.h -- launch arguments and the arithmetic of Optimizer::OptimizeSim3
// (sim3opt_kernels.hip), shared with the host entry points (api_solvers.hip) and with the
// one-core host program of tools/sim3opt_bench.py (sim3opt_host.hip).
//
// Everything g2o evaluates for the one free VertexSim3Expmap is here as __host__ __device__
// functions in fp64 with a fixed operation order (the build has -ffp-contract=off), so a host
// program runs the very same statements: g2o::Sim3 (exp, product, inverse, map;
// Thirdparty/g2o/g2o/types/sim3.h), the two projection edges (types_seven_dof_expmap.h:
// 130-171), Huber (robust_kernel_impl.cpp:65-91) and the numeric Jacobian of
// BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205).  The quaternion formulas,
// Eigen's pivoted LDLT and the Levenberg-Marquardt step control are g2o_math.h's.
// Quaternions are (x, y, z, w) and, as in g2o::Sim3, never re-normalised.
#pragma once

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <stdint.h>

#include "../../include/orbg.h"
#include "orbg_device.h"
#include "g2o_math.h"

#pragma clang fp contract(off)

namespace orbg {

#define ORBG_SIM3OPT_MAX_N 8192  // correspondences per candidate (as Sim3Solver's limit)
#define SO_NV 36                 // robust chi2, 28 lower-triangle H entries, 7 b entries
#define SO_NP 14                 // perturbed estimates of one linearisation: +-delta per column

struct Sim3d {
    double q[4], t[3], s;
};

struct Sim3OptArgs {
    const orbg_sim3opt_problem *problems;  // [npairs]
    const orbg_sim3opt_corr *corrs;        // [npairs][cap]
    const orbg_sim3_hyp *init;             // [npairs]
    int32_t npairs, cap, n1cap;
    orbg_sim3opt_result *results;          // [npairs]
    uint8_t *keep;                         // [npairs][n1cap]
};

// Correspondences the candidate really has: a count outside [0, cap], or a th2 that is not
// finite and positive, runs nothing (the record is that of n = 0).
__host__ __device__ static inline int sim3opt_n(const orbg_sim3opt_problem &P, int cap)
{
    if (!(P.th2 > 0.0f) || !(P.th2 <= FLT_MAX)) return 0;
    return (P.n < 0 || P.n > cap) ? 0 : P.n;
}

// ---- exp pinned to one polynomial (host and device agree bit for bit; sin / cos are
// orbg_device.h's pinned_sincos) ----
// exp: x = k ln2 + r, |r| <= ln2 / 2, Taylor to r^13 / 13! (remainder below 1e-17 relative),
// scaled by 2^k.  exp(0) is exactly 1.  |x| past 700 is clamped (a scale step never is).
__host__ __device__ static inline double so_exp(double x)
{
    if (!(x == x)) return x;
    x = x > 700.0 ? 700.0 : (x < -700.0 ? -700.0 : x);
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double kd = rint(x * 1.44269504088896338700e+00);
    const double r = (x - kd * ln2_hi) - kd * ln2_lo;
    double p = 1.0 / 6227020800.0;
    const double c[12] = {1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0,
                          1.0 / 40320.0,     1.0 / 5040.0,     1.0 / 720.0,     1.0 / 120.0,
                          1.0 / 24.0,        1.0 / 6.0,        0.5,             1.0};
    for (int i = 0; i < 12; i++) p = c[i] + r * p;
    return ldexp(1.0 + r * p, (int)kd);
}

// ---- g2o::Sim3 ----
// g2o::Sim3(Converter::toMatrix3d(R12), toVector3d(t12), s12): the float hypothesis widened
__host__ __device__ static inline void so_init(const orbg_sim3_hyp &h, Sim3d *S)
{
    double R[3][3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = h.R[3 * i + j];
        S->t[i] = h.t[i];
    }
    q_from_rot(R, S->q);
    S->s = h.s;
}

// Sim3(const Vector7d &update), sim3.h:70-142: (omega, upsilon, sigma), four branches
__host__ __device__ static inline void so_exp_sim3(const double u[7], Sim3d *S)
{
    const double w[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double O[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    const double s = so_exp(sigma);
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    const double eps = 0.00001;
    double A, B, C;
    double sn = 0, cs = 1;
    if (!(theta < eps)) pinned_sincos(theta, &sn, &cs);
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    if (theta < eps) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                R[i][j] = ((i == j ? 1.0 : 0.0) + ra * O[i][j]) + rb * O2[i][j];
    }
    q_from_rot(R, S->q);
    for (int i = 0; i < 3; i++) {
        double W[3];
        for (int j = 0; j < 3; j++) W[j] = (A * O[i][j] + B * O2[i][j]) + (i == j ? C : 0.0);
        S->t[i] = W[0] * ups[0] + W[1] * ups[1] + W[2] * ups[2];
    }
    S->s = s;
}

// Sim3::operator*: r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
__host__ __device__ static inline void so_mul(const Sim3d &a, const Sim3d &b, Sim3d *o)
{
    double rt[3];
    q_mul(a.q, b.q, o->q);
    q_rotate(a.q, b.t, rt);
    for (int i = 0; i < 3; i++) o->t[i] = a.s * rt[i] + a.t[i];
    o->s = a.s * b.s;
}

// Sim3::inverse: (r.conjugate(), r.conjugate() * ((-1 / s) * t), 1 / s)
__host__ __device__ static inline void so_inverse(const Sim3d &a, Sim3d *o)
{
    const double k = -1. / a.s;
    const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
    o->q[0] = -a.q[0];
    o->q[1] = -a.q[1];
    o->q[2] = -a.q[2];
    o->q[3] = a.q[3];
    q_rotate(o->q, v, o->t);
    o->s = 1. / a.s;
}

// Sim3::map: s * (r * xyz) + t
__host__ __device__ static inline void so_map(const Sim3d &a, const double x[3], double o[3])
{
    double r[3];
    q_rotate(a.q, x, r);
    for (int i = 0; i < 3; i++) o[i] = a.s * r[i] + a.t[i];
}

// VertexSim3Expmap::oplusImpl: Sim3(update) * estimate, update[6] = 0 under _fix_scale
__host__ __device__ static inline void so_oplus(const Sim3d &est, const double upd[7], bool fix_scale,
                                                Sim3d *o)
{
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = upd[i];
    if (fix_scale) u[6] = 0;
    Sim3d d;
    so_exp_sim3(u, &d);
    so_mul(d, est, o);
}

// The 14 estimates of one numeric linearisation (base_binary_edge.hpp:176-197): k = 2 d is
// column d's oplus(+delta), k = 2 d + 1 its oplus(-delta); with their inverses, which
// EdgeInverseSim3ProjectXYZ::computeError takes of whatever the estimate is.
#define SO_DELTA 1e-9
__host__ __device__ static inline void so_perturbed(const Sim3d &est, int k, bool fix_scale,
                                                    Sim3d *P, Sim3d *Pinv)
{
    double u[7] = {0, 0, 0, 0, 0, 0, 0};
    u[k >> 1] = (k & 1) ? -SO_DELTA : SO_DELTA;
    so_oplus(est, u, fix_scale, P);
    so_inverse(*P, Pinv);
}

// ---- the edges ----
// One correspondence as the optimiser holds it: the two fixed VertexSBAPointXYZ (float
// camera-frame points, sim3_transform's order, widened), the measurements and informations.
struct SoPair {
    double P1c[3], P2c[3], obs1[2], obs2[2], info1, info2;
};

__host__ __device__ static inline void so_pair(const orbg_sim3opt_problem &P, const orbg_sim3opt_corr &c,
                                               SoPair *e)
{
    for (int r = 0; r < 3; r++) {
        const float a = ((P.T1w[4 * r] * c.Xw1[0] + P.T1w[4 * r + 1] * c.Xw1[1]) + P.T1w[4 * r + 2] * c.Xw1[2]) + P.T1w[4 * r + 3];
        const float b = ((P.T2w[4 * r] * c.Xw2[0] + P.T2w[4 * r + 1] * c.Xw2[1]) + P.T2w[4 * r + 2] * c.Xw2[2]) + P.T2w[4 * r + 3];
        e->P1c[r] = a;
        e->P2c[r] = b;
    }
    e->obs1[0] = c.obs1[0];
    e->obs1[1] = c.obs1[1];
    e->obs2[0] = c.obs2[0];
    e->obs2[1] = c.obs2[1];
    e->info1 = c.inv_sigma2_1;
    e->info2 = c.inv_sigma2_2;
}

// EdgeSim3ProjectXYZ::computeError: obs1 - cam_map1(project(S.map(P2c)))
__host__ __device__ static inline void so_err12(const Sim3d &S, const orbg_sim3opt_problem &P,
                                                const SoPair &e, double err[2])
{
    double x[3];
    so_map(S, e.P2c, x);
    err[0] = e.obs1[0] - ((x[0] / x[2]) * (double)P.fx1 + (double)P.cx1);
    err[1] = e.obs1[1] - ((x[1] / x[2]) * (double)P.fy1 + (double)P.cy1);
}

// EdgeInverseSim3ProjectXYZ::computeError: obs2 - cam_map2(project(S.inverse().map(P1c)))
__host__ __device__ static inline void so_err21(const Sim3d &Sinv, const orbg_sim3opt_problem &P,
                                                const SoPair &e, double err[2])
{
    double x[3];
    so_map(Sinv, e.P1c, x);
    err[0] = e.obs2[0] - ((x[0] / x[2]) * (double)P.fx2 + (double)P.cx2);
    err[1] = e.obs2[1] - ((x[1] / x[2]) * (double)P.fy2 + (double)P.cy2);
}

// chi2(): _error.dot(information() * _error), information = info * I
__host__ __device__ static inline double so_chi2(const double err[2], double info)
{
    return err[0] * (info * err[0]) + err[1] * (info * err[1]);
}

// const float deltaHuber = sqrt(th2); RobustKernelHuber keeps delta^2 in a float
__host__ __device__ static inline double so_huber_delta(float th2) { return (double)(float)sqrt((double)th2); }

__host__ __device__ static inline void so_huber(double chi2, double delta, double *rho0, double *rho1)
{
    const float dsqr = (float)(delta * delta);
    *rho0 = chi2;
    *rho1 = 1.0;
    if (!(chi2 <= dsqr)) {
        const double sq = sqrt(chi2);
        *rho1 = delta / sq;
        *rho0 = 2 * sq * delta - dsqr;
    }
}

// the drop test of Optimizer.cc:1529 / :1563 at the estimate S: a NaN is not greater
__host__ __device__ static inline bool so_is_bad(const Sim3d &S, const Sim3d &Sinv,
                                                 const orbg_sim3opt_problem &P, const SoPair &e)
{
    double e12[2], e21[2];
    so_err12(S, P, e, e12);
    so_err21(Sinv, P, e, e21);
    const double th2 = (double)P.th2;
    return so_chi2(e12, e.info1) > th2 || so_chi2(e21, e.info2) > th2;
}

// one pair's share of activeRobustChi2 at S (the error pass of an LM trial)
__host__ __device__ static inline double so_pair_chi(const Sim3d &S, const Sim3d &Sinv,
                                                     const orbg_sim3opt_problem &P, const SoPair &e,
                                                     double delta)
{
    double e12[2], e21[2], r0a, r0b, r1;
    so_err12(S, P, e, e12);
    so_err21(Sinv, P, e, e21);
    so_huber(so_chi2(e12, e.info1), delta, &r0a, &r1);
    so_huber(so_chi2(e21, e.info2), delta, &r0b, &r1);
    return r0a + r0b;
}

// one edge into the sums: p[0] += rho, H += J^T (rho' Omega) J, b += J^T (-Omega e rho')
__host__ __device__ static inline void so_add_edge(const double err[2], const double J[2][7],
                                                   double info, double delta, double p[SO_NV])
{
    double rho0, rho1;
    so_huber(so_chi2(err, info), delta, &rho0, &rho1);
    p[0] += rho0;
    const double w = rho1 * info;
    const double wr[2] = {-info * err[0] * rho1, -info * err[1] * rho1};
    int hi = 1;
#pragma unroll
    for (int r = 0; r < 7; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) p[hi++] += J[0][r] * w * J[0][c] + J[1][r] * w * J[1][c];
#pragma unroll
    for (int r = 0; r < 7; r++) p[29 + r] += J[0][r] * wr[0] + J[1][r] * wr[1];
}

// computeError + linearizeOplus + constructQuadraticForm of one pair's two edges at S, given
// the 14 perturbed estimates Pp / Pi of S (so_perturbed)
__host__ __device__ static inline void so_add_pair(const Sim3d &S, const Sim3d &Sinv, const Sim3d *Pp,
                                                   const Sim3d *Pi, const orbg_sim3opt_problem &P,
                                                   const SoPair &e, double delta, double p[SO_NV])
{
    const double scalar = 1.0 / (2 * SO_DELTA);
    double e12[2], e21[2], J12[2][7], J21[2][7];
    so_err12(S, P, e, e12);
    so_err21(Sinv, P, e, e21);
#pragma unroll
    for (int d = 0; d < 7; d++) {
        double a[2], b[2];
        so_err12(Pp[2 * d], P, e, a);
        so_err12(Pp[2 * d + 1], P, e, b);
        J12[0][d] = scalar * (a[0] - b[0]);
        J12[1][d] = scalar * (a[1] - b[1]);
        so_err21(Pi[2 * d], P, e, a);
        so_err21(Pi[2 * d + 1], P, e, b);
        J21[0][d] = scalar * (a[0] - b[0]);
        J21[1][d] = scalar * (a[1] - b[1]);
    }
    so_add_edge(e12, J12, e.info1, delta, p);
    so_add_edge(e21, J21, e.info2, delta, p);
}

// ---- one LM trial (g2o_math.h has the step control) ----
// setLambda, the LDLT solve, oplus into *trial, restoreDiagonal; returns the solver's ok
// (Hd: 49 doubles of workspace for the damped copy; the kernel passes LDS)
__host__ __device__ static inline bool so_lm_trial(const LmState *L, const double H[49], const double b[7],
                                                   const Sim3d &est, bool fix_scale, double x[7],
                                                   Sim3d *trial, double (*Hd)[7])
{
    for (int r = 0; r < 7; r++)
        for (int c = 0; c < 7; c++) Hd[r][c] = H[r * 7 + c];
    for (int j = 0; j < 7; j++) Hd[j][j] += L->lambda;
    const bool ok = ldlt_solve<7>(Hd, b, x);
    so_oplus(est, x, fix_scale, trial);
    return ok;
}

// the result record from the estimate: R / tf / sf = toRotationMatrix, t, s rounded once
__host__ __device__ static inline void so_result(const Sim3d &S, int nin, int nbad, int ncorr, int it0,
                                                 int it1, orbg_sim3opt_result *r)
{
    double R[3][3];
    q_to_rot(S.q, R);
    for (int i = 0; i < 4; i++) r->q[i] = S.q[i];
    for (int i = 0; i < 3; i++) {
        r->t[i] = S.t[i];
        r->tf[i] = (float)S.t[i];
        for (int j = 0; j < 3; j++) r->R[3 * i + j] = (float)R[i][j];
    }
    r->s = S.s;
    r->sf = (float)S.s;
    r->ninliers = nin;
    r->nbad = nbad;
    r->ncorr = ncorr;
    r->iterations[0] = it0;
    r->iterations[1] = it1;
}

struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_sim3opt(hipStream_t st, const Sim3OptArgs &A, Prof *prof);

}  // namespace orbg
