// pnp_device.h -- the EPnP arithmetic of PnPsolver (Lepetit, Moreno-Noguer, Fua: "EPnP: an
// accurate O(n) solution to the PnP problem", IJCV 2009), shared by k_pnp_hypothesis and
// k_pnp_refine (pnp_kernels.hip).
//
// Everything is fp64 in a fixed operation order (the build has -ffp-contract=off).  The
// functions take (lane, nl): the caller's position in a group of nl cooperating lanes that
// share one PnpWork.  Work is split into independent tasks (`for (e = lane; e < tasks; e +=
// nl)`), each of which computes its outputs alone, so the results do not depend on nl; a
// host program calls the same statements with lane = 0, nl = 1.  ORBG_GROUP_SYNC() separates
// the phases: every lane of the workgroup reaches every one of them (all trip counts are fixed).
//
// Runtime-indexed arrays live in PnpWork (LDS on the device); the 3x3 problems are unrolled
// into registers.  The eigen and singular value solves are jacobi.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "jacobi.h"

namespace orbg {

#ifndef ORBG_PNP_SWEEPS12
#define ORBG_PNP_SWEEPS12 12  // parallel-ordering sweeps of the 12x12 eigen solve
#endif
#define ORBG_PNP_SWEEPS3 10   // cyclic sweeps of the 3x3 eigen / singular value solves
#define ORBG_PNP_GN_STEPS 5   // gauss_newton's iterations_number

// One point as the sums see it: the barycentric coordinates a[0..3], du = uc - u, dv = vc - v
// and d = pw - cws[0].
#define PNP_REC 9
// MtM's 78 unique entries, then K = sum a_i d_i^T (4x3) and Sa = sum a_i (4)
#define PNP_SUMS (78 + 12 + 4)

struct PnpCand {
    double qa[30], qb[6], x[5];  // the least-squares system of the beta start / a Gauss-Newton step
    double betas[4];
    double cc[4][3];             // ccs
    double R[9], t[3];
};

struct PnpWork {
    double A[144];     // MtM; its diagonal holds the eigenvalues after the sweeps
    double V[144];     // eigenvectors as columns
    double cs[12];     // (c, s) of a round's six rotations
    double nv[4][12];  // the four eigenvectors of least eigenvalue, ascending (ut rows 11, 10, 9, 8)
    double L[60], rho[6];
    double cw[4][3];   // cws
    double ku[3][3];   // row j: PCA axis j over k_j, so that alpha[1 + j] = ku[j] . (pw - cws[0])
    double K[4][3], Sa[4];
    double afirst[4];  // the first point's alphas (solve_for_sign reads pcs[2])
    double npts;
    PnpCand c[3];
};

// R = U V^T of b = U S V^T by one-sided Jacobi (b V = U S), the columns then scaled by their
// norms.  estimate_R_and_t's cvSVD.  In registers: every index is a compile-time constant.
__host__ __device__ static inline void pnp_polar3(double b[3][3], double R[9])
{
    double v[3][3];
    jacobi_onesided<3, ORBG_PNP_SWEEPS3>(b, v);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double inv = 1.0 / sqrt(jacobi_coldot<3>(b, k, k));
        b[0][k] *= inv;
        b[1][k] *= inv;
        b[2][k] *= inv;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            R[3 * i + j] = (b[i][0] * v[j][0] + b[i][1] * v[j][1]) + b[i][2] * v[j][2];
}

// choose_control_points: cws[0] = c0, cws[1 + j] = c0 + sqrt(lambda_j / n) u_j over the PCA
// axes in descending eigenvalue order, from the centred second moments cov (sum d d^T).
// One lane.
__host__ __device__ static inline void pnp_control_points(PnpWork *W, const double c0[3],
                                                          const double cov[6], double n)
{
    double a[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    double v[3][3];
    jacobi_eig_sym<3, ORBG_PNP_SWEEPS3>(a, v);
    double lam[3] = {a[0][0], a[1][1], a[2][2]};
    sort3_desc(lam, v);
    // An axis' sign is the SVD routine's choice, and with noisy points the pose depends on it
    // (the control tetrahedron is mirrored).  Here: the component of largest magnitude (the
    // first of equals) is positive.
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (largest_sign3(v, j) < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; k++) v[k][j] = -v[k][j];
        }
    W->npts = n;
#pragma unroll
    for (int k = 0; k < 3; k++) W->cw[0][k] = c0[k];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double kj = sqrt(lam[j] / n);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            W->cw[1 + j][k] = c0[k] + kj * v[k][j];
            W->ku[j][k] = v[k][j] / kj;
        }
    }
}

// compute_barycentric_coordinates + fill_M's per-point terms.  The inverse of the matrix of
// control-point offsets [k_j u_j] is [u_j / k_j]^T, as the axes are orthonormal.
__host__ __device__ static inline void pnp_point_rec(const PnpWork *W, double X, double Y, double Z,
                                                     double u, double v, double uc, double vc,
                                                     double *rec)
{
    const double d0 = X - W->cw[0][0], d1 = Y - W->cw[0][1], d2 = Z - W->cw[0][2];
    const double a1 = (W->ku[0][0] * d0 + W->ku[0][1] * d1) + W->ku[0][2] * d2;
    const double a2 = (W->ku[1][0] * d0 + W->ku[1][1] * d1) + W->ku[1][2] * d2;
    const double a3 = (W->ku[2][0] * d0 + W->ku[2][1] * d1) + W->ku[2][2] * d2;
    rec[0] = ((1.0 - a1) - a2) - a3;
    rec[1] = a1, rec[2] = a2, rec[3] = a3;
    rec[4] = uc - u, rec[5] = vc - v;
    rec[6] = d0, rec[7] = d1, rec[8] = d2;
}

// One point's term of sum e: M^T M [3j + p][3k + q] += a_j a_k w_pq with the two rows of
// fill_M r1 = (fu, 0, du), r2 = (0, fv, dv) and w = r1 r1^T + r2 r2^T; then K and Sa.
__host__ __device__ static inline double pnp_sum_term(int e, const double *rec, double fu, double fv)
{
    if (e >= 78 + 12) return rec[e - 90];
    if (e >= 78) {
        const int m = (e - 78) / 3, k = (e - 78) - 3 * m;
        return rec[m] * rec[6 + k];
    }
    int r, c;
    sym_index<12>(e, &r, &c);
    const int j = r / 3, p = r - 3 * j, k = c / 3, q = c - 3 * k;
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    const double du = rec[4], dv = rec[5];
    double w;
    if (hi == 2)
        w = lo == 0 ? fu * du : (lo == 1 ? fv * dv : du * du + dv * dv);
    else
        w = lo != hi ? 0.0 : (lo == 0 ? fu * fu : fv * fv);
    return (rec[j] * rec[k]) * w;
}

__host__ __device__ static inline void pnp_sum_store(PnpWork *W, int e, double s)
{
    if (e >= 78 + 12) {
        W->Sa[e - 90] = s;
    } else if (e >= 78) {
        (&W->K[0][0])[e - 78] = s;
    } else {
        int r, c;
        sym_index<12>(e, &r, &c);
        W->A[12 * r + c] = s;
        W->A[12 * c + r] = s;
    }
}

// Least squares of the 6 x nc system a (row-major, stride nc) x = b by Householder
// reflections, in place.  A zero column divides by zero: the NaN marks the hypothesis.
__host__ __device__ static inline void pnp_lstsq6(double *a, double *b, int nc, double *x)
{
    for (int k = 0; k < nc; k++) {
        double s2 = 0.0;
        for (int i = k; i < 6; i++) s2 += a[i * nc + k] * a[i * nc + k];
        const double akk = a[k * nc + k];
        const double alpha = akk < 0.0 ? sqrt(s2) : -sqrt(s2);
        const double v0 = akk - alpha;            // v = (v0, a[k+1..][k])
        const double vv = (s2 - akk * akk) + v0 * v0;
        for (int j = k + 1; j < nc; j++) {
            double dot = v0 * a[k * nc + j];
            for (int i = k + 1; i < 6; i++) dot += a[i * nc + k] * a[i * nc + j];
            const double tau = 2.0 * dot / vv;
            a[k * nc + j] -= tau * v0;
            for (int i = k + 1; i < 6; i++) a[i * nc + j] -= tau * a[i * nc + k];
        }
        double dot = v0 * b[k];
        for (int i = k + 1; i < 6; i++) dot += a[i * nc + k] * b[i];
        const double tau = 2.0 * dot / vv;
        b[k] -= tau * v0;
        for (int i = k + 1; i < 6; i++) b[i] -= tau * a[i * nc + k];
        a[k * nc + k] = alpha;
    }
    for (int i = nc - 1; i >= 0; i--) {
        double s = b[i];
        for (int j = i + 1; j < nc; j++) s -= a[i * nc + j] * x[j];
        x[i] = s / a[i * nc + i];
    }
}

// compute_L_6x10 and compute_rho: one entry per task
__host__ __device__ static inline void pnp_L_rho(PnpWork *W, int lane, int nl)
{
    for (int e = lane; e < 66; e += nl) {
        const int i = e < 60 ? e / 10 : e - 60, col = e < 60 ? e - 10 * i : 0;
        // the i-th pair (a, b) of 0 <= a < b < 4: 01 02 03 12 13 23
        const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
        if (e >= 60) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) {
                const double d = W->cw[a][k] - W->cw[b][k];
                s += d * d;
            }
            W->rho[i] = s;
            continue;
        }
        // column -> (m, n) of betas10 = [B11 B12 B22 B13 B23 B33 B14 B24 B34 B44]
        int n = 0, rem = col;
        while (rem > n) {
            rem -= n + 1;
            n++;
        }
        const int m = rem;
        double s = 0.0;
        for (int k = 0; k < 3; k++)
            s += (W->nv[m][3 * a + k] - W->nv[m][3 * b + k]) * (W->nv[n][3 * a + k] - W->nv[n][3 * b + k]);
        W->L[e] = m == n ? s : 2.0 * s;
    }
}

// One of the three candidates: find_betas_approx_{1,2,3}, gauss_newton, compute_ccs,
// solve_for_sign and estimate_R_and_t.  One lane per candidate.
__host__ __device__ static inline void pnp_candidate(PnpWork *W, int which)
{
    PnpCand *C = &W->c[which];
    const double *L = W->L;
    // the columns of L_6x10 the linearised start keeps
    const int nc = which == 0 ? 4 : (which == 1 ? 3 : 5);
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < nc; j++) {
            const int col = which == 0 ? (j == 0 ? 0 : (j == 1 ? 1 : (j == 2 ? 3 : 6))) : j;
            C->qa[i * nc + j] = L[10 * i + col];
        }
        C->qb[i] = W->rho[i];
    }
    pnp_lstsq6(C->qa, C->qb, nc, C->x);
    double *be = C->betas;
    const double *x = C->x;
    if (which == 0) {  // B11 B12 B13 B14
        const double sg = x[0] < 0.0 ? -1.0 : 1.0;
        be[0] = sqrt(sg * x[0]);
        be[1] = sg * x[1] / be[0];
        be[2] = sg * x[2] / be[0];
        be[3] = sg * x[3] / be[0];
    } else {  // B11 B12 B22 (B13 B23)
        if (x[0] < 0.0) {
            be[0] = sqrt(-x[0]);
            be[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
        } else {
            be[0] = sqrt(x[0]);
            be[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
        }
        if (x[1] < 0.0) be[0] = -be[0];
        be[2] = which == 2 ? x[3] / be[0] : 0.0;
        be[3] = 0.0;
    }
    for (int step = 0; step < ORBG_PNP_GN_STEPS; step++) {
        const double b0 = be[0], b1 = be[1], b2 = be[2], b3 = be[3];
        for (int i = 0; i < 6; i++) {
            const double *l = L + 10 * i;
            double *a = C->qa + 4 * i;
            a[0] = ((2.0 * l[0] * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3;
            a[1] = ((l[1] * b0 + 2.0 * l[2] * b1) + l[4] * b2) + l[7] * b3;
            a[2] = ((l[3] * b0 + l[4] * b1) + 2.0 * l[5] * b2) + l[8] * b3;
            a[3] = ((l[6] * b0 + l[7] * b1) + l[8] * b2) + 2.0 * l[9] * b3;
            double q = l[0] * b0 * b0;
            q += l[1] * b0 * b1;
            q += l[2] * b1 * b1;
            q += l[3] * b0 * b2;
            q += l[4] * b1 * b2;
            q += l[5] * b2 * b2;
            q += l[6] * b0 * b3;
            q += l[7] * b1 * b3;
            q += l[8] * b2 * b3;
            q += l[9] * b3 * b3;
            C->qb[i] = W->rho[i] - q;
        }
        pnp_lstsq6(C->qa, C->qb, 4, C->x);
        for (int i = 0; i < 4; i++) be[i] += C->x[i];
    }
    // compute_ccs, and the sign that puts the first point in front of the camera
    double z0 = 0.0;
    for (int j = 0; j < 4; j++) {
        for (int k = 0; k < 3; k++) {
            double s = 0.0;
            for (int i = 0; i < 4; i++) s += be[i] * W->nv[i][3 * j + k];
            C->cc[j][k] = s;
        }
        z0 += W->afirst[j] * C->cc[j][2];
    }
    if (z0 < 0.0)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) C->cc[j][k] = -C->cc[j][k];
    // estimate_R_and_t.  pcs = alphas * ccs is linear, so its centroid and its correlation
    // with pw - pw0 follow from Sa and K; pw0 is cws[0] (the same sum).
    double pc0[3], b[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pc0[j] = (((W->Sa[0] * C->cc[0][j] + W->Sa[1] * C->cc[1][j]) + W->Sa[2] * C->cc[2][j]) +
                  W->Sa[3] * C->cc[3][j]) / W->npts;
#pragma unroll
        for (int k = 0; k < 3; k++)
            b[j][k] = ((C->cc[0][j] * W->K[0][k] + C->cc[1][j] * W->K[1][k]) + C->cc[2][j] * W->K[2][k]) +
                      C->cc[3][j] * W->K[3][k];
    }
    double R[9];
    pnp_polar3(b, R);
    const double det = ((R[0] * R[4] * R[8] + R[1] * R[5] * R[6]) + R[2] * R[3] * R[7]) -
                       ((R[2] * R[4] * R[6] + R[1] * R[3] * R[8]) + R[0] * R[5] * R[7]);
    if (det < 0.0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) C->R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        C->t[i] = pc0[i] - ((R[3 * i] * W->cw[0][0] + R[3 * i + 1] * W->cw[0][1]) + R[3 * i + 2] * W->cw[0][2]);
}

// compute_pose after M^T M: W->A, K, Sa, afirst, cw and npts are set.  Leaves the three
// candidate poses in W->c[].R / .t.  Every lane of the workgroup calls it.
__host__ __device__ static inline void pnp_tail(PnpWork *W, int lane, int nl)
{
    // the 12x12 eigen solve: a round's six rotations and 72 updates split over the lanes
    jacobi_eig_lanes<1, 12, ORBG_PNP_SWEEPS12>(W->A, W->V, W->cs, lane, nl);
    // the four smallest eigenvalues, ascending; ties go to the lower index (every lane)
    int idx[4];
    unsigned used = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int best = -1;
        double bv = 0.0;
        for (int k = 0; k < 12; k++) {
            if ((used >> k) & 1u) continue;
            const double d = W->A[13 * k];
            if (best < 0 || d < bv) best = k, bv = d;
        }
        idx[i] = best;
        used |= 1u << best;
    }
    for (int e = lane; e < 48; e += nl) {
        const int i = e / 12, k = e - 12 * i;
        const int col = i == 0 ? idx[0] : (i == 1 ? idx[1] : (i == 2 ? idx[2] : idx[3]));
        W->nv[i][k] = W->V[12 * k + col];
    }
    ORBG_GROUP_SYNC();
    pnp_L_rho(W, lane, nl);
    ORBG_GROUP_SYNC();
    for (int c = lane; c < 3; c += nl) pnp_candidate(W, c);
    ORBG_GROUP_SYNC();
}

// reprojection_error's term for one point
__host__ __device__ static inline double pnp_reproj(const double *R, const double *t, double X,
                                                    double Y, double Z, double u, double v, double fu,
                                                    double fv, double uc, double vc)
{
    const double Xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
    const double Yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
    const double iz = 1.0 / (((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]);
    const double du = u - (uc + fu * Xc * iz), dv = v - (vc + fv * Yc * iz);
    return sqrt(du * du + dv * dv);
}

// compute_pose's choice among the candidates' mean reprojection errors: `<`, so a NaN never
// wins and candidate 1 stands when all are NaN.  Returns 0, 1 or 2.
__host__ __device__ static inline int pnp_choose(double e1, double e2, double e3)
{
    int n = 0;
    double e = e1;
    if (e2 < e) n = 1, e = e2;
    if (e3 < e) n = 2;
    return n;
}

__host__ __device__ static inline bool pnp_finite(const double *R, const double *t)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && fabs(R[i]) <= 1.0e300;
#pragma unroll
    for (int i = 0; i < 3; i++) ok = ok && fabs(t[i]) <= 1.0e300;
    return ok;  // false for NaN too
}

// PnPsolver::CheckInliers (:308-339) for one correspondence, with the reference's types: Xc,
// Yc the double sums rounded to float, invZc = (float)(1 / double sum), ue / ve in double,
// the distances and error2 in float; strict <, NaN fails.
__host__ __device__ static inline bool pnp_inlier(const double *R, const double *t, float X, float Y,
                                                  float Z, float u, float v, float max_error,
                                                  double fu, double fv, double uc, double vc)
{
    const float Xc = (float)(((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]);
    const float Yc = (float)(((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]);
    const float invZc = (float)(1 / (((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float distX = (float)(u - ue);
    const float distY = (float)(v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}

}  // namespace orbg
