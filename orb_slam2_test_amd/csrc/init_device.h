// init_device.h -- the arithmetic of Initializer (src/Initializer.cc), shared by the kernels
// of init_kernels.hip and the one-core host program init_host.hip.
//
// fp64 linear algebra in a fixed operation order (the build has -ffp-contract=off), float
// where the reference holds CV_32F.  Functions that take (lane, nl) split independent tasks
// over a group of nl cooperating lanes that share one InitWork (`for (e = lane; e < tasks; e
// += nl)`), so the results do not depend on nl; the host program calls the same statements
// with lane = 0, nl = 1.  ORBG_GROUP_SYNC() separates the phases: every lane of the workgroup
// reaches every one of them (all trip counts are fixed).  The eigen and singular value solves
// are jacobi.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "init_args.h"
#include "jacobi.h"

namespace orbg {

#define ORBG_INIT_SWEEPS9 12  // round-robin sweeps of the 9x9 eigen solves
#define ORBG_INIT_SWEEPS3 12  // cyclic sweeps of the one-sided 3x3 Jacobi
#define ORBG_INIT_SWEEPS4 10  // cyclic sweeps of Triangulate's one-sided 4x4 Jacobi

// One (pair, iteration): both models side by side (index 0: H, 1: F).
struct InitWork {
    float pn[8][4];     // the set's normalised (u1, v1, u2, v2)
    float rows[24][9];  // A of ComputeH21 (rows 0..15), A of ComputeF21 (rows 16..23)
    double A[2][81];    // A^T A; the diagonal holds the eigenvalues after the sweeps
    double V[2][81];    // eigenvectors as columns
    double cs[2][8];    // (c, s) of a round's four rotations
    int idx[8];
    int ok;
};

__host__ __device__ static inline bool init_finite9(const float *m)
{
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && isfinite(m[k]);
    return ok;
}

// ---- ComputeH21 / ComputeF21 ----

// vPn1i[j], vPn2i[j]: (x - meanX) * sX in float (:1007-1024)
__host__ __device__ static inline void init_normalized(const float4 r, const InitNorm n1,
                                                       const InitNorm n2, float *pn)
{
    pn[0] = (r.x - n1.mx) * n1.sx;
    pn[1] = (r.y - n1.my) * n1.sy;
    pn[2] = (r.z - n2.mx) * n2.sx;
    pn[3] = (r.w - n2.my) * n2.sy;
}

// the rows of point j: the reference's CV_32F entries (:341-359, :390-398)
__host__ __device__ static inline void init_rows(InitWork *W, int j)
{
    const float u1 = W->pn[j][0], v1 = W->pn[j][1], u2 = W->pn[j][2], v2 = W->pn[j][3];
    float *a = W->rows[2 * j], *b = W->rows[2 * j + 1], *f = W->rows[16 + j];
    a[0] = 0.f, a[1] = 0.f, a[2] = 0.f, a[3] = -u1, a[4] = -v1, a[5] = -1.f;
    a[6] = v2 * u1, a[7] = v2 * v1, a[8] = v2;
    b[0] = u1, b[1] = v1, b[2] = 1.f, b[3] = 0.f, b[4] = 0.f, b[5] = 0.f;
    b[6] = -u2 * u1, b[7] = -u2 * v1, b[8] = -u2;
    f[0] = u2 * u1, f[1] = u2 * v1, f[2] = u2, f[3] = v2 * u1, f[4] = v2 * v1, f[5] = v2;
    f[6] = u1, f[7] = v1, f[8] = 1.f;
}

// A^T A of both models: 2 x 45 sums over the rows in index order
__host__ __device__ static inline void init_ata(InitWork *W, int lane, int nl)
{
    for (int e = lane; e < 90; e += nl) {
        const int m = e / 45;
        int r, c;
        sym_index<9>(e - 45 * m, &r, &c);
        const int k0 = m ? 16 : 0, k1 = m ? 24 : 16;
        double s = 0.0;
        for (int k = k0; k < k1; k++) s += (double)W->rows[k][r] * (double)W->rows[k][c];
        W->A[m][9 * r + c] = s;
        W->A[m][9 * c + r] = s;
    }
}

// vt.row(8): the eigenvector of least eigenvalue (the first of equals)
__host__ __device__ static inline void init_null_vector(const InitWork *W, int m, double h[9])
{
    int j = 0;
    for (int k = 1; k < 9; k++)
        if (W->A[m][10 * k] < W->A[m][10 * j]) j = k;
    for (int k = 0; k < 9; k++) h[k] = W->V[m][9 * k + j];
}

// One-sided Jacobi, b <- b V, with the columns in descending norm order (stable)
__host__ __device__ static inline void init_jacobi3_sorted(double b[3][3], double v[3][3], double n2[3])
{
    jacobi_onesided<3, ORBG_INIT_SWEEPS3>(b, v);
    for (int k = 0; k < 3; k++) n2[k] = jacobi_coldot<3>(b, k, k);
    sort3_desc(n2, b, v);
}

// m = T2 side * x * T1 for the 3x3 x (row-major), T1 = [s1x 0 t1x; 0 s1y t1y; 0 0 1]
__host__ __device__ static inline void init_times_T1(const double x[9], const InitNorm n1, double m[9])
{
    const double sx = n1.sx, sy = n1.sy;
    const double tx = -n1.mx * n1.sx, ty = -n1.my * n1.sy;  // float products, as T holds them
    for (int r = 0; r < 3; r++) {
        m[3 * r] = x[3 * r] * sx;
        m[3 * r + 1] = x[3 * r + 1] * sy;
        m[3 * r + 2] = (x[3 * r] * tx + x[3 * r + 1] * ty) + x[3 * r + 2];
    }
}

// H21i = T2inv Hn T1 rounded to float once, H12i = the inverse of that float matrix rounded
// once.  false: not finite or singular.
__host__ __device__ static inline bool init_h_tail(const double h[9], const InitNorm n1,
                                                   const InitNorm n2, float *H21, float *H12)
{
    double m[9], g[9], inv[9];
    init_times_T1(h, n1, m);
    const double tx = -n2.mx * n2.sx, ty = -n2.my * n2.sy;
    const double ix = 1.0 / (double)n2.sx, iy = 1.0 / (double)n2.sy;
    const double ox = -tx * ix, oy = -ty * iy;  // T2inv = [ix 0 ox; 0 iy oy; 0 0 1]
    for (int c = 0; c < 3; c++) {
        g[c] = m[c] * ix + m[6 + c] * ox;
        g[3 + c] = m[3 + c] * iy + m[6 + c] * oy;
        g[6 + c] = m[6 + c];
    }
    // H12i = H21i.inv() is taken of the CV_32F matrix
    for (int k = 0; k < 9; k++) H21[k] = (float)g[k], g[k] = (double)H21[k];
    const double c00 = g[4] * g[8] - g[5] * g[7], c01 = g[5] * g[6] - g[3] * g[8];
    const double c02 = g[3] * g[7] - g[4] * g[6];
    const double det = (g[0] * c00 + g[1] * c01) + g[2] * c02;
    const double id = 1.0 / det;
    inv[0] = c00 * id, inv[1] = (g[2] * g[7] - g[1] * g[8]) * id, inv[2] = (g[1] * g[5] - g[2] * g[4]) * id;
    inv[3] = c01 * id, inv[4] = (g[0] * g[8] - g[2] * g[6]) * id, inv[5] = (g[2] * g[3] - g[0] * g[5]) * id;
    inv[6] = c02 * id, inv[7] = (g[1] * g[6] - g[0] * g[7]) * id, inv[8] = (g[0] * g[4] - g[1] * g[3]) * id;
    for (int k = 0; k < 9; k++) H12[k] = (float)inv[k];
    return det != 0.0 && init_finite9(H21) && init_finite9(H12);
}

// Fn = u diag(w0, w1, 0) vt of Fpre = the null vector; F21i = T2^T Fn T1, rounded once.
__host__ __device__ static inline bool init_f_tail(const double h[9], const InitNorm n1,
                                                   const InitNorm n2, float *F21)
{
    double b[3][3], v[3][3], n2c[3], fn[9], m[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) b[i][j] = h[3 * i + j];
    init_jacobi3_sorted(b, v, n2c);
    // Fpre = sum_k b_k v_k^T; the column of least norm is dropped
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) fn[3 * i + j] = b[i][0] * v[j][0] + b[i][1] * v[j][1];
    init_times_T1(fn, n1, m);
    const double sx = n2.sx, sy = n2.sy;
    const double tx = -n2.mx * n2.sx, ty = -n2.my * n2.sy;
    for (int c = 0; c < 3; c++) {
        F21[c] = (float)(sx * m[c]);
        F21[3 + c] = (float)(sy * m[3 + c]);
        F21[6 + c] = (float)((tx * m[c] + ty * m[3 + c]) + m[6 + c]);
    }
    return init_finite9(F21);
}

// One (pair, iteration) from its gathered set: W->pn, W->idx filled for j < 8, W->ok = the
// set is usable.  With `store`, writes H21 / H12 / F21 [9] (zero where the model cannot score);
// a group without a row of its own goes through the phases and stores nothing.
__host__ __device__ static inline void init_hypothesis(InitWork *W, const InitNorm n1, const InitNorm n2,
                                                       bool store, float *H21, float *H12, float *F21,
                                                       int lane, int nl)
{
    for (int j = lane; j < 8; j += nl) init_rows(W, j);
    ORBG_GROUP_SYNC();
    init_ata(W, lane, nl);
    ORBG_GROUP_SYNC();
    // both 9x9 eigen solves at once: a round's 8 rotations and 72 updates split over the lanes
    jacobi_eig_lanes<2, 9, ORBG_INIT_SWEEPS9>(W->A[0], W->V[0], W->cs[0], lane, nl);
    for (int m = lane; m < 2; m += nl) {
        double h[9];
        init_null_vector(W, m, h);
        float a[9], b[9];
        if (m == 0) {
            const bool ok = init_h_tail(h, n1, n2, a, b) && W->ok;
            if (store)
                for (int k = 0; k < 9; k++) H21[k] = ok ? a[k] : 0.f, H12[k] = ok ? b[k] : 0.f;
        } else {
            const bool ok = init_f_tail(h, n1, n2, a) && W->ok;
            if (store)
                for (int k = 0; k < 9; k++) F21[k] = ok ? a[k] : 0.f;
        }
    }
}

__host__ __device__ static inline bool init_is_zero9(const float *m)
{
    bool z = true;
    for (int k = 0; k < 9; k++) z = z && m[k] == 0.f;
    return z;
}

// ---- CheckHomography / CheckFundamental: one match (:457-508, :546-594) ----
// Returns bIn; t1 / t2 are the two score terms (0 where chiSquare > th).

__host__ __device__ static inline bool init_check_h(const float *H21, const float *H12, const float4 r,
                                                    float invSigmaSquare, float *t1, float *t2)
{
    const float th = 5.991f;
    const float u1 = r.x, v1 = r.y, u2 = r.z, v2 = r.w;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    *t1 = 0.f, *t2 = 0.f;
    if (chiSquare1 > th)
        bIn = false;
    else
        *t1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
        bIn = false;
    else
        *t2 = th - chiSquare2;
    return bIn;
}

__host__ __device__ static inline bool init_check_f(const float *F, const float4 r, float invSigmaSquare,
                                                    float *t1, float *t2)
{
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = r.x, v1 = r.y, u2 = r.z, v2 = r.w;
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    *t1 = 0.f, *t2 = 0.f;
    if (chiSquare1 > th)
        bIn = false;
    else
        *t1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
        bIn = false;
    else
        *t2 = thScore - chiSquare2;
    return bIn;
}

__host__ __device__ static inline float init_inv_sigma2(float sigma)
{
    return (float)(1.0 / (double)(sigma * sigma));
}

// ---- the reconstruction ----

// a = U diag(w) V^T with w descending; every right singular vector has its component of
// largest magnitude (the first of equals) positive.  rank2: the third vectors are the cross
// products of the first two (DecomposeE).
__host__ __device__ static inline void init_svd3(const double a[9], double U[3][3], double w[3],
                                                 double V[3][3], bool rank2)
{
    double n2[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) U[i][j] = a[3 * i + j];
    init_jacobi3_sorted(U, V, n2);
    for (int k = 0; k < 3; k++) {
        w[k] = sqrt(n2[k]);
        const double inv = 1.0 / w[k];
        const double sg = largest_sign3(V, k);
        for (int i = 0; i < 3; i++) {
            U[i][k] = (U[i][k] * inv) * sg;
            V[i][k] = V[i][k] * sg;
        }
    }
    if (rank2) {
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        V[0][2] = V[1][0] * V[2][1] - V[2][0] * V[1][1];
        V[1][2] = V[2][0] * V[0][1] - V[0][0] * V[2][1];
        V[2][2] = V[0][0] * V[1][1] - V[1][0] * V[0][1];
    }
}

__host__ __device__ static inline double init_det3(const double m[3][3])
{
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) -
            m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// c = a b for float 3x3 (row-major): products and sums in double, rounded once (cv::gemm)
__host__ __device__ static inline void init_mul3f(const float *a, const float *b, float *c)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            c[3 * i + j] = (float)(((double)a[3 * i] * b[j] + (double)a[3 * i + 1] * b[3 + j]) +
                                   (double)a[3 * i + 2] * b[6 + j]);
}

// One motion hypothesis as CheckRT sees it (:1109-1128)
struct InitHyp {
    float R[9], t[3];
    float P2[12];  // K [R | t]
    float O2[3];   // -R^T t
};

__host__ __device__ static inline void init_hyp_setup(InitHyp *h, const orbg_init_problem &P)
{
    const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            const float x0 = j < 3 ? h->R[j] : h->t[0], x1 = j < 3 ? h->R[3 + j] : h->t[1];
            const float x2 = j < 3 ? h->R[6 + j] : h->t[2];
            h->P2[4 * i + j] = (float)(((double)K[3 * i] * x0 + (double)K[3 * i + 1] * x1) +
                                       (double)K[3 * i + 2] * x2);
        }
    for (int i = 0; i < 3; i++)
        h->O2[i] = (float)(((double)(-h->R[i]) * h->t[0] + (double)(-h->R[3 + i]) * h->t[1]) +
                           (double)(-h->R[6 + i]) * h->t[2]);
}

// DecomposeE on E21 = K^T F21 K: the four hypotheses of ReconstructF (:630-644)
__host__ __device__ static inline void init_decompose_f(const float *F21, const orbg_init_problem &P,
                                                        InitHyp *hyp)
{
    const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
    const float Kt[9] = {P.fx, 0.f, 0.f, 0.f, P.fy, 0.f, P.cx, P.cy, 1.f};
    float KtF[9], E[9];
    init_mul3f(Kt, F21, KtF);
    init_mul3f(KtF, K, E);
    double a[9], U[3][3], w[3], V[3][3];
    for (int k = 0; k < 9; k++) a[k] = E[k];
    init_svd3(a, U, w, V, true);
    float u[9], vt[9], t[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) u[3 * i + j] = (float)U[i][j], vt[3 * i + j] = (float)V[j][i];
    // t = u.col(2) / norm(t): the norm in double, the division per float entry
    const double nt = sqrt(((double)u[2] * u[2] + (double)u[5] * u[5]) + (double)u[8] * u[8]);
    for (int k = 0; k < 3; k++) t[k] = (float)((double)u[3 * k + 2] / nt);
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float uw[9], R1[9], R2[9];
    init_mul3f(u, Wm, uw);
    init_mul3f(uw, vt, R1);
    init_mul3f(u, Wt, uw);
    init_mul3f(uw, vt, R2);
    double d1[3][3], d2[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d1[i][j] = R1[3 * i + j], d2[i][j] = R2[3 * i + j];
    if (init_det3(d1) < 0.0)
        for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    if (init_det3(d2) < 0.0)
        for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    for (int q = 0; q < 4; q++) {
        const float *R = (q & 1) ? R2 : R1;
        for (int k = 0; k < 9; k++) hyp[q].R[k] = R[k];
        for (int k = 0; k < 3; k++) hyp[q].t[k] = q < 2 ? t[k] : -t[k];
        init_hyp_setup(&hyp[q], P);
    }
}

// The eight hypotheses of ReconstructH (:760-864).  false: the early return of :775.
__host__ __device__ static inline bool init_decompose_h(const float *H21, const orbg_init_problem &P,
                                                        InitHyp *hyp)
{
    const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
    // invK = K.inv(): of the upper-triangular K, in double, rounded once
    const double ifx = 1.0 / (double)P.fx, ify = 1.0 / (double)P.fy;
    const float invK[9] = {(float)ifx, 0.f, (float)(-(double)P.cx * ifx), 0.f, (float)ify,
                           (float)(-(double)P.cy * ify), 0.f, 0.f, 1.f};
    float iH[9], Af[9];
    init_mul3f(invK, H21, iH);
    init_mul3f(iH, K, Af);
    double a[9], Ud[3][3], wd[3], Vd[3][3];
    for (int k = 0; k < 9; k++) a[k] = Af[k];
    init_svd3(a, Ud, wd, Vd, false);
    // s = det(U) det(Vt); the early return in float on the float singular values
    double Vtd[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Vtd[i][j] = Vd[j][i];
    const double s = init_det3(Ud) * init_det3(Vtd);
    {
        const float d1 = (float)wd[0], d2 = (float)wd[1], d3 = (float)wd[2];
        if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    }
    // the Faugeras hypotheses in double, R and t rounded to float once: the float expressions
    // cancel in d1 - d3 and leave an R that is no rotation when the singular values are close
    const double d1 = wd[0], d2 = wd[1], d3 = wd[2];
    const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const double aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const double x1[4] = {aux1, aux1, -aux1, -aux1};
    const double x3[4] = {aux3, -aux3, aux3, -aux3};
    const double aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const double ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const double stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const double aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const double cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const double sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int q = 0; q < 8; q++) {
        const int i = q & 3;
        double Rp[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, tp[3];
        if (q < 4) {
            Rp[0][0] = ctheta, Rp[0][2] = -stheta[i], Rp[2][0] = stheta[i], Rp[2][2] = ctheta;
            tp[0] = x1[i] * (d1 - d3), tp[1] = 0.0, tp[2] = -x3[i] * (d1 - d3);
        } else {
            Rp[0][0] = cphi, Rp[0][2] = sphi[i], Rp[1][1] = -1.0, Rp[2][0] = sphi[i], Rp[2][2] = -cphi;
            tp[0] = x1[i] * (d1 + d3), tp[1] = 0.0, tp[2] = x3[i] * (d1 + d3);
        }
        double UR[3][3], t[3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                UR[r][c] = s * ((Ud[r][0] * Rp[0][c] + Ud[r][1] * Rp[1][c]) + Ud[r][2] * Rp[2][c]);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                hyp[q].R[3 * r + c] = (float)((UR[r][0] * Vtd[0][c] + UR[r][1] * Vtd[1][c]) + UR[r][2] * Vtd[2][c]);
        for (int k = 0; k < 3; k++) t[k] = (Ud[k][0] * tp[0] + Ud[k][1] * tp[1]) + Ud[k][2] * tp[2];
        const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        for (int k = 0; k < 3; k++) hyp[q].t[k] = (float)(t[k] / nt);
        init_hyp_setup(&hyp[q], P);
    }
    return true;  // vn (:817-825, :855-863) is never read
}

// Triangulate (:939-973): x3D = (float)(v[k] / v[3]) of the right singular vector of least
// singular value of the float A.
__host__ __device__ static inline void init_triangulate(const float *P2, const orbg_init_problem &P,
                                                        float u1, float v1, float u2, float v2,
                                                        float *x3d)
{
    double b[4][4], v[4][4];
    // P1 = K [I | 0]
    b[0][0] = u1 * 0.f - P.fx, b[0][1] = u1 * 0.f - 0.f, b[0][2] = u1 * 1.f - P.cx, b[0][3] = u1 * 0.f - 0.f;
    b[1][0] = v1 * 0.f - 0.f, b[1][1] = v1 * 0.f - P.fy, b[1][2] = v1 * 1.f - P.cy, b[1][3] = v1 * 0.f - 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        b[2][c] = u2 * P2[8 + c] - P2[c];
        b[3][c] = v2 * P2[8 + c] - P2[4 + c];
    }
    // jacobi_onesided's statements at 4x4, written out: through the call k_init_reconstruct,
    // whose inner loop this is, measured 0.7 % slower
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ORBG_INIT_SWEEPS4; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double al = ((b[0][p] * b[0][p] + b[1][p] * b[1][p]) + b[2][p] * b[2][p]) + b[3][p] * b[3][p];
                const double be = ((b[0][q] * b[0][q] + b[1][q] * b[1][q]) + b[2][q] * b[2][q]) + b[3][q] * b[3][q];
                const double ga = ((b[0][p] * b[0][q] + b[1][p] * b[1][q]) + b[2][p] * b[2][q]) + b[3][p] * b[3][q];
                if (ga == 0.0) continue;
                double c, s;
                jacobi_rot((be - al) / (2.0 * ga), &c, &s);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double bkp = b[k][p], bkq = b[k][q];
                    b[k][p] = c * bkp - s * bkq;
                    b[k][q] = s * bkp + c * bkq;
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double best = 0.0, x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double n2 = ((b[0][k] * b[0][k] + b[1][k] * b[1][k]) + b[2][k] * b[2][k]) + b[3][k] * b[3][k];
        if (k == 0 || n2 < best) {
            best = n2;
            x[0] = v[0][k], x[1] = v[1][k], x[2] = v[2][k], x[3] = v[3][k];
        }
    }
    x3d[0] = (float)(x[0] / x[3]);
    x3d[1] = (float)(x[1] / x[3]);
    x3d[2] = (float)(x[2] / x[3]);
}

// CheckRT's loop body for one inlier match (:1139-1216).  Bit 0: counted in nGood (vP3D and
// vCosParallax take it); bit 1: vbGood.
__host__ __device__ static inline int init_check_point(const InitHyp &h, const orbg_init_problem &P,
                                                       float th2, const float4 r, float *x3d,
                                                       float *cosp)
{
    const float u1 = r.x, v1 = r.y, u2 = r.z, v2 = r.w;
    init_triangulate(h.P2, P, u1, v1, u2, v2, x3d);
    *cosp = 0.f;
    if (!isfinite(x3d[0]) || !isfinite(x3d[1]) || !isfinite(x3d[2])) return 0;
    const float X = x3d[0], Y = x3d[1], Z = x3d[2];
    // normal1 = p3dC1 - O1, normal2 = p3dC1 - O2 (float); cv::norm and dot accumulate in double
    const float n1x = X - 0.f, n1y = Y - 0.f, n1z = Z - 0.f;
    const float n2x = X - h.O2[0], n2y = Y - h.O2[1], n2z = Z - h.O2[2];
    const float dist1 = (float)sqrt(((double)n1x * n1x + (double)n1y * n1y) + (double)n1z * n1z);
    const float dist2 = (float)sqrt(((double)n2x * n2x + (double)n2y * n2y) + (double)n2z * n2z);
    const double dot = ((double)n1x * n2x + (double)n1y * n2y) + (double)n1z * n2z;
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    *cosp = cosParallax;
    if (Z <= 0 && cosParallax < 0.99998) return 0;
    // p3dC2 = R * p3dC1 + t: one gemm
    const float X2 = (float)((((double)h.R[0] * X + (double)h.R[1] * Y) + (double)h.R[2] * Z) + (double)h.t[0]);
    const float Y2 = (float)((((double)h.R[3] * X + (double)h.R[4] * Y) + (double)h.R[5] * Z) + (double)h.t[1]);
    const float Z2 = (float)((((double)h.R[6] * X + (double)h.R[7] * Y) + (double)h.R[8] * Z) + (double)h.t[2]);
    if (Z2 <= 0 && cosParallax < 0.99998) return 0;
    const float invZ1 = (float)(1.0 / (double)Z);
    const float im1x = P.fx * X * invZ1 + P.cx;
    const float im1y = P.fy * Y * invZ1 + P.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;
    const float invZ2 = (float)(1.0 / (double)Z2);
    const float im2x = P.fx * X2 * invZ2 + P.cx;
    const float im2y = P.fy * Y2 * invZ2 + P.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;
    return cosParallax < 0.99998 ? 3 : 1;
}

// th2 = 4.0 * mSigma2 passed as float (:641)
__host__ __device__ static inline float init_th2(float sigma)
{
    return (float)(4.0 * (double)(sigma * sigma));
}

// floats as unsigned keys of the same order (selection of the order statistic)
__host__ __device__ static inline uint32_t init_order_key(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float init_key_value(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
#define INIT_NO_KEY 0xffffffffu

// parallax = acos(vCosParallax[idx]) * 180 / CV_PI
__host__ __device__ static inline float init_parallax(float c)
{
    return (float)(acos((double)c) * 180.0 / 3.1415926535897932384626433832795);
}

// The decision of ReconstructF (:646-721) / ReconstructH (:867-923) from the counts and
// parallaxes.  Returns success; *which = the hypothesis the rule looked at last (-1: none).
__host__ __device__ static inline int init_decide_f(const int *ng, const float *par, int N,
                                                    const orbg_init_problem &P, int *which)
{
    const int maxGood = max(ng[0], max(ng[1], max(ng[2], ng[3])));
    const int nMinGood = max((int)(0.9 * N), P.min_triangulated);
    int nsimilar = 0;
    for (int k = 0; k < 4; k++)
        if (ng[k] > 0.7 * maxGood) nsimilar++;
    *which = -1;
    if (maxGood < nMinGood || nsimilar > 1) return 0;
    for (int k = 0; k < 4; k++)
        if (maxGood == ng[k]) {
            *which = k;
            return par[k] > P.min_parallax ? 1 : 0;
        }
    return 0;
}

__host__ __device__ static inline int init_decide_h(const int *ng, const float *par, int N,
                                                    const orbg_init_problem &P, int *which)
{
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    for (int i = 0; i < 8; i++) {
        if (ng[i] > bestGood) {
            secondBestGood = bestGood;
            bestGood = ng[i];
            bestSolutionIdx = i;
            bestParallax = par[i];
        } else if (ng[i] > secondBestGood) {
            secondBestGood = ng[i];
        }
    }
    *which = bestSolutionIdx;
    return (secondBestGood < 0.75 * bestGood && bestParallax >= P.min_parallax &&
            bestGood > P.min_triangulated && bestGood > 0.9 * N)
               ? 1
               : 0;
}

// RH and the model from the two best scores (:177-184)
__host__ __device__ static inline int init_model(float SH, float SF, float *RH)
{
    *RH = SH / (SH + SF);
    if (!(SH > 0.f) && !(SF > 0.f)) return 0;
    return *RH > 0.40 ? 1 : 2;
}

}  // namespace orbg
