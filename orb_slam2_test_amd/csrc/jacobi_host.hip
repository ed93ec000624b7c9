// jacobi_host.hip -- the solvers' entry points that sit on jacobi.h (sim3_args.h, pnp_device.h,
// init_device.h), run on the host over seeded inputs; every output value is printed exactly
// (%a), one named section per entry point.  No kernel and no GPU: the functions are __host__
// __device__ and the build forbids contraction, so these are the kernels' statements.
// tests/test_jacobi_host.py pins a digest per section, which holds the bits across changes to
// the shared solves.
//
// The inputs come from an integer LCG scaled by exact powers of two, plus the degenerate cases
// each solve has a branch for.  A NaN is printed as `nan`: its sign and payload are not pinned.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "init_device.h"
#include "pnp_device.h"
#include "sim3_args.h"

#pragma clang fp contract(off)

using namespace orbg;

static uint64_t g_state;

static void seed(uint64_t s) { g_state = s * 0x9e3779b97f4a7c15ull + 1; }

// uniform in [-1, 1) on a grid of 2^-23: exact in float and in double
static double unit()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return std::ldexp((double)(int32_t)((g_state >> 40) & 0xffffff) - 8388608.0, -23);
}

static void put(const char *name, const double *v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; i++) {
        if (v[i] != v[i])
            printf(" nan");
        else
            printf(" %a", v[i]);
    }
    printf("\n");
}

static void putf(const char *name, const float *v, int n)
{
    double d[16];
    for (int i = 0; i < n; i++) d[i] = v[i];
    put(name, d, n);
}

// ---- sim3_horn ----

static void horn_case(const float p1[3][3], const float p2[3][3])
{
    for (int fix = 0; fix < 2; fix++) {
        orbg_sim3_hyp H;
        memset(&H, 0, sizeof(H));
        const double ok = sim3_horn(p1, p2, fix != 0, &H) ? 1.0 : 0.0;
        put("ok", &ok, 1);
        putf("R", H.R, 9);
        putf("t", H.t, 3);
        putf("s", &H.s, 1);
    }
}

static void section_horn()
{
    printf("[sim3_horn]\n");
    float p1[3][3], p2[3][3];
    for (int n = 0; n < 24; n++) {
        seed(100 + n);
        for (int k = 0; k < 3; k++)
            for (int d = 0; d < 3; d++) p1[k][d] = (float)(4.0 * unit()), p2[k][d] = (float)(4.0 * unit());
        horn_case(p1, p2);
    }
    for (int n = 0; n < 4; n++) {  // a related pair: p1 = a rotation of p2 about z, scaled and moved
        seed(150 + n);
        for (int k = 0; k < 3; k++) {
            for (int d = 0; d < 3; d++) p2[k][d] = (float)(2.0 * unit());
            p1[k][0] = 1.5f * (0.6f * p2[k][0] - 0.8f * p2[k][1]) + 1.0f;
            p1[k][1] = 1.5f * (0.8f * p2[k][0] + 0.6f * p2[k][1]) - 2.0f;
            p1[k][2] = 1.5f * p2[k][2] + 0.5f;
        }
        horn_case(p1, p2);
    }
    for (int k = 0; k < 3; k++)  // a collinear triple
        for (int d = 0; d < 3; d++) p1[k][d] = (float)(1 + d + k * (d + 1)), p2[k][d] = (float)(2 - d + k * (3 - d));
    horn_case(p1, p2);
    seed(180);  // two identical points
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) p1[k][d] = (float)unit(), p2[k][d] = (float)unit();
    for (int d = 0; d < 3; d++) p1[1][d] = p1[0][d], p2[1][d] = p2[0][d];
    horn_case(p1, p2);
    // a pure translation of a triple whose moments are diagonal: every off-diagonal entry of
    // the 4x4 is zero and every plane is skipped
    const float r[3][3] = {{1.f, 1.f, 0.f}, {-1.f, 1.f, 0.f}, {0.f, -2.f, 0.f}};
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) p1[k][d] = r[k][d] + 3.f * (d + 1), p2[k][d] = r[k][d] - 6.f * (d + 1);
    horn_case(p1, p2);
}

// ---- pnp_control_points / pnp_polar3 / the EPnP chain ----

static void control_case(const double c0[3], const double cov[6], double n)
{
    static PnpWork W;
    memset(&W, 0, sizeof(W));
    pnp_control_points(&W, c0, cov, n);
    put("cw", &W.cw[0][0], 12);
    put("ku", &W.ku[0][0], 9);
    put("npts", &W.npts, 1);
}

static void section_control_points()
{
    printf("[pnp_control_points]\n");
    for (int n = 0; n < 24; n++) {
        seed(200 + n);
        const int m = 4 + n % 5;
        double pw[8][3], c0[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < m; k++)
            for (int d = 0; d < 3; d++) pw[k][d] = 3.0 * unit(), c0[d] += pw[k][d];
        for (int d = 0; d < 3; d++) c0[d] /= m;
        for (int k = 0; k < m; k++) {
            const double d0 = pw[k][0] - c0[0], d1 = pw[k][1] - c0[1], d2 = pw[k][2] - c0[2];
            cov[0] += d0 * d0, cov[1] += d0 * d1, cov[2] += d0 * d2;
            cov[3] += d1 * d1, cov[4] += d1 * d2, cov[5] += d2 * d2;
        }
        control_case(c0, cov, (double)m);
    }
    const double c0[3] = {0.5, -1.0, 2.0};
    const double diag[6] = {1.0, 0.0, 0.0, 3.0, 0.0, 2.0};
    const double twin[6] = {3.0, 1.0, 1.0, 3.0, 1.0, 3.0};   // eigenvalues 5, 2, 2
    const double rank1[6] = {1.0, 2.0, 3.0, 4.0, 6.0, 9.0};  // (1, 2, 3) (1, 2, 3)^T
    control_case(c0, diag, 4.0);
    control_case(c0, twin, 5.0);
    control_case(c0, rank1, 6.0);
}

static void polar_case(double b[3][3])
{
    double R[9];
    pnp_polar3(b, R);
    put("R", R, 9);
    put("b", &b[0][0], 9);
}

static void section_polar()
{
    printf("[pnp_polar3]\n");
    double b[3][3];
    for (int n = 0; n < 32; n++) {
        seed(300 + n);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) b[i][j] = 2.0 * unit();
        polar_case(b);
    }
    double rot[3][3] = {{0.0, -1.0, 0.0}, {1.0, 0.0, 0.0}, {0.0, 0.0, 1.0}};
    polar_case(rot);
    double rot2[3][3] = {{0.6, -0.8, 0.0}, {0.8, 0.6, 0.0}, {0.0, 0.0, 1.0}};
    polar_case(rot2);
    seed(340);  // a zero column: its norm divides by zero
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) b[i][j] = j == 1 ? 0.0 : unit();
    polar_case(b);
}

// compute_pose on a sampled set, as k_pnp_hypothesis feeds it
static void section_epnp()
{
    printf("[pnp_tail]\n");
    static PnpWork W;
    const int sizes[3] = {4, 5, 8};
    const double fu = 500.0, fv = 480.0, uc = 320.0, vc = 240.0;
    for (int n = 0; n < 30; n++) {
        seed(400 + n);
        const int m = sizes[n % 3];
        memset(&W, 0, sizeof(W));
        double pw[8][3], uv[8][2], rec[8][PNP_REC];
        for (int k = 0; k < m; k++) {
            const float X = (float)(2.0 * unit()), Y = (float)(2.0 * unit()), Z = (float)(2.0 * unit());
            const double xc = (0.6 * X - 0.8 * Y) + 0.25, yc = (0.8 * X + 0.6 * Y) - 0.5, zc = Z + 6.0;
            const float u = (float)((uc + fu * xc / zc) + 0.5 * unit());
            const float v = (float)((vc + fv * yc / zc) + 0.5 * unit());
            pw[k][0] = X, pw[k][1] = Y, pw[k][2] = Z, uv[k][0] = u, uv[k][1] = v;
        }
        double c0[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < m; k++) c0[0] += pw[k][0], c0[1] += pw[k][1], c0[2] += pw[k][2];
        c0[0] /= m, c0[1] /= m, c0[2] /= m;
        for (int k = 0; k < m; k++) {
            const double d0 = pw[k][0] - c0[0], d1 = pw[k][1] - c0[1], d2 = pw[k][2] - c0[2];
            cov[0] += d0 * d0, cov[1] += d0 * d1, cov[2] += d0 * d2;
            cov[3] += d1 * d1, cov[4] += d1 * d2, cov[5] += d2 * d2;
        }
        pnp_control_points(&W, c0, cov, (double)m);
        for (int k = 0; k < m; k++)
            pnp_point_rec(&W, pw[k][0], pw[k][1], pw[k][2], uv[k][0], uv[k][1], uc, vc, rec[k]);
        for (int j = 0; j < 4; j++) W.afirst[j] = rec[0][j];
        for (int e = 0; e < PNP_SUMS; e++) {
            double s = 0.0;
            for (int k = 0; k < m; k++) s += pnp_sum_term(e, rec[k], fu, fv);
            pnp_sum_store(&W, e, s);
        }
        pnp_tail(&W, 0, 1);
        for (int c = 0; c < 3; c++) {
            put("R", W.c[c].R, 9);
            put("t", W.c[c].t, 3);
        }
        double ev[12];
        for (int k = 0; k < 12; k++) ev[k] = W.A[13 * k];
        put("eig", ev, 12);
    }
}

// ---- init_hypothesis / init_svd3 / init_triangulate ----

// a camera at (R about y by (c, s)) X + t, pixels through (fx, fy, cx, cy)
static void pixel(const float X[3], float c, float s, const float t[3], const orbg_init_problem &P,
                  float *u, float *v)
{
    const float x = (c * X[0] + s * X[2]) + t[0], y = X[1] + t[1], z = (-s * X[0] + c * X[2]) + t[2];
    *u = P.fx * x / z + P.cx;
    *v = P.fy * y / z + P.cy;
}

static InitNorm norm_of(const float (*px)[4], int o)
{
    float mx = 0.f, my = 0.f, dx = 0.f, dy = 0.f;
    for (int j = 0; j < 8; j++) mx += px[j][o], my += px[j][o + 1];
    mx /= 8.f, my /= 8.f;
    for (int j = 0; j < 8; j++) dx += fabsf(px[j][o] - mx), dy += fabsf(px[j][o + 1] - my);
    InitNorm n;
    n.mx = mx, n.my = my, n.sx = 8.f / dx, n.sy = 8.f / dy;
    return n;
}

static void section_hypothesis()
{
    printf("[init_hypothesis]\n");
    static InitWork W;
    const orbg_init_problem P = {520.f, 510.f, 320.f, 240.f, 1.f, 1.f, 50, 200};
    const float t0[3] = {0.f, 0.f, 0.f}, t1[3] = {-0.5f, 0.125f, 0.25f};
    for (int n = 0; n < 26; n++) {
        seed(500 + n);
        float px[8][4];
        for (int j = 0; j < 8; j++) {
            float X[3] = {(float)(2.0 * unit()), (float)(1.5 * unit()), (float)(5.0 + 2.0 * unit())};
            if (n == 24) X[2] = 5.f + 0.25f * X[0];  // a planar set
            pixel(X, 1.f, 0.f, t0, P, &px[j][0], &px[j][1]);
            pixel(X, 0.96f, 0.28f, t1, P, &px[j][2], &px[j][3]);
            px[j][2] += (float)(0.25 * unit()), px[j][3] += (float)(0.25 * unit());
        }
        if (n == 25)  // a repeated point
            for (int k = 0; k < 4; k++) px[7][k] = px[2][k];
        const InitNorm n1 = norm_of(px, 0), n2 = norm_of(px, 2);
        memset(&W, 0, sizeof(W));
        for (int j = 0; j < 8; j++) {
            init_normalized(make_float4(px[j][0], px[j][1], px[j][2], px[j][3]), n1, n2, W.pn[j]);
            W.idx[j] = j;
        }
        W.ok = 1;
        float H21[9], H12[9], F21[9];
        init_hypothesis(&W, n1, n2, true, H21, H12, F21, 0, 1);
        putf("H21", H21, 9);
        putf("H12", H12, 9);
        putf("F21", F21, 9);
    }
}

static void svd_case(const double a[9])
{
    for (int rank2 = 0; rank2 < 2; rank2++) {
        double U[3][3], w[3], V[3][3];
        init_svd3(a, U, w, V, rank2 != 0);
        put("U", &U[0][0], 9);
        put("w", w, 3);
        put("V", &V[0][0], 9);
    }
}

static void section_svd()
{
    printf("[init_svd3]\n");
    double a[9];
    for (int n = 0; n < 32; n++) {
        seed(600 + n);
        for (int k = 0; k < 9; k++) a[k] = 3.0 * unit();
        svd_case(a);
    }
    seed(640);  // rank 2: the sum of two outer products
    double x[3], y[3], p[3], q[3];
    for (int k = 0; k < 3; k++) x[k] = unit(), y[k] = unit(), p[k] = unit(), q[k] = unit();
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[3 * i + j] = x[i] * y[j] + p[i] * q[j];
    svd_case(a);
    const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    svd_case(eye);
}

static void section_triangulate()
{
    printf("[init_triangulate]\n");
    const orbg_init_problem P = {520.f, 510.f, 320.f, 240.f, 1.f, 1.f, 50, 200};
    for (int n = 0; n < 40; n++) {
        seed(700 + n);
        // R about y by an angle with (c, s) = (1 - 2 a^2, 2 a sqrt(1 - a^2)) rounded to float
        const float a = (float)(0.25 * unit());
        const float c = 1.f - 2.f * a * a, s = 2.f * a * sqrtf(1.f - a * a);
        float t[3] = {(float)unit(), (float)(0.25 * unit()), (float)(0.25 * unit())};
        const bool still = n >= 36;  // zero baseline: P2 = K [I | 0]
        if (still) t[0] = t[1] = t[2] = 0.f;
        const float cc = still ? 1.f : c, ss = still ? 0.f : s;
        const float R[9] = {cc, 0.f, ss, 0.f, 1.f, 0.f, -ss, 0.f, cc};
        float P2[12];
        for (int j = 0; j < 4; j++) {
            const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
            P2[j] = P.fx * r0 + P.cx * r2;
            P2[4 + j] = P.fy * r1 + P.cy * r2;
            P2[8 + j] = r2;
        }
        const float X[3] = {(float)(2.0 * unit()), (float)(1.5 * unit()), (float)(6.0 + 3.0 * unit())};
        const float t0[3] = {0.f, 0.f, 0.f};
        float u1, v1, u2, v2, x3d[3];
        pixel(X, 1.f, 0.f, t0, P, &u1, &v1);
        pixel(X, cc, ss, t, P, &u2, &v2);
        u2 += (float)(0.5 * unit()), v2 += (float)(0.5 * unit());
        init_triangulate(P2, P, u1, v1, u2, v2, x3d);
        putf("x3d", x3d, 3);
    }
}

int main()
{
    section_horn();
    section_control_points();
    section_polar();
    section_epnp();
    section_hypothesis();
    section_svd();
    section_triangulate();
    return 0;
}
