// init_host.hip -- Initializer::Initialize on one host core, through the very __host__
// __device__ statements the kernels of init_kernels.hip run (init_device.h) and in the kernels'
// summation orders (Normalize: 256 strided partial sums and a binary tree; a score: 64 strided
// partial sums and a butterfly), so its records equal the device's.  No kernel and no GPU:
// tools/init_bench.py times it, and tests/test_initializer_ref.py checks the shared arithmetic
// with it.
//
//   init_host <in> <out> [repeat]
//   init_host decide <model> <N> <minParallax> <minTriangulated> <nGood x 8> <parallax x 8>
//   in : int32 npairs, cap, max_its, frame_stride, nframes, match_stride, 0, 0;
//        orbg_init_problem[npairs];
//        orbg_keypoint[nframes][frame_stride]; int32 counts[nframes]; int32 f1[npairs],
//        f2[npairs]; int32 matches12[npairs][match_stride]; int32 sets[npairs][max_its][8]
//   out: orbg_init_result[npairs]; float p3d[npairs][cap][3]; uint8 triangulated[npairs][cap];
//        float scores_h[npairs][max_its], scores_f[..]; float H21[npairs][max_its][9], F21[..];
//        uint64 masks_h[npairs][max_its][cap / 64], masks_f[..]
// Prints the seconds of one pass over the batch (the best of `repeat`).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "init_device.h"

#pragma clang fp contract(off)

using namespace orbg;

#define IH_T 256

// the kernel's init_block_sum2 on the 256 per-thread values
static double tree(double *v)
{
    for (int d = IH_T / 2; d > 0; d >>= 1)
        for (int t = 0; t < d; t++) v[t] += v[t + d];
    return v[0];
}

static InitNorm normalize(const orbg_keypoint *k, int n)
{
    double ax[IH_T] = {0}, ay[IH_T] = {0};
    for (int i = 0; i < n; i++) ax[i % IH_T] += (double)k[i].x, ay[i % IH_T] += (double)k[i].y;
    const float meanX = (float)(tree(ax) / n), meanY = (float)(tree(ay) / n);
    memset(ax, 0, sizeof(ax));
    memset(ay, 0, sizeof(ay));
    for (int i = 0; i < n; i++) {
        ax[i % IH_T] += (double)fabsf(k[i].x - meanX);
        ay[i % IH_T] += (double)fabsf(k[i].y - meanY);
    }
    const float meanDevX = (float)(tree(ax) / n), meanDevY = (float)(tree(ay) / n);
    InitNorm o;
    o.mx = meanX, o.my = meanY;
    o.sx = (float)(1.0 / (double)meanDevX), o.sy = (float)(1.0 / (double)meanDevY);
    return o;
}

// the kernel's init_wave_sum
static double butterfly(double *a)
{
    for (int o = 32; o > 0; o >>= 1) {
        double b[64];
        for (int l = 0; l < 64; l++) b[l] = a[l] + a[l ^ o];
        memcpy(a, b, sizeof(b));
    }
    return a[0];
}

struct Batch {
    int np, cap, its, stride, nframes, mstride;
    std::vector<orbg_init_problem> probs;
    std::vector<orbg_keypoint> kps;
    std::vector<int32_t> counts, f1, f2, m12, sets;
    std::vector<orbg_init_result> res;
    std::vector<float> p3d, sh, sf, H21, F21;
    std::vector<uint8_t> tri;
    std::vector<uint64_t> mh, mf;
};

static int frame(const Batch &B, int f, int limit, const orbg_keypoint **k)
{
    *k = B.kps.data();
    if (f < 0 || f >= B.nframes) return 0;
    *k = B.kps.data() + (size_t)f * B.stride;
    const int n = B.counts[f];
    return n < 0 ? 0 : (n > limit ? limit : n);
}

static void initialize_one(Batch &B, int p)
{
    const orbg_init_problem P = B.probs[p];
    const int cap = B.cap, words = cap / 64;
    const orbg_keypoint *k1, *k2;
    const int n1 = frame(B, B.f1[p], std::min(std::min(cap, B.stride), B.mstride), &k1);
    const int n2 = frame(B, B.f2[p], B.stride, &k2);
    const InitNorm nm1 = normalize(k1, n1), nm2 = normalize(k2, n2);
    std::vector<float4> recs;
    std::vector<int> first;
    for (int i = 0; i < n1; i++) {
        const int m = B.m12[(size_t)p * B.mstride + i];
        if (m >= 0 && m < n2) {
            recs.push_back(make_float4(k1[i].x, k1[i].y, k2[m].x, k2[m].y));
            first.push_back(i);
        }
    }
    const int N = (int)recs.size(), its = init_iterations(P, N, B.its);
    const size_t row0 = (size_t)p * B.its;
    std::vector<float> H12((size_t)B.its * 9, 0.f);
    const float invSigmaSquare = init_inv_sigma2(P.sigma);
    InitWork W;
    for (int it = 0; it < B.its; it++) {
        const size_t row = row0 + it;
        float *H21 = &B.H21[row * 9], *F21 = &B.F21[row * 9], *h12 = &H12[(size_t)it * 9];
        uint64_t *mh = &B.mh[row * words], *mf = &B.mf[row * words];
        memset(H21, 0, 36), memset(F21, 0, 36), memset(mh, 0, words * 8), memset(mf, 0, words * 8);
        B.sh[row] = B.sf[row] = 0.f;
        if (it >= its) continue;
        bool ok = true;
        for (int j = 0; j < 8; j++) {
            const int s = B.sets[row * 8 + j];
            const bool good = s >= 0 && s < N;
            W.idx[j] = good ? s : -1;
            ok = ok && good;
            for (int i = 0; i < j; i++) ok = ok && W.idx[i] != W.idx[j];
            if (good)
                init_normalized(recs[s], nm1, nm2, W.pn[j]);
            else
                W.pn[j][0] = W.pn[j][1] = W.pn[j][2] = W.pn[j][3] = 0.f;
        }
        W.ok = ok ? 1 : 0;
        init_hypothesis(&W, nm1, nm2, true, H21, h12, F21, 0, 1);
        for (int m = 0; m < 2; m++) {
            const float *M = m ? F21 : H21;
            if (init_is_zero9(M)) continue;
            uint64_t *mask = m ? mf : mh;
            double acc[64] = {0};
            for (int i = 0; i < N; i++) {
                float t1, t2;
                const bool in = m ? init_check_f(M, recs[i], invSigmaSquare, &t1, &t2)
                                  : init_check_h(M, h12, recs[i], invSigmaSquare, &t1, &t2);
                if (in) mask[i >> 6] |= 1ull << (i & 63);
                acc[i & 63] += (double)t1;
                acc[i & 63] += (double)t2;
            }
            (m ? B.sf : B.sh)[row] = (float)butterfly(acc);
        }
    }
    // the first strict maxima, the model, the reconstruction
    orbg_init_result &R = B.res[p];
    memset(&R, 0, sizeof(R));
    float S[2] = {0.f, 0.f};
    int best[2] = {-1, -1};
    for (int m = 0; m < 2; m++)
        for (int it = 0; it < its; it++) {
            const float s = (m ? B.sf : B.sh)[row0 + it];
            if (s > S[m]) S[m] = s, best[m] = it;
        }
    float RH;
    int model = init_model(S[0], S[1], &RH);
    if (best[model == 1 ? 0 : 1] < 0) model = 0;
    InitHyp hyp[8];
    int nhyp = 0;
    const uint64_t *mask = nullptr;
    if (model == 1) {
        nhyp = init_decompose_h(&B.H21[(row0 + best[0]) * 9], P, hyp) ? 8 : 0;
        mask = &B.mh[(row0 + best[0]) * words];
    } else if (model == 2) {
        init_decompose_f(&B.F21[(row0 + best[1]) * 9], P, hyp);
        nhyp = 4;
        mask = &B.mf[(row0 + best[1]) * words];
    }
    int ninl = 0;
    if (mask)
        for (int w = 0; w < (N + 63) / 64; w++) ninl += __builtin_popcountll(mask[w]);
    const float th2 = init_th2(P.sigma);
    int ng[8] = {0};
    float par[8] = {0.f};
    std::vector<uint32_t> keys;
    for (int h = 0; h < nhyp; h++) {
        keys.clear();
        for (int i = 0; i < N; i++)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                float x3d[3], cosp;
                if (init_check_point(hyp[h], P, th2, recs[i], x3d, &cosp) & 1) keys.push_back(init_order_key(cosp));
            }
        ng[h] = (int)keys.size();
        if (ng[h] > 0) {
            const int k = std::min(50, ng[h] - 1);
            std::nth_element(keys.begin(), keys.begin() + k, keys.end());
            par[h] = init_parallax(init_key_value(keys[k]));
        }
    }
    int which = -1, success = 0;
    if (model == 1 && nhyp) success = init_decide_h(ng, par, ninl, P, &which);
    if (model == 2) success = init_decide_f(ng, par, ninl, P, &which);
    float *p3d = &B.p3d[(size_t)p * cap * 3];
    uint8_t *tri = &B.tri[(size_t)p * cap];
    memset(p3d, 0, (size_t)cap * 12);
    memset(tri, 0, cap);
    int ntri = 0;
    if (success)
        for (int i = 0; i < N; i++)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) {
                float x3d[3], cosp;
                const int f = init_check_point(hyp[which], P, th2, recs[i], x3d, &cosp);
                if (f & 1) memcpy(p3d + 3 * first[i], x3d, 12);
                if (f & 2) tri[first[i]] = 1, ntri++;
            }
    R.n = N, R.best_h = best[0], R.best_f = best[1];
    R.SH = S[0], R.SF = S[1], R.RH = RH;
    R.model = model, R.success = success, R.hyp = which;
    R.ntriangulated = ntri, R.ninliers = ninl, R.nhyp = nhyp;
    for (int h = 0; h < 8; h++) R.ngood[h] = ng[h], R.parallax[h] = par[h];
    for (int h = 0; h < nhyp; h++) {
        memcpy(R.hyp_R[h], hyp[h].R, 36);
        memcpy(R.hyp_t[h], hyp[h].t, 12);
    }
    if (success) memcpy(R.R21, hyp[which].R, 36), memcpy(R.t21, hyp[which].t, 12);
}

template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T>
static void wr(FILE *f, const std::vector<T> &v)
{
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv)
{
    if (argc == 22 && !strcmp(argv[1], "decide")) {
        // init_host decide <model> <N> <minParallax> <minTriangulated> <nGood x 8> <parallax x 8>:
        // the decision of ReconstructH (model 1) / ReconstructF (model 2) alone, as the kernel
        // takes it from its counts; prints "<success> <hypothesis>"
        orbg_init_problem P = {};
        P.min_parallax = (float)atof(argv[4]);
        P.min_triangulated = atoi(argv[5]);
        int ng[8], which;
        float par[8];
        for (int k = 0; k < 8; k++) ng[k] = atoi(argv[6 + k]), par[k] = (float)atof(argv[14 + k]);
        const int ok = atoi(argv[2]) == 1 ? init_decide_h(ng, par, atoi(argv[3]), P, &which)
                                          : init_decide_f(ng, par, atoi(argv[3]), P, &which);
        printf("%d %d\n", ok, which);
        return 0;
    }
    if (argc < 3) {
        fprintf(stderr, "usage: %s <in> <out> [repeat] | decide ...\n", argv[0]);
        return 2;
    }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[8];
    if (!f || fread(hd, 4, 8, f) != 8) return 1;
    Batch B;
    B.np = hd[0], B.cap = hd[1], B.its = hd[2], B.stride = hd[3], B.nframes = hd[4], B.mstride = hd[5];
    if (B.np < 0 || B.cap < 64 || (B.cap & 63) || B.cap > ORBG_INIT_MAX_N || B.its < 1 || B.stride < 1 ||
        B.nframes < 1 || B.its > (1 << 20) || B.mstride < 1)
        return 1;
    const size_t np = B.np, rows = np * B.its, words = B.cap / 64;
    if (!rd(f, B.probs, np) || !rd(f, B.kps, (size_t)B.nframes * B.stride) || !rd(f, B.counts, B.nframes) ||
        !rd(f, B.f1, np) || !rd(f, B.f2, np) || !rd(f, B.m12, np * B.mstride) || !rd(f, B.sets, rows * 8))
        return 1;
    fclose(f);
    B.res.resize(np);
    B.p3d.resize(np * B.cap * 3), B.tri.resize(np * B.cap);
    B.sh.resize(rows), B.sf.resize(rows), B.H21.resize(rows * 9), B.F21.resize(rows * 9);
    B.mh.resize(rows * words), B.mf.resize(rows * words);
    double best = 1e300;
    for (int r = 0; r < (repeat > 0 ? repeat : 1); r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < B.np; p++) initialize_one(B, p);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dt < best) best = dt;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    wr(f, B.res), wr(f, B.p3d), wr(f, B.tri), wr(f, B.sh), wr(f, B.sf), wr(f, B.H21), wr(f, B.F21);
    wr(f, B.mh), wr(f, B.mf);
    fclose(f);
    printf("%.9f\n", best);
    return 0;
}
