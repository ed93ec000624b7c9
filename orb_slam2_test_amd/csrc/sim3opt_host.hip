// sim3opt_host.hip -- Optimizer::OptimizeSim3 on one host core, through the very
// __host__ __device__ statements k_sim3_opt runs (sim3opt_args.h, g2o_math.h) and in the kernel's
// summation order (256 strided partial sums, butterfly per 64, (w0 + w1) + (w2 + w3)), so its
// records equal the device's bit for bit.  No kernel and no GPU: tools/sim3opt_bench.py times
// it, and tests/test_sim3opt_ref.py checks the shared arithmetic with it.
//
//   sim3opt_host <in> <out> [repeat]
//   in : int32 npairs, cap, n1cap, 0; orbg_sim3opt_problem[npairs];
//        orbg_sim3opt_corr[npairs][cap]; orbg_sim3_hyp[npairs]
//   out: orbg_sim3opt_result[npairs]; uint8 keep[npairs][n1cap]
// Prints the seconds of one pass over the batch (the best of `repeat`).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sim3opt_args.h"

#pragma clang fp contract(off)

using namespace orbg;

#define SO_T 256

// the kernel's wg_reduce on the 256 per-thread values v[t * nv + j]
static void reduce(const std::vector<double> &v, int nv, double *red)
{
    for (int j = 0; j < nv; j++) {
        double w[4];
        for (int wv = 0; wv < 4; wv++) {
            double a[64];
            for (int l = 0; l < 64; l++) a[l] = v[(size_t)(wv * 64 + l) * nv + j];
            for (int o = 32; o > 0; o >>= 1) {
                double b[64];
                for (int l = 0; l < 64; l++) b[l] = a[l] + a[l ^ o];
                memcpy(a, b, sizeof(a));
            }
            w[wv] = a[0];
        }
        red[j] = (w[0] + w[1]) + (w[2] + w[3]);
    }
}

static void optimize_one(const orbg_sim3opt_problem &P, const orbg_sim3opt_corr *corrs,
                         const orbg_sim3_hyp &h0, int cap, int n1cap, orbg_sim3opt_result *res,
                         uint8_t *keep)
{
    const int n = sim3opt_n(P, cap);
    const bool fix_scale = P.fix_scale != 0;
    const double delta = so_huber_delta(P.th2);
    std::vector<uint8_t> dead(n > 0 ? n : 1, 0);
    std::vector<SoPair> E(n > 0 ? n : 1);
    for (int e = 0; e < n; e++) so_pair(P, corrs[e], &E[e]);
    memset(keep, 0, n1cap);
    Sim3d init, est, est_inv, trial, trial_inv, last, last_inv, Pp[SO_NP], Pi[SO_NP];
    so_init(h0, &init);
    est = last = init;
    so_inverse(est, &last_inv);
    int nBad = 0, nIn = 0, its[2] = {0, 0};
    bool give_input = true;
    LmState lm = {0, 2, 0, 0, 0, 0};
    std::vector<double> part((size_t)SO_T * SO_NV), part1(SO_T);
    double red[SO_NV], H[49], b[7], x[7], Hd[7][7];
    for (int round = 0; round < 2 && n > 0; round++) {
        const int iters = round == 0 ? 5 : (nBad > 0 ? 10 : 5);
        int go = 0;
        for (int it = 0; it < iters; it++) {
            for (int k = 0; k < SO_NP; k++) so_perturbed(est, k, fix_scale, &Pp[k], &Pi[k]);
            so_inverse(est, &est_inv);
            std::fill(part.begin(), part.end(), 0.0);
            for (int e = 0; e < n; e++)
                if (!dead[e])
                    so_add_pair(est, est_inv, Pp, Pi, P, E[e], delta, &part[(size_t)(e % SO_T) * SO_NV]);
            reduce(part, SO_NV, red);
            last = est;
            last_inv = est_inv;
            unpack_sys<7>(red, H, b);
            lm.currentChi = red[0];
            lm_begin(&lm, it, it == 0 ? lm_max_diag<7>(H) : 0.0);
            for (;;) {
                const bool ok = so_lm_trial(&lm, H, b, est, fix_scale, x, &trial, Hd);
                so_inverse(trial, &trial_inv);
                last = trial;
                last_inv = trial_inv;
                std::fill(part1.begin(), part1.end(), 0.0);
                for (int e = 0; e < n; e++)
                    if (!dead[e]) part1[e % SO_T] += so_pair_chi(trial, trial_inv, P, E[e], delta);
                double chi;
                reduce(part1, 1, &chi);
                double rho;
                if (lm_trial(&lm, ok, chi, lm_scale<7>(&lm, x, b), &rho)) est = trial;
                go = lm_retry(&lm, rho) ? 1 : (lm_end(&lm, rho) ? 2 : 0);
                if (go != 1) break;
            }
            its[round]++;
            if (go == 2) break;
        }
        int total = 0;
        for (int e = 0; e < n; e++)
            if (!dead[e] && so_is_bad(last, last_inv, P, E[e])) {
                dead[e] = 1;
                total++;
            }
        if (round == 0) {
            nBad = total;
            if (n - nBad < 10) break;
        } else {
            nIn = (n - nBad) - total;
            give_input = false;
        }
    }
    so_result(give_input ? init : est, nIn, nBad, n, its[0], its[1], res);
    for (int e = 0; e < n; e++) {
        const int j = corrs[e].index1;
        if (!dead[e] && j >= 0 && j < n1cap) keep[j] = 1;
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s <in> <out> [repeat]\n", argv[0]);
        return 2;
    }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[4];
    if (!f || fread(hd, 4, 4, f) != 4) return 1;
    const int np = hd[0], cap = hd[1], n1cap = hd[2];
    if (np < 0 || cap < 1 || cap > ORBG_SIM3OPT_MAX_N || n1cap < 1) return 1;
    std::vector<orbg_sim3opt_problem> probs(np);
    std::vector<orbg_sim3opt_corr> corrs((size_t)np * cap);
    std::vector<orbg_sim3_hyp> init(np);
    if (fread(probs.data(), sizeof(probs[0]), np, f) != (size_t)np ||
        fread(corrs.data(), sizeof(corrs[0]), corrs.size(), f) != corrs.size() ||
        fread(init.data(), sizeof(init[0]), np, f) != (size_t)np)
        return 1;
    fclose(f);
    std::vector<orbg_sim3opt_result> res(np);
    std::vector<uint8_t> keep((size_t)np * n1cap);
    memset(res.data(), 0, res.size() * sizeof(res[0]));
    double best = 1e300;
    for (int r = 0; r < (repeat > 0 ? repeat : 1); r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < np; p++)
            optimize_one(probs[p], &corrs[(size_t)p * cap], init[p], cap, n1cap, &res[p],
                         &keep[(size_t)p * n1cap]);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dt < best) best = dt;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(res.data(), sizeof(res[0]), np, f);
    fwrite(keep.data(), 1, keep.size(), f);
    fclose(f);
    printf("%.9f\n", best);
    return 0;
}
