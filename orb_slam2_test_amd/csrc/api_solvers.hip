// api_solvers.hip -- Sim3Solver, PnPsolver, OptimizeSim3
#include "orbg_ctx.h"
#include "sim3_args.h"
#include "sim3opt_args.h"
#include "pnp_args.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// Sim3Solver: batched RANSAC of LoopClosing::ComputeSim3 (sim3_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_sim3_ransac_iterations(double prob, int min_inliers, int max_its, int n)
{
    // Sim3Solver::SetRansacParameters (:114-138), type for type
    const float epsilon = (float)min_inliers / n;
    int nit;
    if (min_inliers == n) {
        nit = 1;
    } else {
        // a quotient that is NaN or outside int (n < min_inliers, a tiny epsilon) converts to
        // INT_MIN in the reference's x86-64 build, so mRansacMaxIts ends as 1
        const double v = ceil(log(1 - prob) / log(1 - pow(epsilon, 3)));
        nit = (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT32_MIN;
    }
    return std::max(1, std::min(nit, max_its));
}

// the prepared-correspondence arrays of `pairs` pairs at `b`
static size_t sim3_prep_bytes(size_t pairs, size_t cap) { return 3 * al256(pairs * cap * sizeof(float4)); }
static Sim3Prep sim3_prep_at(uint8_t *b, size_t pairs, size_t cap)
{
    const size_t one = al256(pairs * cap * sizeof(float4));
    return Sim3Prep{(float4 *)b, (float4 *)(b + one), (float4 *)(b + 2 * one)};
}

extern "C" int orbg_sim3_solve_batch_device(orbg_ctx *c, const orbg_sim3_problem *d_problems,
                                            const orbg_sim3_corr *d_corrs, const int32_t *d_samples,
                                            int npairs, int cap, int max_its, int32_t *d_counts,
                                            orbg_sim3_hyp *d_hyps, uint64_t *d_masks,
                                            orbg_sim3_result *d_results, uint8_t *d_inliers12,
                                            int n1cap)
{
    if (!c) return set_err(ORBG_EINVAL, "context is NULL");
    if (npairs < 0 || cap < 64 || (cap & 63) || max_its < 1 || n1cap < 1)
        return set_err(ORBG_EINVAL, "bad npairs / cap (a multiple of 64) / max_its / n1cap");
    if (cap > ORBG_SIM3_MAX_N)
        return set_err(ORBG_ENOTSUP, "cap %d (> %d correspondences per pair)", cap, ORBG_SIM3_MAX_N);
    if (npairs == 0) return ORBG_OK;
    if ((int64_t)npairs * ((max_its + 3) / 4) > INT32_MAX)
        return set_err(ORBG_ENOTSUP, "npairs * max_its too large for one launch");
    if (!d_problems || !d_corrs || !d_samples || !d_counts || !d_hyps || !d_masks || !d_results ||
        !d_inliers12)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    void *s;
    int rc = scratch(c, sim3_prep_bytes(npairs, cap), &s);
    if (rc) return rc;
    Sim3Args A{};
    A.problems = d_problems;
    A.corrs = d_corrs;
    A.samples = d_samples;
    A.npairs = npairs;
    A.cap = cap;
    A.max_its = max_its;
    A.n1cap = n1cap;
    A.prep = sim3_prep_at((uint8_t *)s, npairs, cap);
    A.counts = d_counts;
    A.hyps = d_hyps;
    A.masks = (unsigned long long *)d_masks;
    A.results = d_results;
    A.inliers12 = d_inliers12;
    if ((rc = launch_sim3(c->stream, A, &c->prof))) return set_err(rc, "Sim3Solver launch failed");
    return ORBG_OK;
}

extern "C" int orbg_sim3_solve(orbg_ctx *c, const orbg_sim3_problem *problem,
                               const orbg_sim3_corr *corrs, const int32_t *samples, int n1,
                               int32_t *counts, orbg_sim3_hyp *hyps, uint64_t *masks,
                               orbg_sim3_result *result, uint8_t *inliers12)
{
    if (!c || !problem || !result) return set_err(ORBG_EINVAL, "NULL argument");
    const orbg_sim3_problem P = *problem;
    if (P.n < 0 || P.iterations < 0 || n1 < 0) return set_err(ORBG_EINVAL, "negative size");
    if (P.n > ORBG_SIM3_MAX_N)
        return set_err(ORBG_ENOTSUP, "%d correspondences (> %d)", P.n, ORBG_SIM3_MAX_N);
    if (P.iterations > (1 << 20)) return set_err(ORBG_ENOTSUP, "%d iterations", P.iterations);
    if ((P.n && !corrs) || (n1 && !inliers12)) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < P.n; i++)
        if (corrs[i].index1 < 0 || corrs[i].index1 >= n1)
            return set_err(ORBG_EINVAL, "index1 %d of correspondence %d outside [0, %d)",
                           corrs[i].index1, i, n1);
    const int cap = std::max(64, (P.n + 63) & ~63), its = std::max(P.iterations, 1);
    const int run = sim3_iterations(P, cap, its), words = cap / 64;
    if (run && !samples) return set_err(ORBG_EINVAL, "samples is NULL");
    for (int it = 0; it < run; it++) {
        const int32_t *s = samples + 3 * (size_t)it;
        for (int k = 0; k < 3; k++)
            if (s[k] < 0 || s[k] >= P.n)
                return set_err(ORBG_EINVAL, "sample %d of iteration %d outside [0, %d)", s[k], it, P.n);
        if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2])
            return set_err(ORBG_EINVAL, "iteration %d repeats a sample index", it);
    }
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_p = L.take(sizeof(P)), o_k = L.take((size_t)cap * sizeof(orbg_sim3_corr));
    const size_t o_s = L.take((size_t)its * 12), o_c = L.take((size_t)its * 4);
    const size_t o_h = L.take((size_t)its * sizeof(orbg_sim3_hyp));
    const size_t o_m = L.take((size_t)its * words * 8), o_r = L.take(sizeof(orbg_sim3_result));
    const size_t o_i = L.take((size_t)std::max(n1, 1)), o_x = L.take(sim3_prep_bytes(1, cap));
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b + o_p, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    if (P.n) HIPCHK(hipMemcpyAsync(b + o_k, corrs, (size_t)P.n * sizeof(orbg_sim3_corr), hipMemcpyHostToDevice, c->stream));
    if (run) HIPCHK(hipMemcpyAsync(b + o_s, samples, (size_t)run * 12, hipMemcpyHostToDevice, c->stream));
    Sim3Args A{};
    A.problems = L.at<orbg_sim3_problem>(b, o_p);
    A.corrs = L.at<orbg_sim3_corr>(b, o_k);
    A.samples = L.at<int32_t>(b, o_s);
    A.npairs = 1;
    A.cap = cap;
    A.max_its = its;
    A.n1cap = std::max(n1, 1);
    A.prep = sim3_prep_at(b + o_x, 1, cap);
    A.counts = L.at<int32_t>(b, o_c);
    A.hyps = L.at<orbg_sim3_hyp>(b, o_h);
    A.masks = L.at<unsigned long long>(b, o_m);
    A.results = L.at<orbg_sim3_result>(b, o_r);
    A.inliers12 = b + o_i;
    if ((rc = launch_sim3(c->stream, A, &c->prof))) return set_err(rc, "Sim3Solver launch failed");
    const int nout = P.iterations, nw = (P.n + 63) / 64;
    if (counts && nout) HIPCHK(hipMemcpyAsync(counts, b + o_c, (size_t)nout * 4, hipMemcpyDeviceToHost, c->stream));
    if (hyps && nout) HIPCHK(hipMemcpyAsync(hyps, b + o_h, (size_t)nout * sizeof(orbg_sim3_hyp), hipMemcpyDeviceToHost, c->stream));
    if (masks && nout && nw)
        HIPCHK(hipMemcpy2DAsync(masks, (size_t)nw * 8, b + o_m, (size_t)words * 8, (size_t)nw * 8, nout,
                                hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(result, b + o_r, sizeof(orbg_sim3_result), hipMemcpyDeviceToHost, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(inliers12, b + o_i, (size_t)n1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// PnPsolver: batched EPnP RANSAC of Tracking::Relocalization (pnp_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_pnp_ransac_parameters(double prob, int min_inliers, int max_its, int min_set,
                                          float epsilon, int n, int *min_inliers_out,
                                          int *iterations_out)
{
    if (n < 1) return set_err(ORBG_EINVAL, "PnPsolver: n %d < 1", n);
    if (!min_inliers_out || !iterations_out) return set_err(ORBG_EINVAL, "NULL output");
    // PnPsolver::SetRansacParameters (:121-152), type for type
    const float fn = (float)n * epsilon;  // int * float
    int nmin = (fn > -2147483904.0f && fn < 2147483648.0f) ? (int)fn : INT32_MIN;
    if (nmin < min_inliers) nmin = min_inliers;
    if (nmin < min_set) nmin = min_set;
    if (epsilon < (float)nmin / n) epsilon = (float)nmin / n;
    int nit;
    if (nmin == n) {
        nit = 1;
    } else {
        // a quotient that is NaN or outside int converts to INT_MIN in the reference's x86-64
        // build, so mRansacMaxIts ends as 1
        const double v = ceil(log(1 - prob) / log(1 - pow(epsilon, 3)));
        nit = (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT32_MIN;
    }
    *min_inliers_out = nmin;
    *iterations_out = std::max(1, std::min(nit, max_its));
    return ORBG_OK;
}

extern "C" int orbg_pnp_solve_batch_device(orbg_ctx *c, const orbg_pnp_problem *d_problems,
                                           const orbg_pnp_corr *d_corrs, const int32_t *d_samples,
                                           int ncand, int cap, int max_its, int32_t *d_counts,
                                           orbg_pnp_hyp *d_hyps, uint64_t *d_masks,
                                           orbg_pnp_refine *d_refines, uint64_t *d_refined_masks,
                                           orbg_pnp_result *d_results, uint8_t *d_inliers, int n1cap)
{
    if (!c) return set_err(ORBG_EINVAL, "context is NULL");
    if (ncand < 0 || cap < 64 || (cap & 63) || max_its < 1 || n1cap < 1)
        return set_err(ORBG_EINVAL, "bad ncand / cap (a multiple of 64) / max_its / n1cap");
    if (cap > ORBG_PNP_MAX_N)
        return set_err(ORBG_ENOTSUP, "cap %d (> %d correspondences per candidate)", cap, ORBG_PNP_MAX_N);
    if (ncand == 0) return ORBG_OK;
    if ((int64_t)ncand * max_its > INT32_MAX)
        return set_err(ORBG_ENOTSUP, "ncand * max_its too large for one launch");
    if (!d_problems || !d_corrs || !d_samples || !d_counts || !d_hyps || !d_masks || !d_refines ||
        !d_refined_masks || !d_results || !d_inliers)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    PnpArgs A{};
    A.problems = d_problems;
    A.corrs = d_corrs;
    A.samples = d_samples;
    A.ncand = ncand;
    A.cap = cap;
    A.max_its = max_its;
    A.n1cap = n1cap;
    A.counts = d_counts;
    A.hyps = d_hyps;
    A.masks = (unsigned long long *)d_masks;
    A.refines = d_refines;
    A.refined_masks = (unsigned long long *)d_refined_masks;
    A.results = d_results;
    A.inliers = d_inliers;
    int rc;
    if ((rc = launch_pnp(c->stream, A, &c->prof))) return set_err(rc, "PnPsolver launch failed");
    return ORBG_OK;
}

extern "C" int orbg_pnp_solve(orbg_ctx *c, const orbg_pnp_problem *problem, const orbg_pnp_corr *corrs,
                              const int32_t *samples, int n1, int32_t *counts, orbg_pnp_hyp *hyps,
                              uint64_t *masks, orbg_pnp_refine *refines, uint64_t *refined_masks,
                              orbg_pnp_result *result, uint8_t *inliers)
{
    if (!c || !problem || !result) return set_err(ORBG_EINVAL, "NULL argument");
    const orbg_pnp_problem P = *problem;
    if (P.n < 0 || P.iterations < 0 || n1 < 0) return set_err(ORBG_EINVAL, "negative size");
    if (P.min_set < 4 || P.min_set > ORBG_PNP_MAX_SET)
        return set_err(ORBG_EINVAL, "min_set %d outside 4 .. %d", P.min_set, ORBG_PNP_MAX_SET);
    if (P.n > ORBG_PNP_MAX_N)
        return set_err(ORBG_ENOTSUP, "%d correspondences (> %d)", P.n, ORBG_PNP_MAX_N);
    if (P.iterations > (1 << 20)) return set_err(ORBG_ENOTSUP, "%d iterations", P.iterations);
    if ((P.n && !corrs) || (n1 && !inliers)) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < P.n; i++)
        if (corrs[i].index < 0 || corrs[i].index >= n1)
            return set_err(ORBG_EINVAL, "index %d of correspondence %d outside [0, %d)",
                           corrs[i].index, i, n1);
    const int cap = std::max(64, (P.n + 63) & ~63), its = std::max(P.iterations, 1);
    const int run = pnp_iterations(P, cap, its), words = cap / 64, m = P.min_set;
    if (run && !samples) return set_err(ORBG_EINVAL, "samples is NULL");
    std::vector<int32_t> padded((size_t)its * ORBG_PNP_MAX_SET, 0);
    for (int it = 0; it < run; it++) {
        const int32_t *s = samples + (size_t)m * it;
        for (int k = 0; k < m; k++) {
            if (s[k] < 0 || s[k] >= P.n)
                return set_err(ORBG_EINVAL, "sample %d of iteration %d outside [0, %d)", s[k], it, P.n);
            for (int j = 0; j < k; j++)
                if (s[j] == s[k]) return set_err(ORBG_EINVAL, "iteration %d repeats a sample index", it);
            padded[(size_t)it * ORBG_PNP_MAX_SET + k] = s[k];
        }
    }
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_p = L.take(sizeof(P)), o_k = L.take((size_t)cap * sizeof(orbg_pnp_corr));
    const size_t o_s = L.take(padded.size() * 4), o_c = L.take((size_t)its * 4);
    const size_t o_h = L.take((size_t)its * sizeof(orbg_pnp_hyp));
    const size_t o_m = L.take((size_t)its * words * 8);
    const size_t o_f = L.take((size_t)its * sizeof(orbg_pnp_refine));
    const size_t o_g = L.take((size_t)its * words * 8), o_r = L.take(sizeof(orbg_pnp_result));
    const size_t o_i = L.take((size_t)std::max(n1, 1));
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b + o_p, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    if (P.n) HIPCHK(hipMemcpyAsync(b + o_k, corrs, (size_t)P.n * sizeof(orbg_pnp_corr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_s, padded.data(), padded.size() * 4, hipMemcpyHostToDevice, c->stream));
    PnpArgs A{};
    A.problems = L.at<orbg_pnp_problem>(b, o_p);
    A.corrs = L.at<orbg_pnp_corr>(b, o_k);
    A.samples = L.at<int32_t>(b, o_s);
    A.ncand = 1;
    A.cap = cap;
    A.max_its = its;
    A.n1cap = std::max(n1, 1);
    A.counts = L.at<int32_t>(b, o_c);
    A.hyps = L.at<orbg_pnp_hyp>(b, o_h);
    A.masks = L.at<unsigned long long>(b, o_m);
    A.refines = L.at<orbg_pnp_refine>(b, o_f);
    A.refined_masks = L.at<unsigned long long>(b, o_g);
    A.results = L.at<orbg_pnp_result>(b, o_r);
    A.inliers = b + o_i;
    if ((rc = launch_pnp(c->stream, A, &c->prof))) return set_err(rc, "PnPsolver launch failed");
    const int nout = P.iterations, nw = (P.n + 63) / 64;
    if (counts && nout) HIPCHK(hipMemcpyAsync(counts, b + o_c, (size_t)nout * 4, hipMemcpyDeviceToHost, c->stream));
    if (hyps && nout) HIPCHK(hipMemcpyAsync(hyps, b + o_h, (size_t)nout * sizeof(orbg_pnp_hyp), hipMemcpyDeviceToHost, c->stream));
    if (refines && nout) HIPCHK(hipMemcpyAsync(refines, b + o_f, (size_t)nout * sizeof(orbg_pnp_refine), hipMemcpyDeviceToHost, c->stream));
    if (masks && nout && nw)
        HIPCHK(hipMemcpy2DAsync(masks, (size_t)nw * 8, b + o_m, (size_t)words * 8, (size_t)nw * 8, nout,
                                hipMemcpyDeviceToHost, c->stream));
    if (refined_masks && nout && nw)
        HIPCHK(hipMemcpy2DAsync(refined_masks, (size_t)nw * 8, b + o_g, (size_t)words * 8, (size_t)nw * 8,
                                nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(result, b + o_r, sizeof(orbg_pnp_result), hipMemcpyDeviceToHost, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(inliers, b + o_i, (size_t)n1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// Optimizer::OptimizeSim3: batched Sim3 refinement of loop candidates (sim3opt_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_optimize_sim3_batch_device(orbg_ctx *c, const orbg_sim3opt_problem *d_problems,
                                               const orbg_sim3opt_corr *d_corrs,
                                               const orbg_sim3_hyp *d_init, int npairs, int cap,
                                               orbg_sim3opt_result *d_results, uint8_t *d_keep,
                                               int n1cap)
{
    if (!c) return set_err(ORBG_EINVAL, "context is NULL");
    if (npairs < 0 || cap < 64 || (cap & 63) || n1cap < 1)
        return set_err(ORBG_EINVAL, "bad npairs / cap (a multiple of 64) / n1cap");
    if (cap > ORBG_SIM3OPT_MAX_N)
        return set_err(ORBG_ENOTSUP, "cap %d (> %d correspondences per candidate)", cap,
                       ORBG_SIM3OPT_MAX_N);
    if (npairs == 0) return ORBG_OK;
    if (!d_problems || !d_corrs || !d_init || !d_results || !d_keep)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    Sim3OptArgs A{};
    A.problems = d_problems;
    A.corrs = d_corrs;
    A.init = d_init;
    A.npairs = npairs;
    A.cap = cap;
    A.n1cap = n1cap;
    A.results = d_results;
    A.keep = d_keep;
    int rc;
    if ((rc = launch_sim3opt(c->stream, A, &c->prof))) return set_err(rc, "OptimizeSim3 launch failed");
    return ORBG_OK;
}

extern "C" int orbg_optimize_sim3(orbg_ctx *c, const orbg_sim3opt_problem *problem,
                                  const orbg_sim3opt_corr *corrs, const orbg_sim3_hyp *init, int n1,
                                  orbg_sim3opt_result *result, uint8_t *keep)
{
    if (!c || !problem || !init || !result) return set_err(ORBG_EINVAL, "NULL argument");
    const orbg_sim3opt_problem P = *problem;
    if (P.n < 0 || n1 < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!(P.th2 > 0.0f) || !(P.th2 <= FLT_MAX))
        return set_err(ORBG_EINVAL, "th2 %g is not finite and positive", (double)P.th2);
    if (P.n > ORBG_SIM3OPT_MAX_N)
        return set_err(ORBG_ENOTSUP, "%d correspondences (> %d)", P.n, ORBG_SIM3OPT_MAX_N);
    if ((P.n && !corrs) || (n1 && !keep)) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < P.n; i++)
        if (corrs[i].index1 < 0 || corrs[i].index1 >= n1)
            return set_err(ORBG_EINVAL, "index1 %d of correspondence %d outside [0, %d)",
                           corrs[i].index1, i, n1);
    const int cap = std::max(64, (P.n + 63) & ~63);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_p = L.take(sizeof(P)), o_k = L.take((size_t)cap * sizeof(orbg_sim3opt_corr));
    const size_t o_h = L.take(sizeof(orbg_sim3_hyp)), o_r = L.take(sizeof(orbg_sim3opt_result));
    const size_t o_i = L.take((size_t)std::max(n1, 1));
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b + o_p, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    if (P.n) HIPCHK(hipMemcpyAsync(b + o_k, corrs, (size_t)P.n * sizeof(orbg_sim3opt_corr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_h, init, sizeof(orbg_sim3_hyp), hipMemcpyHostToDevice, c->stream));
    Sim3OptArgs A{};
    A.problems = L.at<orbg_sim3opt_problem>(b, o_p);
    A.corrs = L.at<orbg_sim3opt_corr>(b, o_k);
    A.init = L.at<orbg_sim3_hyp>(b, o_h);
    A.npairs = 1;
    A.cap = cap;
    A.n1cap = std::max(n1, 1);
    A.results = L.at<orbg_sim3opt_result>(b, o_r);
    A.keep = b + o_i;
    if ((rc = launch_sim3opt(c->stream, A, &c->prof))) return set_err(rc, "OptimizeSim3 launch failed");
    HIPCHK(hipMemcpyAsync(result, b + o_r, sizeof(orbg_sim3opt_result), hipMemcpyDeviceToHost, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(keep, b + o_i, (size_t)n1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}
