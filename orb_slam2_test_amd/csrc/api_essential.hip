// api_essential.hip -- Optimizer::OptimizeEssentialGraph: the host plan of a graph (elimination
// order, block pattern of L, summation lists), the LM loop and the entry points
// (essential_kernels.hip has the kernels)
#include "orbg_ctx.h"
#include "essential_args.h"

#include <set>

#pragma clang fp contract(off)

using namespace orbg;

static_assert(sizeof(orbg_sim3d) == sizeof(Sim3d) && sizeof(Sim3d) == 64, "orbg_sim3d is Sim3d");

struct orbg_eg_graph {
    int device = 0;
    int nvert = 0, nedge = 0, fixed = 0, nfree = 0, hblocks = 0, lblocks = 0;
    uint8_t *d_plan = nullptr, *d_work = nullptr;
    EgPlan P{};
    EgWork W{};
    Sim3d *d_backup = nullptr;  // [nvert]: the estimates a trial may have to restore
};

static int eg_check(const orbg_eg_edge *edges, int nedge, int nvert, int fixed)
{
    if (nvert < 1 || nedge < 0) return set_err(ORBG_EINVAL, "nvert %d / nedge %d", nvert, nedge);
    if (nedge && !edges) return set_err(ORBG_EINVAL, "edges is NULL");
    if (fixed < 0 || fixed >= nvert)
        return set_err(ORBG_EINVAL, "fixed_vertex %d outside [0, %d)", fixed, nvert);
    for (int e = 0; e < nedge; e++) {
        const orbg_eg_edge &d = edges[e];
        if (d.i < 0 || d.i >= nvert || d.j < 0 || d.j >= nvert)
            return set_err(ORBG_EINVAL, "edge %d: vertex outside [0, %d)", e, nvert);
        if (d.i == d.j) return set_err(ORBG_EINVAL, "edge %d joins vertex %d to itself", e, d.i);
        if (d.kind != 0 && d.kind != 1) return set_err(ORBG_EINVAL, "edge %d: kind %d", e, d.kind);
    }
    if (nedge > ORBG_EG_MAX_EDGES) return set_err(ORBG_ENOTSUP, "%d edges (> %d)", nedge, ORBG_EG_MAX_EDGES);
    return ORBG_OK;
}

// the plan's host arrays
struct EgPlanHost {
    std::vector<int32_t> vfree, colptr, rowidx, coff, clist, boff, blist, upoff, rowoff;
    std::vector<int4> up;
    std::vector<int2> row;
    int nfree = 0, hblocks = 0, lblocks = 0;
};

// Symbolic elimination of the free vertices' graph in minimum-degree order (the smallest
// vertex index among those of least degree: deterministic), then every list the kernels walk.
static int eg_plan(const orbg_eg_edge *edges, int nedge, int nvert, int fixed, EgPlanHost &H)
{
    std::vector<std::set<int>> adj(nvert);
    int64_t npair = 0;
    for (int e = 0; e < nedge; e++) {
        const int i = edges[e].i, j = edges[e].j;
        if (i == fixed || j == fixed) continue;
        if (adj[i].insert(j).second) {
            adj[j].insert(i);
            npair++;
        }
    }
    H.nfree = nvert - 1;
    if (npair + H.nfree > ORBG_EG_MAX_BLOCKS)
        return set_err(ORBG_ENOTSUP, "%lld blocks of H (> %d)", (long long)(npair + H.nfree),
                       ORBG_EG_MAX_BLOCKS);
    H.hblocks = (int)npair + H.nfree;
    std::set<std::pair<int, int>> queue;  // (degree, vertex)
    for (int v = 0; v < nvert; v++)
        if (v != fixed) queue.insert({(int)adj[v].size(), v});
    std::vector<int> order;
    std::vector<std::vector<int>> below(nvert);  // column v's rows, as vertices
    H.vfree.assign(nvert, -1);
    int64_t lblocks = 0;
    while (!queue.empty()) {
        const int v = queue.begin()->second;
        queue.erase(queue.begin());
        H.vfree[v] = (int)order.size();
        order.push_back(v);
        std::vector<int> nb(adj[v].begin(), adj[v].end());
        lblocks += 1 + (int64_t)nb.size();
        if (lblocks > ORBG_EG_MAX_BLOCKS)
            return set_err(ORBG_ENOTSUP, "more than %d blocks of L", ORBG_EG_MAX_BLOCKS);
        for (int a : nb) {
            queue.erase({(int)adj[a].size(), a});
            adj[a].erase(v);
        }
        for (size_t x = 0; x < nb.size(); x++)
            for (size_t y = x + 1; y < nb.size(); y++)
                if (adj[nb[x]].insert(nb[y]).second) adj[nb[y]].insert(nb[x]);
        for (int a : nb) queue.insert({(int)adj[a].size(), a});
        below[v] = std::move(nb);
        adj[v].clear();
    }
    H.lblocks = (int)lblocks;
    const int n = H.nfree;
    // L by columns (rows ascending, the diagonal first) and by rows (columns ascending)
    H.colptr.assign(n + 1, 0);
    H.rowidx.clear();
    std::vector<std::vector<int2>> rows(n);
    for (int p = 0; p < n; p++) {
        std::vector<int> r;
        for (int a : below[order[p]]) r.push_back(H.vfree[a]);
        std::sort(r.begin(), r.end());
        H.rowidx.push_back(p);
        for (int q : r) {
            rows[q].push_back(int2{(int)H.rowidx.size(), p});
            H.rowidx.push_back(q);
        }
        H.colptr[p + 1] = (int)H.rowidx.size();
    }
    H.rowoff.assign(n + 1, 0);
    H.row.clear();
    for (int p = 0; p < n; p++) {
        H.row.insert(H.row.end(), rows[p].begin(), rows[p].end());
        H.rowoff[p + 1] = (int)H.row.size();
    }
    auto slot = [&](int r, int c) {  // (r, c), r >= c: present by construction
        const int32_t *b = H.rowidx.data() + H.colptr[c], *e = H.rowidx.data() + H.colptr[c + 1];
        return (int)(std::lower_bound(b, e, r) - H.rowidx.data());
    };
    // block (r, j) -= L(r, k) D(k) L(j, k)^T over the columns k both rows have
    H.upoff.assign((size_t)H.lblocks + 1, 0);
    H.up.clear();
    for (int j = 0; j < n; j++)
        for (int s = H.colptr[j]; s < H.colptr[j + 1]; s++) {
            const int r = H.rowidx[s];
            const std::vector<int2> &a = rows[r], &b = rows[j];
            size_t x = 0, y = 0;
            while (x < a.size() && y < b.size() && a[x].y < j && b[y].y < j) {
                if (a[x].y < b[y].y) x++;
                else if (a[x].y > b[y].y) y++;
                else {
                    H.up.push_back(int4{a[x].x, b[y].x, a[x].y, 0});
                    x++;
                    y++;
                }
            }
            if (H.up.size() > (size_t)ORBG_EG_MAX_UPDATES)
                return set_err(ORBG_ENOTSUP, "more than %d block updates in the factorisation",
                               ORBG_EG_MAX_UPDATES);
            H.upoff[s + 1] = (int)H.up.size();
        }
    // contributions to H's blocks and b's segments, in edge order
    std::vector<std::vector<int32_t>> cl(H.lblocks), bl(n);
    for (int e = 0; e < nedge; e++) {
        const int pi = H.vfree[edges[e].i], pj = H.vfree[edges[e].j];
        if (pi >= 0) {
            cl[H.colptr[pi]].push_back(e * 4 + 0);
            bl[pi].push_back(e * 2 + 0);
        }
        if (pj >= 0) {
            cl[H.colptr[pj]].push_back(e * 4 + 1);
            bl[pj].push_back(e * 2 + 1);
        }
        if (pi >= 0 && pj >= 0) {
            if (pi > pj) cl[slot(pi, pj)].push_back(e * 4 + 2);  // J_r^T J_c with r = i: Ji^T Jj
            else cl[slot(pj, pi)].push_back(e * 4 + 3);          // r = j: its transpose
        }
    }
    H.coff.assign((size_t)H.lblocks + 1, 0);
    H.clist.clear();
    for (int s = 0; s < H.lblocks; s++) {
        H.clist.insert(H.clist.end(), cl[s].begin(), cl[s].end());
        H.coff[s + 1] = (int)H.clist.size();
    }
    H.boff.assign(n + 1, 0);
    H.blist.clear();
    for (int p = 0; p < n; p++) {
        H.blist.insert(H.blist.end(), bl[p].begin(), bl[p].end());
        H.boff[p + 1] = (int)H.blist.size();
    }
    return ORBG_OK;
}

extern "C" int orbg_eg_graph_destroy(orbg_eg_graph *g)
{
    if (!g) return ORBG_OK;
    hipSetDevice(g->device);
    if (g->d_plan) hipFree(g->d_plan);
    if (g->d_work) hipFree(g->d_work);
    delete g;
    return ORBG_OK;
}

extern "C" int orbg_eg_graph_create(orbg_ctx *c, const orbg_eg_edge *edges, int nedge, int nvert,
                                    int fixed, orbg_eg_graph **out)
{
    if (!c || !out) return set_err(ORBG_EINVAL, "ctx / out is NULL");
    int rc = eg_check(edges, nedge, nvert, fixed);
    if (rc) return rc;
    EgPlanHost H;
    if ((rc = eg_plan(edges, nedge, nvert, fixed, H))) return rc;
    HIPCHK(hipSetDevice(c->device));
    orbg_eg_graph *g = new orbg_eg_graph;
    g->device = c->device;
    g->nvert = nvert;
    g->nedge = nedge;
    g->fixed = fixed;
    g->nfree = H.nfree;
    g->hblocks = H.hblocks;
    g->lblocks = H.lblocks;
    const size_t n = (size_t)H.nfree, nv = (size_t)nvert, ne = (size_t)nedge, nl = (size_t)H.lblocks;
    Layout L;
    const size_t o_e = L.take(ne * sizeof(orbg_eg_edge)), o_vf = L.take(nv * 4),
                 o_cp = L.take((n + 1) * 4), o_ri = L.take(nl * 4), o_co = L.take((nl + 1) * 4),
                 o_cl = L.take(H.clist.size() * 4), o_bo = L.take((n + 1) * 4),
                 o_bl = L.take(H.blist.size() * 4), o_uo = L.take((nl + 1) * 4),
                 o_up = L.take(H.up.size() * sizeof(int4)), o_ro = L.take((n + 1) * 4),
                 o_rw = L.take(H.row.size() * sizeof(int2));
    Layout K;
    const size_t w_m = K.take(ne * sizeof(Sim3d)), w_ei = K.take(nv * sizeof(Sim3d)),
                 w_p = K.take(nv * EG_NP * sizeof(Sim3d)), w_pi = K.take(nv * EG_NP * sizeof(Sim3d)),
                 w_eo = K.take(ne * EG_EO * 8), w_a = K.take(nl * 49 * 8), w_l = K.take(nl * 49 * 8),
                 w_d = K.take(n * 7 * 8), w_b = K.take(n * 7 * 8), w_y = K.take(n * 7 * 8),
                 w_x = K.take(n * 7 * 8), w_pt = K.take(EG_RG * 8), w_sc = K.take(4 * 8),
                 w_bk = K.take(nv * sizeof(Sim3d));
    if (hipMalloc((void **)&g->d_plan, L.total()) != hipSuccess ||
        hipMalloc((void **)&g->d_work, K.total()) != hipSuccess) {
        orbg_eg_graph_destroy(g);
        return set_err(ORBG_ENOMEM, "essential graph: %zu + %zu bytes", L.total(), K.total());
    }
    uint8_t *b = g->d_plan;
    hipStream_t st = c->stream;
    auto up = [&](size_t off, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(b + off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    hipError_t e = up(o_e, edges, ne * sizeof(orbg_eg_edge));
    if (e == hipSuccess) e = up(o_vf, H.vfree.data(), nv * 4);
    if (e == hipSuccess) e = up(o_cp, H.colptr.data(), (n + 1) * 4);
    if (e == hipSuccess) e = up(o_ri, H.rowidx.data(), nl * 4);
    if (e == hipSuccess) e = up(o_co, H.coff.data(), (nl + 1) * 4);
    if (e == hipSuccess) e = up(o_cl, H.clist.data(), H.clist.size() * 4);
    if (e == hipSuccess) e = up(o_bo, H.boff.data(), (n + 1) * 4);
    if (e == hipSuccess) e = up(o_bl, H.blist.data(), H.blist.size() * 4);
    if (e == hipSuccess) e = up(o_uo, H.upoff.data(), (nl + 1) * 4);
    if (e == hipSuccess) e = up(o_up, H.up.data(), H.up.size() * sizeof(int4));
    if (e == hipSuccess) e = up(o_ro, H.rowoff.data(), (n + 1) * 4);
    if (e == hipSuccess) e = up(o_rw, H.row.data(), H.row.size() * sizeof(int2));
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the plan's host arrays die here
    if (e != hipSuccess) {
        orbg_eg_graph_destroy(g);
        return set_err(ORBG_EIO, "essential graph upload: %s", hipGetErrorString(e));
    }
    EgPlan &P = g->P;
    P.nvert = nvert;
    P.nedge = nedge;
    P.nfree = H.nfree;
    P.lblocks = H.lblocks;
    P.edges = L.at<orbg_eg_edge>(b, o_e);
    P.vfree = L.at<int32_t>(b, o_vf);
    P.colptr = L.at<int32_t>(b, o_cp);
    P.rowidx = L.at<int32_t>(b, o_ri);
    P.coff = L.at<int32_t>(b, o_co);
    P.clist = L.at<int32_t>(b, o_cl);
    P.boff = L.at<int32_t>(b, o_bo);
    P.blist = L.at<int32_t>(b, o_bl);
    P.upoff = L.at<int32_t>(b, o_uo);
    P.up = L.at<int4>(b, o_up);
    P.rowoff = L.at<int32_t>(b, o_ro);
    P.row = L.at<int2>(b, o_rw);
    uint8_t *w = g->d_work;
    EgWork &W = g->W;
    W.meas = K.at<Sim3d>(w, w_m);
    W.estinv = K.at<Sim3d>(w, w_ei);
    W.P = K.at<Sim3d>(w, w_p);
    W.Pinv = K.at<Sim3d>(w, w_pi);
    W.eo = K.at<double>(w, w_eo);
    W.A = K.at<double>(w, w_a);
    W.L = K.at<double>(w, w_l);
    W.D = K.at<double>(w, w_d);
    W.b = K.at<double>(w, w_b);
    W.y = K.at<double>(w, w_y);
    W.x = K.at<double>(w, w_x);
    W.part = K.at<double>(w, w_pt);
    W.sc = K.at<double>(w, w_sc);
    g->d_backup = K.at<Sim3d>(w, w_bk);
    *out = g;
    return ORBG_OK;
}

extern "C" int orbg_eg_graph_info(const orbg_eg_graph *g, int32_t *nfree, int32_t *h_blocks,
                                  int32_t *l_blocks)
{
    if (!g) return set_err(ORBG_EINVAL, "graph is NULL");
    if (nfree) *nfree = g->nfree;
    if (h_blocks) *h_blocks = g->hblocks;
    if (l_blocks) *l_blocks = g->lblocks;
    return ORBG_OK;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg under
// setUserLambdaInit(1e-16), the estimates in HBM (see include/orbg.h)
extern "C" int orbg_eg_graph_optimize(orbg_ctx *c, orbg_eg_graph *g, const orbg_sim3d *d_Scw,
                                      const orbg_sim3d *d_Snc, int fix_scale, int iterations,
                                      orbg_sim3d *d_Siw_out, float *d_Tiw_out, orbg_lm_report *rep)
{
    if (!c || !g) return set_err(ORBG_EINVAL, "ctx / graph is NULL");
    if (g->device != c->device) return set_err(ORBG_EINVAL, "graph of another device");
    if (!d_Scw || !d_Snc || !d_Siw_out) return set_err(ORBG_EINVAL, "NULL device array");
    if (iterations < 0) return set_err(ORBG_EINVAL, "negative iterations");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const EgPlan &P = g->P;
    const EgWork &W = g->W;
    Sim3d *est = (Sim3d *)d_Siw_out;
    const size_t vbytes = (size_t)g->nvert * sizeof(Sim3d);
    if ((const void *)d_Scw != (const void *)d_Siw_out)
        HIPCHK(hipMemcpyAsync(est, d_Scw, vbytes, hipMemcpyDeviceToDevice, st));
    orbg_lm_report R{};
    int rc;
    auto fail = [&](const char *what) { return set_err(ORBG_EIO, "essential graph: %s launch failed", what); };
    auto read = [&](double *h, int n) -> int {
        HIPCHK(hipMemcpyAsync(h, W.sc, n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return ORBG_OK;
    };
    if (g->nfree > 0 && g->nedge > 0 && iterations > 0) {
        if (launch_eg_measure(st, P, (const Sim3d *)d_Scw, (const Sim3d *)d_Snc, W.meas)) return fail("k_eg_measure");
        LmState lm = {0, 2, 0, 0, 0, 0};  // the step control is g2o_math.h's
        double hs[4] = {0, 0, 0, 0};      // chi2, computeScale, -, the solver's ok
        for (int it = 0; it < iterations; it++) {
            if (it == 0) {  // computeActiveErrors at the start (later: the last accepted trial's)
                if (launch_eg_errors(st, P, W, est, W.sc, &c->prof)) return fail("k_eg_errors");
                if ((rc = read(hs, 1))) return rc;
                lm.currentChi = hs[0];
                R.initial_chi2 = lm.currentChi;
            }
            if (launch_eg_build(st, P, W, est, fix_scale, &c->prof)) return fail("build");
            lm_begin(&lm, it, 0.0, 1e-16);  // setUserLambdaInit(1e-16): the diagonal is not read
            double rhoLM = 0.0;
            do {
                HIPCHK(hipMemcpyAsync(g->d_backup, est, vbytes, hipMemcpyDeviceToDevice, st));  // push
                if (launch_eg_solve(st, P, W, lm.lambda, (int32_t *)(W.sc + 3), &c->prof) ||
                    launch_eg_update(st, P, W, lm.lambda, est, fix_scale, W.sc + 1, &c->prof) ||
                    launch_eg_errors(st, P, W, est, W.sc, &c->prof))
                    return fail("trial");
                if ((rc = read(hs, 4))) return rc;
                const bool ok2 = *(const int32_t *)&hs[3] != 0;
                R.trials++;
                if (!lm_trial(&lm, ok2, hs[0], hs[1], &rhoLM))  // pop
                    HIPCHK(hipMemcpyAsync(est, g->d_backup, vbytes, hipMemcpyDeviceToDevice, st));
            } while (lm_retry(&lm, rhoLM));
            R.iterations = it + 1;
            R.final_chi2 = lm.currentChi;
            R.lambda = lm.lambda;
            const int term = lm_end(&lm, rhoLM);
            if (term) {
                R.terminated = term;
                break;
            }
        }
    }
    if (d_Tiw_out && launch_eg_poses(st, est, g->nvert, d_Tiw_out)) return fail("k_eg_poses");
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    if (rep) *rep = R;
    return ORBG_OK;
}

extern "C" int orbg_eg_correct_points_device(orbg_ctx *c, const orbg_sim3d *d_Scw,
                                             const orbg_sim3d *d_Siw, int nvert, const int32_t *d_ref,
                                             const float *d_points, int n, float *d_out)
{
    if (!c) return set_err(ORBG_EINVAL, "context is NULL");
    if (n < 0 || nvert < 1) return set_err(ORBG_EINVAL, "n %d / nvert %d", n, nvert);
    if (n == 0) return ORBG_OK;
    if (!d_Scw || !d_Siw || !d_ref || !d_points || !d_out) return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    if (launch_eg_correct_points(c->stream, (const Sim3d *)d_Scw, (const Sim3d *)d_Siw, nvert, d_ref,
                                 d_points, n, d_out))
        return set_err(ORBG_EIO, "k_eg_correct_points launch failed");
    return ORBG_OK;
}

extern "C" int orbg_optimize_essential_graph(orbg_ctx *c, const orbg_sim3d *Scw, const orbg_sim3d *Snc,
                                             int nvert, const orbg_eg_edge *edges, int nedge,
                                             int fixed, int fix_scale, int iterations,
                                             orbg_sim3d *Siw_out, float *Tiw_out, orbg_lm_report *rep)
{
    if (!c || !Scw || !Snc || !Siw_out) return set_err(ORBG_EINVAL, "NULL argument");
    if (iterations < 0) return set_err(ORBG_EINVAL, "negative iterations");
    orbg_eg_graph *g = nullptr;
    int rc = orbg_eg_graph_create(c, edges, nedge, nvert, fixed, &g);
    if (rc) return rc;
    struct Guard {
        orbg_eg_graph *g;
        ~Guard() { orbg_eg_graph_destroy(g); }
    } guard{g};
    const size_t vbytes = (size_t)nvert * sizeof(orbg_sim3d);
    Layout L;
    const size_t o_c = L.take(vbytes), o_n = L.take(vbytes), o_o = L.take(vbytes),
                 o_t = L.take((size_t)nvert * 48);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(b + o_c, Scw, vbytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b + o_n, Snc, vbytes, hipMemcpyHostToDevice, st));
    orbg_lm_report R{};
    if ((rc = orbg_eg_graph_optimize(c, g, L.at<orbg_sim3d>(b, o_c), L.at<orbg_sim3d>(b, o_n), fix_scale,
                                     iterations, L.at<orbg_sim3d>(b, o_o),
                                     Tiw_out ? L.at<float>(b, o_t) : nullptr, &R)))
        return rc;
    HIPCHK(hipMemcpyAsync(Siw_out, b + o_o, vbytes, hipMemcpyDeviceToHost, st));
    if (Tiw_out) HIPCHK(hipMemcpyAsync(Tiw_out, b + o_t, (size_t)nvert * 48, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (rep) *rep = R;
    return ORBG_OK;
}
