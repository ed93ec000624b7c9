// api_map.hip -- orbg_map_*
#include "orbg_ctx.h"
#include "map_args.h"
#include "essential_args.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// the covisibility Map: observation table, covisibility graph, local map (map_kernels.hip)
// ---------------------------------------------------------------------------
struct orbg_map {
    int device = 0;
    MapDev D{};
    void *d_mem = nullptr;       // one allocation behind every MapDev array
    size_t mem_bytes = 0, o_zero = 0;
    bool dirty = true;           // the observation index is stale (a row changed since)
    bool tree_dirty = true;      // the children lists are stale (a parent may have changed)
    bool touched = false;        // any device work issued yet
    int epoch = 0;               // number of the last call that marks rows dirty
    int32_t *d_cnt = nullptr;    // local_points' per-keyframe counts [nframes][lkf_cap]
    size_t cnt_n = 0;
    hipStream_t stream = nullptr;  // the context stream of the last call
    MapAttach att{};             // orbg_map_attach_keyframes: not owned
    bool attached = false;
    MapEditWs W{};               // Fuse / SearchInNeighbors workspace, allocated at the first call
    void *d_ws = nullptr;
    void *d_lc = nullptr;        // LoopConnections' rows [MAX_LOOP_SET][K] u16 and counts [MAX_LOOP_SET]
    void *d_ap = nullptr;        // the correction's positions in and out [2][P][3] and vertices [P]
    MapLbaWs LW{};               // LocalBundleAdjustment's marks, allocated at the first call
    void *d_lw = nullptr;
    MapLbaWindow LB{};           // orbg_map_local_ba's window, grown on demand
    void *d_lb = nullptr;
    uint8_t *d_lb_erase = nullptr;  // [edge_cap] the vToErase flags of that window
    MapGeom geom{};              // orbg_map_attach_keyframe_geometry: not owned
    MapCreateWs CW{};            // CreateNewMapPoints / ProcessNewKeyFrame workspace, allocated at the first call
    void *d_cw = nullptr;
    std::vector<orbg_edge> lb_edges;           // its edge records, fixed flags and vToErase on the host
    std::vector<int32_t> lb_fixed;
    std::vector<uint8_t> lb_fixed8, lb_erase;
    MapGbaWs GW{};               // GlobalBundleAdjustment's marks (sized by K and P), allocated at the first call
    void *d_gw = nullptr;
    MapLbaWindow GB{};           // orbg_map_global_ba's window, its edges grown on demand
    void *d_gb = nullptr;
    std::vector<orbg_edge> gb_edges;           // its edge records and fixed flags on the host
    std::vector<int32_t> gb_fixed;
    std::vector<uint8_t> gb_fixed8;
};

static int map_reset(orbg_map *m, hipStream_t st)
{
    MapDev &D = m->D;
    uint8_t *b = (uint8_t *)m->d_mem;
    HIPCHK(hipMemsetAsync(b + m->o_zero, 0, m->mem_bytes - m->o_zero, st));
    HIPCHK(hipMemsetAsync(D.kf_points, 0xFF, (size_t)D.K * D.cap * 4, st));
    HIPCHK(hipMemsetAsync(D.parent, 0xFF, (size_t)D.K * 4, st));
    HIPCHK(hipMemsetAsync(D.neigh, 0xFF, (size_t)D.K * ORBG_MAP_NEIGH * 4, st));
    HIPCHK(hipMemsetAsync(D.child_head, 0xFF, (size_t)D.K * 4, st));
    HIPCHK(hipMemsetAsync(D.child_next, 0xFF, (size_t)D.K * 4, st));
    HIPCHK(hipMemsetAsync(D.mp_replaced, 0xFF, (size_t)D.P * 4, st));
    if (launch_map_point_defaults(st, D)) return set_err(ORBG_EIO, "k_map_point_defaults launch failed");
    if (launch_map_loop_defaults(st, D)) return set_err(ORBG_EIO, "k_loop_defaults launch failed");
    m->dirty = m->tree_dirty = true;
    return ORBG_OK;
}

extern "C" int orbg_map_create(orbg_ctx *c, int max_keyframes, int kf_cap, int max_points,
                               orbg_map **out)
{
    if (!c || !out) return set_err(ORBG_EINVAL, "NULL argument");
    *out = nullptr;
    if (max_keyframes < 1 || kf_cap < 1 || max_points < 1)
        return set_err(ORBG_EINVAL, "max_keyframes / kf_cap / max_points < 1");
    if (max_keyframes > ORBG_MAP_MAX_KEYFRAMES)
        return set_err(ORBG_ENOTSUP, "max_keyframes %d (> %d: the per-slot counters live in LDS)",
                       max_keyframes, ORBG_MAP_MAX_KEYFRAMES);
    if (kf_cap > ORBG_MAP_MAX_KF_CAP)
        return set_err(ORBG_ENOTSUP, "kf_cap %d (> %d)", kf_cap, ORBG_MAP_MAX_KF_CAP);
    HIPCHK(hipSetDevice(c->device));
    const size_t K = (size_t)max_keyframes, kc = K * (size_t)kf_cap, P = (size_t)max_points;
    Layout L;
    const size_t o_kp = L.take(kc * 4), o_ot = L.take(kc * 4), o_ob = L.take(kc * 4);
    const size_t o_ko = L.take(kc);  // everything from here on starts at zero
    const size_t o_fl = L.take(K * 4), o_kn = L.take(K * 4), o_ce = L.take(K * 12);
    const size_t o_pa = L.take(K * 4), o_fc = L.take(K * 4);
    const size_t o_mp = L.take(P * sizeof(orbg_map_point)), o_md = L.take(P * 32);
    const size_t o_mr = L.take(P * 4);
    const size_t o_w = L.take(K * K * 2), o_os = L.take(K * K * 2), o_ow = L.take(K * K * 2);
    const size_t o_no = L.take(K * 4), o_ng = L.take(K * ORBG_MAP_NEIGH * 4);
    const size_t o_of = L.take((P + 1) * 4), o_oc = L.take(P * 4);
    const size_t o_pt = L.take((P / 2048 + 2) * 4);
    const size_t o_ch = L.take(K * 4), o_cn = L.take(K * 4);
    const size_t o_di = L.take(K * 4), o_mk = L.take(K * 4), o_nl = L.take(4);
    const size_t o_kf = L.take(kc), o_ke = L.take(K * 4);
    const size_t o_pf = L.take(P * 4), o_pv = L.take(P * 4), o_pn = L.take(P * 4);
    const size_t o_rt = L.take(K * 4), o_cl = L.take(K * 4), o_cs = L.take(K * 8), o_co = L.take(16);
    const size_t o_rp = L.take(P * 4), o_en = L.take(P * 4), o_et = L.take(P * 4);
    const size_t o_ec = L.take(P * 4), o_ei = L.take(P * 4), o_em = L.take(P * 4);
    const size_t o_ef = L.take(P * 4);
    const size_t o_tc = L.take(K * 48), o_kp2 = L.take(K * 4), o_id = L.take(K * 4);
    const size_t o_ln = L.take(K * 4), o_ls = L.take(K * ORBG_MAP_MAX_LOOP_EDGES * 4);
    const size_t o_ck = L.take(P * 4), o_cr = L.take(P * 4);
    const size_t o_lt = L.take(K * 48), o_lc = L.take(K * 12), o_lp = L.take(K * 4);
    const size_t o_lh = L.take(64), o_sn = L.take(K * 2);
    const size_t o_cs2 = L.take(P * 4), o_vm = L.take(K * 4), o_ec2 = L.take((K + 1) * 4);
    const size_t o_gt = L.take(K * 48), o_gb = L.take(K * 48), o_gk = L.take(K * 4);
    const size_t o_gp = L.take(P * 12), o_gq = L.take(P * 4);
    auto *m = new orbg_map();
    m->device = c->device;
    if (hipMalloc(&m->d_mem, L.total()) != hipSuccess) {
        delete m;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes)", L.total());
    }
    m->mem_bytes = L.total();
    m->o_zero = o_ko;
    uint8_t *b = (uint8_t *)m->d_mem;
    MapDev &D = m->D;
    D.K = max_keyframes;
    D.cap = kf_cap;
    D.P = max_points;
    D.kf_points = L.at<int32_t>(b, o_kp);
    D.obs_tmp = L.at<uint32_t>(b, o_ot);
    D.obs = L.at<uint32_t>(b, o_ob);
    D.kf_oct = L.at<uint8_t>(b, o_ko);
    D.kf_flags = L.at<int32_t>(b, o_fl);
    D.kf_n = L.at<int32_t>(b, o_kn);
    D.kf_centre = L.at<float>(b, o_ce);
    D.parent = L.at<int32_t>(b, o_pa);
    D.first_conn = L.at<int32_t>(b, o_fc);
    D.mp = L.at<orbg_map_point>(b, o_mp);
    D.mdesc = L.at<uint8_t>(b, o_md);
    D.mp_ref = L.at<int32_t>(b, o_mr);
    D.W = L.at<uint16_t>(b, o_w);
    D.ord_slot = L.at<uint16_t>(b, o_os);
    D.ord_w = L.at<uint16_t>(b, o_ow);
    D.nord = L.at<int32_t>(b, o_no);
    D.neigh = L.at<int32_t>(b, o_ng);
    D.obs_off = L.at<int32_t>(b, o_of);
    D.obs_cnt = L.at<int32_t>(b, o_oc);
    D.part = L.at<int32_t>(b, o_pt);
    D.child_head = L.at<int32_t>(b, o_ch);
    D.child_next = L.at<int32_t>(b, o_cn);
    D.dirty = L.at<int32_t>(b, o_di);
    D.mark = L.at<int32_t>(b, o_mk);
    D.nlive = L.at<int32_t>(b, o_nl);
    D.kf_feat = L.at<uint8_t>(b, o_kf);
    D.kf_erase = L.at<int32_t>(b, o_ke);
    D.mp_first = L.at<int32_t>(b, o_pf);
    D.mp_visible = L.at<int32_t>(b, o_pv);
    D.mp_found = L.at<int32_t>(b, o_pn);
    D.row_touch = L.at<int32_t>(b, o_rt);
    D.cull_list = L.at<int32_t>(b, o_cl);
    D.cull_score = L.at<int32_t>(b, o_cs);
    D.cull_out = L.at<int32_t>(b, o_co);
    D.mp_replaced = L.at<int32_t>(b, o_rp);
    D.ed_next = L.at<int32_t>(b, o_en);
    D.ed_tail = L.at<int32_t>(b, o_et);
    D.ed_chain = L.at<int32_t>(b, o_ec);
    D.ed_inkf = L.at<int32_t>(b, o_ei);
    D.ed_mark = L.at<int32_t>(b, o_em);
    D.ed_first = L.at<int32_t>(b, o_ef);
    D.kf_Tcw = L.at<float>(b, o_tc);
    D.kf_pose = L.at<int32_t>(b, o_kp2);
    D.kf_mnid = L.at<int32_t>(b, o_id);
    D.le_n = L.at<int32_t>(b, o_ln);
    D.le_slot = L.at<int32_t>(b, o_ls);
    D.mp_corr_kf = L.at<int32_t>(b, o_ck);
    D.mp_corr_ref = L.at<int32_t>(b, o_cr);
    D.lp_T = L.at<float>(b, o_lt);
    D.lp_c = L.at<float>(b, o_lc);
    D.lp_pos = L.at<int32_t>(b, o_lp);
    D.lp_hdr = L.at<int32_t>(b, o_lh);
    D.lp_snap = L.at<uint16_t>(b, o_sn);
    D.mp_corr_slot = L.at<int32_t>(b, o_cs2);
    D.lp_vmap = L.at<int32_t>(b, o_vm);
    D.lp_ecnt = L.at<int32_t>(b, o_ec2);
    D.kf_TcwGBA = L.at<float>(b, o_gt);
    D.kf_TcwBef = L.at<float>(b, o_gb);
    D.kf_gba = L.at<int32_t>(b, o_gk);
    D.mp_posGBA = L.at<float>(b, o_gp);
    D.mp_gba = L.at<int32_t>(b, o_gq);
    int rc = map_reset(m, c->stream);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess)
        rc = set_err(ORBG_EIO, "Map: the initial clear failed");
    if (rc) {
        hipFree(m->d_mem);
        delete m;
        return rc;
    }
    m->stream = c->stream;
    *out = m;
    return ORBG_OK;
}

extern "C" void orbg_map_destroy(orbg_map *m)
{
    if (!m) return;
    hipSetDevice(m->device);
    if (m->d_cnt) hipFree(m->d_cnt);
    if (m->d_ws) hipFree(m->d_ws);
    if (m->d_lc) hipFree(m->d_lc);
    if (m->d_ap) hipFree(m->d_ap);
    if (m->d_lw) hipFree(m->d_lw);
    if (m->d_lb) hipFree(m->d_lb);
    if (m->d_cw) hipFree(m->d_cw);
    if (m->d_gw) hipFree(m->d_gw);
    if (m->d_gb) hipFree(m->d_gb);
    if (m->d_mem) hipFree(m->d_mem);
    delete m;
}

extern "C" int orbg_map_info(orbg_map *m, int32_t *nlive, int32_t *max_keyframes, int32_t *kf_cap,
                             int32_t *max_points)
{
    if (!m) return set_err(ORBG_EINVAL, "map is NULL");
    if (max_keyframes) *max_keyframes = m->D.K;
    if (kf_cap) *kf_cap = m->D.cap;
    if (max_points) *max_points = m->D.P;
    if (nlive) {
        *nlive = 0;
        if (m->touched) {
            HIPCHK(hipSetDevice(m->device));
            if (launch_map_count(m->stream, m->D)) return set_err(ORBG_EIO, "k_map_count launch failed");
            HIPCHK(hipMemcpyAsync(nlive, m->D.nlive, 4, hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
        }
    }
    return ORBG_OK;
}

static int map_enter(orbg_ctx *c, orbg_map *m)
{
    if (!c || !m) return set_err(ORBG_EINVAL, "NULL context or map");
    if (m->device != c->device) return set_err(ORBG_EINVAL, "map lives on another device");
    HIPCHK(hipSetDevice(c->device));
    if (m->stream != c->stream) {  // the context's stream changed: finish what the old one holds
        if (m->touched) HIPCHK(hipStreamSynchronize(m->stream));
        m->stream = c->stream;
    }
    return ORBG_OK;
}

static int map_slot_ok(const orbg_map *m, int slot)
{
    if (slot < 0 || slot >= m->D.K)
        return set_err(ORBG_EINVAL, "slot %d outside [0, %d)", slot, m->D.K);
    return ORBG_OK;
}

// ---- mutations ----
extern "C" int orbg_map_set_keyframes_device(orbg_ctx *c, orbg_map *m, const int32_t *d_slots,
                                             int n, const int32_t *d_point_ids,
                                             const uint8_t *d_octaves, int row_cap,
                                             const int32_t *d_counts, const float *d_centres,
                                             const int32_t *d_flags)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (row_cap < 1) return set_err(ORBG_EINVAL, "row_cap < 1");
    if (!d_slots || !d_point_ids || !d_octaves || !d_counts || !d_centres || !d_flags)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = launch_map_set_keyframes(c->stream, m->D, d_slots, n, d_point_ids, d_octaves, row_cap,
                                       d_counts, d_centres, d_flags)))
        return set_err(rc, "k_map_set_kf launch failed");
    m->dirty = m->tree_dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_keyframe(orbg_ctx *c, orbg_map *m, int slot, const int32_t *point_ids,
                                     const uint8_t *octaves, int n, const float *centre, int flags)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (n < 0 || n > m->D.cap) return set_err(ORBG_EINVAL, "%d features (kf_cap %d)", n, m->D.cap);
    if (!centre || (n && (!point_ids || !octaves))) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < n; i++)
        if (point_ids[i] >= m->D.P)
            return set_err(ORBG_EINVAL, "point id %d outside [0, %d)", point_ids[i], m->D.P);
    const int cap = std::max(n, 1);
    Layout L;
    const size_t o_p = L.take((size_t)cap * 4), o_o = L.take(cap), o_c = L.take(12);
    const size_t o_h = L.take(12);  // slot, count, flags
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[3] = {slot, n, flags};
    if (n) HIPCHK(hipMemcpyAsync(b + o_p, point_ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(b + o_o, octaves, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, centre, 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_h, hdr, 12, hipMemcpyHostToDevice, c->stream));
    const int32_t *h = L.at<int32_t>(b, o_h);
    rc = orbg_map_set_keyframes_device(c, m, h, 1, L.at<int32_t>(b, o_p), L.at<uint8_t>(b, o_o), cap,
                                       h + 1, L.at<float>(b, o_c), h + 2);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // the scratch is the next host call's too
    return ORBG_OK;
}

extern "C" int orbg_map_set_points_device(orbg_ctx *c, orbg_map *m, const int32_t *d_ids, int first,
                                          int n, const orbg_map_point *d_mps, const uint8_t *d_desc,
                                          const int32_t *d_ref_kf)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_ids && (first < 0 || (int64_t)first + n > m->D.P))
        return set_err(ORBG_EINVAL, "ids %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.P);
    if (!d_mps || !d_desc || !d_ref_kf) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = launch_map_set_points(c->stream, m->D, d_ids, first, n, d_mps, d_desc, d_ref_kf)))
        return set_err(rc, "k_map_set_points launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_points(orbg_ctx *c, orbg_map *m, int first, int n,
                                   const orbg_map_point *mps, const uint8_t *desc,
                                   const int32_t *ref_kf)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (first < 0 || (int64_t)first + n > m->D.P)
        return set_err(ORBG_EINVAL, "ids %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.P);
    if (n == 0) return ORBG_OK;
    if (!mps || !desc || !ref_kf) return set_err(ORBG_EINVAL, "NULL array");
    Layout L;
    const size_t o_m = L.take((size_t)n * sizeof(orbg_map_point)), o_d = L.take((size_t)n * 32);
    const size_t o_r = L.take((size_t)n * 4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_m, mps, (size_t)n * sizeof(orbg_map_point), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_d, desc, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_r, ref_kf, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    rc = orbg_map_set_points_device(c, m, nullptr, first, n, L.at<orbg_map_point>(b, o_m),
                                    L.at<uint8_t>(b, o_d), L.at<int32_t>(b, o_r));
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_get_points(orbg_ctx *c, orbg_map *m, int first, int n, orbg_map_point *mps)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || first < 0 || (int64_t)first + n > m->D.P)
        return set_err(ORBG_EINVAL, "ids %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.P);
    if (n == 0) return ORBG_OK;
    if (!mps) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(mps, m->D.mp + first, (size_t)n * sizeof(orbg_map_point),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_set_point_bad(orbg_ctx *c, orbg_map *m, int id)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (id < 0 || id >= m->D.P) return set_err(ORBG_EINVAL, "point id %d outside [0, %d)", id, m->D.P);
    if (launch_map_point_bad(c->stream, m->D, id)) return set_err(ORBG_EIO, "k_map_point_bad launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_parent(orbg_ctx *c, orbg_map *m, int slot, int parent)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (parent < -1 || parent >= m->D.K)
        return set_err(ORBG_EINVAL, "parent %d outside [-1, %d)", parent, m->D.K);
    if (launch_map_set_parent(c->stream, m->D, slot, parent))
        return set_err(ORBG_EIO, "k_map_set_parent launch failed");
    m->tree_dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_erase_keyframe(orbg_ctx *c, orbg_map *m, int slot)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (launch_map_erase(c->stream, m->D, slot, ++m->epoch))
        return set_err(ORBG_EIO, "k_map_erase launch failed");
    m->dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_clear(orbg_ctx *c, orbg_map *m)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_reset(m, c->stream))) return rc;
    m->epoch = 0;
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_rebuild(orbg_ctx *c, orbg_map *m)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (m->dirty) {
        if ((rc = launch_map_rebuild(c->stream, m->D, &c->prof)))
            return set_err(rc, "observation index rebuild launch failed");
        m->dirty = false;
        m->touched = true;
    }
    if (m->tree_dirty) {
        if ((rc = launch_map_tree(c->stream, m->D))) return set_err(rc, "k_map_tree launch failed");
        m->tree_dirty = false;
        m->touched = true;
    }
    return ORBG_OK;
}

// ---- readers ----
extern "C" int orbg_map_neighbours(orbg_map *m, const int32_t **d_neigh)
{
    if (!m || !d_neigh) return set_err(ORBG_EINVAL, "NULL argument");
    *d_neigh = m->D.neigh;
    return ORBG_OK;
}

extern "C" int orbg_map_get_neighbours(orbg_ctx *c, orbg_map *m, int32_t *neigh)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (!neigh) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(neigh, m->D.neigh, (size_t)m->D.K * ORBG_MAP_NEIGH * 4,
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_connected_device(orbg_ctx *c, orbg_map *m, const int32_t *d_slots, int n,
                                         int32_t *d_conn, int conn_cap, int32_t *d_nconn)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || conn_cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_slots || !d_nconn || (conn_cap && !d_conn)) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = launch_map_connected(c->stream, m->D, d_slots, n, d_conn, conn_cap, d_nconn)))
        return set_err(rc, "k_map_connected launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_get_connections(orbg_ctx *c, orbg_map *m, int slot, int32_t *slots,
                                        int32_t *weights, int cap, int32_t *n, int32_t *parent)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (cap < 0 || !n || (cap && (!slots || !weights))) return set_err(ORBG_EINVAL, "bad cap / NULL array");
    const MapDev &D = m->D;
    int32_t hdr[2] = {0, -1};
    HIPCHK(hipMemcpyAsync(&hdr[0], D.nord + slot, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&hdr[1], D.parent + slot, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(hdr[0], cap);
    if (nw > 0) {
        std::vector<uint16_t> s(nw), w(nw);
        HIPCHK(hipMemcpy(s.data(), D.ord_slot + (size_t)slot * D.K, (size_t)nw * 2, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(w.data(), D.ord_w + (size_t)slot * D.K, (size_t)nw * 2, hipMemcpyDeviceToHost));
        for (int i = 0; i < nw; i++) {
            slots[i] = s[i];
            weights[i] = w[i];
        }
    }
    *n = hdr[0];
    if (parent) *parent = hdr[1];
    if (hdr[0] > cap) return set_err(ORBG_ERANGE, "%d connections (cap %d)", hdr[0], cap);
    return ORBG_OK;
}

extern "C" int orbg_map_get_weights(orbg_ctx *c, orbg_map *m, int slot, uint16_t *weights)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (!weights) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(weights, m->D.W + (size_t)slot * m->D.K, (size_t)m->D.K * 2,
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

// ---- KeyFrame::UpdateConnections ----
extern "C" int orbg_map_update_connections_batch_device(orbg_ctx *c, orbg_map *m,
                                                        const int32_t *d_slots, int n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_slots) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_update_connections(c->stream, m->D, d_slots, n, ++m->epoch, &c->prof)))
        return set_err(rc, "k_map_update launch failed");
    m->tree_dirty = m->touched = true;  // a first connection sets a parent
    return ORBG_OK;
}

extern "C" int orbg_map_update_connections(orbg_ctx *c, orbg_map *m, int slot)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    Layout L;
    const size_t o_s = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t sl = slot;
    HIPCHK(hipMemcpyAsync(b + o_s, &sl, 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_update_connections_batch_device(c, m, L.at<int32_t>(b, o_s), 1))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// ---- Tracking::UpdateLocalKeyFrames / UpdateLocalPoints ----
extern "C" int orbg_map_local_keyframes_batch_device(orbg_ctx *c, orbg_map *m,
                                                     int32_t *d_frame_points, int frame_cap,
                                                     const int32_t *d_counts, int nframes,
                                                     int32_t *d_local_kfs, int lkf_cap,
                                                     int32_t *d_nlocal, int32_t *d_ref_kf)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (nframes < 0 || frame_cap < 1 || lkf_cap < 0) return set_err(ORBG_EINVAL, "bad nframes / cap");
    if (nframes == 0) return ORBG_OK;
    if (!d_frame_points || !d_counts || !d_nlocal || !d_ref_kf || (lkf_cap && !d_local_kfs))
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_local_keyframes(c->stream, m->D, d_frame_points, frame_cap, d_counts, nframes,
                                         d_local_kfs, lkf_cap, d_nlocal, d_ref_kf, &c->prof)))
        return set_err(rc, "k_map_local_kfs launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_local_points_batch_device(orbg_ctx *c, orbg_map *m,
                                                  const int32_t *d_local_kfs, int lkf_cap,
                                                  const int32_t *d_nlocal,
                                                  const int32_t *d_frame_points, int frame_cap,
                                                  const int32_t *d_counts, int nframes,
                                                  int32_t *d_local_ids, orbg_map_point *d_mps,
                                                  uint8_t *d_qdesc, int lp_cap,
                                                  int32_t *d_nlocal_points)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (nframes < 0 || nframes > 65535 || frame_cap < 1 || lkf_cap < 1 || lp_cap < 0)
        return set_err(ORBG_EINVAL, "bad nframes / cap");
    if (frame_cap > ORBG_MAP_MAX_FRAME_CAP)
        return set_err(ORBG_ENOTSUP, "frame_cap %d (> %d)", frame_cap, ORBG_MAP_MAX_FRAME_CAP);
    if (lkf_cap > m->D.K) return set_err(ORBG_EINVAL, "lkf_cap %d above max_keyframes %d", lkf_cap, m->D.K);
    if (nframes == 0) return ORBG_OK;
    if (!d_local_kfs || !d_nlocal || !d_frame_points || !d_counts || !d_nlocal_points ||
        (lp_cap && (!d_local_ids || !d_mps || !d_qdesc)))
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    const size_t need = (size_t)nframes * lkf_cap;
    if (need > m->cnt_n) {
        if (m->d_cnt) {
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipFree(m->d_cnt));
            m->d_cnt = nullptr;
            m->cnt_n = 0;
        }
        if ((rc = dalloc(&m->d_cnt, need))) return rc;
        m->cnt_n = need;
    }
    if ((rc = launch_map_local_points(c->stream, m->D, d_local_kfs, lkf_cap, d_nlocal, d_frame_points,
                                      frame_cap, d_counts, nframes, m->d_cnt, d_local_ids, d_mps,
                                      d_qdesc, lp_cap, d_nlocal_points, &c->prof)))
        return set_err(rc, "k_map_lp launch failed");
    m->touched = true;
    return ORBG_OK;
}

// one frame from host arrays: uploads, runs the batched forms with one frame, downloads
extern "C" int orbg_map_local_keyframes(orbg_ctx *c, orbg_map *m, int32_t *frame_points, int n,
                                        int32_t *local_kfs, int lkf_cap, int32_t *nlocal,
                                        int32_t *ref_kf)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || lkf_cap < 0 || !nlocal) return set_err(ORBG_EINVAL, "bad size / NULL argument");
    if ((n && !frame_points) || (lkf_cap && !local_kfs)) return set_err(ORBG_EINVAL, "NULL array");
    const int fc = std::max(n, 1);
    Layout L;
    const size_t o_f = L.take((size_t)fc * 4), o_c = L.take(4), o_l = L.take((size_t)lkf_cap * 4);
    const size_t o_o = L.take(8);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t cnt = n;
    if (n) HIPCHK(hipMemcpyAsync(b + o_f, frame_points, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, &cnt, 4, hipMemcpyHostToDevice, c->stream));
    int32_t *o = L.at<int32_t>(b, o_o);
    if ((rc = orbg_map_local_keyframes_batch_device(c, m, L.at<int32_t>(b, o_f), fc,
                                                    L.at<int32_t>(b, o_c), 1, L.at<int32_t>(b, o_l),
                                                    lkf_cap, o, o + 1)))
        return rc;
    int32_t out[2] = {0, -1};
    HIPCHK(hipMemcpyAsync(out, o, 8, hipMemcpyDeviceToHost, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(frame_points, b + o_f, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(out[0], lkf_cap);
    if (nw > 0) HIPCHK(hipMemcpy(local_kfs, b + o_l, (size_t)nw * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *nlocal = out[0];
    if (ref_kf) *ref_kf = out[1];
    if (out[0] > lkf_cap) return set_err(ORBG_ERANGE, "%d local keyframes (cap %d)", out[0], lkf_cap);
    return ORBG_OK;
}

extern "C" int orbg_map_local_points(orbg_ctx *c, orbg_map *m, const int32_t *local_kfs, int nlocal,
                                     const int32_t *frame_points, int n, int32_t *local_ids,
                                     orbg_map_point *mps, uint8_t *qdesc, int lp_cap,
                                     int32_t *nlocal_points)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || nlocal < 0 || lp_cap < 0 || !nlocal_points)
        return set_err(ORBG_EINVAL, "bad size / NULL argument");
    if (nlocal > m->D.K) return set_err(ORBG_EINVAL, "%d local keyframes (max_keyframes %d)", nlocal, m->D.K);
    if ((n && !frame_points) || (nlocal && !local_kfs) || (lp_cap && (!local_ids || !mps || !qdesc)))
        return set_err(ORBG_EINVAL, "NULL array");
    const int fc = std::max(n, 1), lc = std::max(nlocal, 1);
    Layout L;
    const size_t o_f = L.take((size_t)fc * 4), o_c = L.take(8), o_l = L.take((size_t)lc * 4);
    const size_t o_i = L.take((size_t)lp_cap * 4), o_m = L.take((size_t)lp_cap * sizeof(orbg_map_point));
    const size_t o_d = L.take((size_t)lp_cap * 32), o_o = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t cnt[2] = {n, nlocal};
    if (n) HIPCHK(hipMemcpyAsync(b + o_f, frame_points, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (nlocal) HIPCHK(hipMemcpyAsync(b + o_l, local_kfs, (size_t)nlocal * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, cnt, 8, hipMemcpyHostToDevice, c->stream));
    const int32_t *dc = L.at<int32_t>(b, o_c);
    if ((rc = orbg_map_local_points_batch_device(c, m, L.at<int32_t>(b, o_l), lc, dc + 1,
                                                 L.at<int32_t>(b, o_f), fc, dc, 1,
                                                 L.at<int32_t>(b, o_i), L.at<orbg_map_point>(b, o_m),
                                                 L.at<uint8_t>(b, o_d), lp_cap, L.at<int32_t>(b, o_o))))
        return rc;
    int32_t out = 0;
    HIPCHK(hipMemcpyAsync(&out, b + o_o, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(out, lp_cap);
    if (nw > 0) {
        HIPCHK(hipMemcpy(local_ids, b + o_i, (size_t)nw * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mps, b + o_m, (size_t)nw * sizeof(orbg_map_point), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(qdesc, b + o_d, (size_t)nw * 32, hipMemcpyDeviceToHost));
    }
    c->prof.collect();
    *nlocal_points = out;
    if (out > lp_cap) return set_err(ORBG_ERANGE, "%d local points (cap %d)", out, lp_cap);
    return ORBG_OK;
}

// ---- MapPoint::UpdateNormalAndDepth ----
extern "C" int orbg_map_update_normal_and_depth_batch_device(orbg_ctx *c, orbg_map *m,
                                                             const int32_t *d_point_ids, int n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!d_point_ids && n > m->D.P) return set_err(ORBG_EINVAL, "%d points (max_points %d)", n, m->D.P);
    if (n == 0) return ORBG_OK;
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    MapScales S{};
    S.nlevels = std::min(std::max(c->p.nlevels, 1), 16);
    for (int i = 0; i < 16; i++) S.scale[i] = c->scale[i];
    if ((rc = launch_map_normal_depth(c->stream, m->D, d_point_ids, n, S, &c->prof)))
        return set_err(rc, "k_map_normal_depth launch failed");
    m->touched = true;
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// KeyFrame::SetBadFlag, LocalMapping::KeyFrameCulling / MapPointCulling (map_cull_kernels.hip)
// ---------------------------------------------------------------------------
static int map_range_ok(const orbg_map *m, int first, int n)
{
    if (n < 0 || first < 0 || (int64_t)first + n > m->D.P)
        return set_err(ORBG_EINVAL, "ids %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.P);
    return ORBG_OK;
}

extern "C" int orbg_map_set_keyframe_features_device(orbg_ctx *c, orbg_map *m,
                                                     const int32_t *d_slots, int n,
                                                     const uint8_t *d_flags, int row_cap,
                                                     const int32_t *d_counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (row_cap < 1) return set_err(ORBG_EINVAL, "row_cap < 1");
    if (!d_slots || !d_flags || !d_counts) return set_err(ORBG_EINVAL, "NULL device array");
    if (launch_map_set_features(c->stream, m->D, d_slots, n, d_flags, row_cap, d_counts))
        return set_err(ORBG_EIO, "k_map_set_features launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_keyframe_features(orbg_ctx *c, orbg_map *m, int slot,
                                              const uint8_t *flags, int n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (n < 0 || n > m->D.cap) return set_err(ORBG_EINVAL, "%d features (kf_cap %d)", n, m->D.cap);
    if (n && !flags) return set_err(ORBG_EINVAL, "NULL array");
    const int cap = std::max(n, 1);
    Layout L;
    const size_t o_f = L.take(cap), o_h = L.take(8);  // slot, count
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[2] = {slot, n};
    if (n) HIPCHK(hipMemcpyAsync(b + o_f, flags, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_h, hdr, 8, hipMemcpyHostToDevice, c->stream));
    const int32_t *h = L.at<int32_t>(b, o_h);
    if ((rc = orbg_map_set_keyframe_features_device(c, m, h, 1, b + o_f, cap, h + 1))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_set_point_stats_device(orbg_ctx *c, orbg_map *m, const int32_t *d_ids,
                                               int first, int n, const int32_t *d_first_kf_id,
                                               const int32_t *d_visible, const int32_t *d_found)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!d_ids && (rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (launch_map_set_point_stats(c->stream, m->D, d_ids, first, n, d_first_kf_id, d_visible, d_found))
        return set_err(ORBG_EIO, "k_map_set_point_stats launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_point_stats(orbg_ctx *c, orbg_map *m, int first, int n,
                                        const int32_t *first_kf_id, const int32_t *visible,
                                        const int32_t *found)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    Layout L;
    const size_t o[3] = {L.take((size_t)n * 4), L.take((size_t)n * 4), L.take((size_t)n * 4)};
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t *src[3] = {first_kf_id, visible, found};
    const int32_t *d[3];
    for (int k = 0; k < 3; k++) {
        d[k] = src[k] ? L.at<int32_t>(b, o[k]) : nullptr;
        if (src[k]) HIPCHK(hipMemcpyAsync(b + o[k], src[k], (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = orbg_map_set_point_stats_device(c, m, nullptr, first, n, d[0], d[1], d[2]))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_get_point_stats(orbg_ctx *c, orbg_map *m, int first, int n,
                                        int32_t *first_kf_id, int32_t *visible, int32_t *found,
                                        int32_t *nobs)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    const MapDev &D = m->D;
    const size_t nb = (size_t)n * 4;
    if (first_kf_id) HIPCHK(hipMemcpyAsync(first_kf_id, D.mp_first + first, nb, hipMemcpyDeviceToHost, c->stream));
    if (visible) HIPCHK(hipMemcpyAsync(visible, D.mp_visible + first, nb, hipMemcpyDeviceToHost, c->stream));
    if (found) HIPCHK(hipMemcpyAsync(found, D.mp_found + first, nb, hipMemcpyDeviceToHost, c->stream));
    if (nobs) {
        if ((rc = orbg_map_rebuild(c, m))) return rc;
        Layout L;
        const size_t o_n = L.take(nb);
        uint8_t *b;
        if ((rc = L.device(c, &b))) return rc;
        if (launch_map_point_nobs(c->stream, D, first, n, L.at<int32_t>(b, o_n)))
            return set_err(ORBG_EIO, "k_map_point_nobs launch failed");
        m->touched = true;
        HIPCHK(hipMemcpyAsync(nobs, b + o_n, nb, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

static int map_increase(orbg_ctx *c, orbg_map *m, int32_t *counter, const int32_t *d_ids,
                        const orbg_map_projection *d_proj, int n, int amount)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_ids) return set_err(ORBG_EINVAL, "NULL device array");
    if (launch_map_increase(c->stream, counter, m->D.P, d_ids, d_proj, n, amount))
        return set_err(ORBG_EIO, "k_map_increase launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_increase_visible_device(orbg_ctx *c, orbg_map *m, const int32_t *d_ids,
                                                const orbg_map_projection *d_proj, int n,
                                                int amount)
{
    return map_increase(c, m, m ? m->D.mp_visible : nullptr, d_ids, d_proj, n, amount);
}

extern "C" int orbg_map_increase_found_device(orbg_ctx *c, orbg_map *m, const int32_t *d_ids, int n,
                                              int amount)
{
    return map_increase(c, m, m ? m->D.mp_found : nullptr, d_ids, nullptr, n, amount);
}

extern "C" int orbg_map_get_keyframe_points(orbg_ctx *c, orbg_map *m, int slot, int32_t *ids,
                                            int cap, int32_t *n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (cap < 0 || !n || (cap && !ids)) return set_err(ORBG_EINVAL, "bad cap / NULL array");
    int32_t cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, m->D.kf_n + slot, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(cnt, cap);
    if (nw > 0)
        HIPCHK(hipMemcpy(ids, m->D.kf_points + (size_t)slot * m->D.cap, (size_t)nw * 4, hipMemcpyDeviceToHost));
    *n = cnt;
    return ORBG_OK;
}

extern "C" int orbg_map_get_point_refs(orbg_ctx *c, orbg_map *m, int first, int n, int32_t *ref)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (!ref) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(ref, m->D.mp_ref + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

// on: 1 SetNotErase, 0 SetErase, -1 SetBadFlag; the kernel's status comes back through cull_out
static int map_set_bad(orbg_ctx *c, orbg_map *m, int slot, int on, int32_t *status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (on != 1 && (rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_set_bad(c->stream, m->D, slot, on, ++m->epoch, m->D.cull_out, &c->prof)))
        return set_err(rc, "k_map_set_bad launch failed");
    m->touched = true;
    if (on != 1) m->dirty = m->tree_dirty = true;  // rows lost entries, parents may have changed
    int32_t st = 0;
    HIPCHK(hipMemcpyAsync(&st, m->D.cull_out, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    if (status) *status = st;
    return ORBG_OK;
}

extern "C" int orbg_map_set_not_erase(orbg_ctx *c, orbg_map *m, int slot, int on, int32_t *erased)
{
    return map_set_bad(c, m, slot, on ? 1 : 0, erased);
}

extern "C" int orbg_map_set_bad_flag(orbg_ctx *c, orbg_map *m, int slot, int32_t *status)
{
    return map_set_bad(c, m, slot, -1, status);
}

extern "C" int orbg_map_keyframe_culling_device(orbg_ctx *c, orbg_map *m, int slot, int monocular,
                                                orbg_cull_record *d_records, int rec_cap,
                                                int32_t *d_nrec)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (rec_cap < 0 || !d_nrec || (rec_cap && !d_records))
        return set_err(ORBG_EINVAL, "bad rec_cap / NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_keyframe_culling(c->stream, m->D, slot, monocular != 0, ++m->epoch,
                                          d_records, rec_cap, d_nrec, &c->prof)))
        return set_err(rc, "KeyFrameCulling launch failed");
    m->dirty = m->tree_dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_keyframe_culling(orbg_ctx *c, orbg_map *m, int slot, int monocular,
                                         orbg_cull_record *records, int rec_cap, int32_t *nrec)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (rec_cap < 0 || !nrec || (rec_cap && !records))
        return set_err(ORBG_EINVAL, "bad rec_cap / NULL array");
    Layout L;
    const size_t o_r = L.take((size_t)rec_cap * sizeof(orbg_cull_record)), o_n = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    if ((rc = orbg_map_keyframe_culling_device(c, m, slot, monocular, L.at<orbg_cull_record>(b, o_r),
                                               rec_cap, L.at<int32_t>(b, o_n))))
        return rc;
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(n, rec_cap);
    if (nw > 0) HIPCHK(hipMemcpy(records, b + o_r, (size_t)nw * sizeof(orbg_cull_record), hipMemcpyDeviceToHost));
    c->prof.collect();
    *nrec = n;
    if (n > rec_cap) return set_err(ORBG_ERANGE, "%d list entries (rec_cap %d)", n, rec_cap);
    return ORBG_OK;
}

extern "C" int orbg_map_point_culling_device(orbg_ctx *c, orbg_map *m, int32_t *d_recent, int n,
                                             int current_kf_id, int monocular, int32_t *d_nout,
                                             int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!d_nout || (n && !d_recent)) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_point_culling(c->stream, m->D, d_recent, n, current_kf_id, monocular != 0,
                                       d_nout, d_status, &c->prof)))
        return set_err(rc, "MapPointCulling launch failed");
    m->dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_point_culling(orbg_ctx *c, orbg_map *m, int32_t *recent, int n,
                                      int current_kf_id, int monocular, int32_t *nout,
                                      int32_t *status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || !nout || (n && !recent)) return set_err(ORBG_EINVAL, "negative size / NULL array");
    for (int i = 0; i < n; i++)
        if (recent[i] < 0 || recent[i] >= m->D.P)
            return set_err(ORBG_EINVAL, "point id %d outside [0, %d)", recent[i], m->D.P);
    const size_t nb = (size_t)std::max(n, 1) * 4;
    Layout L;
    const size_t o_r = L.take(nb), o_s = L.take(nb), o_n = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(b + o_r, recent, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_point_culling_device(c, m, L.at<int32_t>(b, o_r), n, current_kf_id, monocular,
                                            L.at<int32_t>(b, o_n), L.at<int32_t>(b, o_s))))
        return rc;
    int32_t k = 0;
    HIPCHK(hipMemcpyAsync(&k, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (n && status) HIPCHK(hipMemcpyAsync(status, b + o_s, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (k > 0) HIPCHK(hipMemcpy(recent, b + o_r, (size_t)k * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *nout = k;
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// MapPoint::Replace, Fuse's map update, SearchInNeighbors (map_edit_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_map_get_point_replaced(orbg_ctx *c, orbg_map *m, int first, int n,
                                           int32_t *replaced)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (!replaced) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(replaced, m->D.mp_replaced + first, (size_t)n * 4, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_get_point_descriptors(orbg_ctx *c, orbg_map *m, int first, int n,
                                              uint8_t *desc)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (!desc) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(desc, m->D.mdesc + (size_t)first * 32, (size_t)n * 32, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_attach_keyframes(orbg_ctx *c, orbg_map *m, const orbg_keyframes *kfs, int cap,
                                         const orbg_frustum_camera *d_cams)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (!kfs) {
        m->attached = false;
        m->att = MapAttach{};
        return ORBG_OK;
    }
    if (cap < 1 || cap > ORBG_MAP_MAX_KF_CAP) return set_err(ORBG_EINVAL, "cap %d outside [1, %d]", cap, ORBG_MAP_MAX_KF_CAP);
    if (!kfs->desc || !kfs->kps || !kfs->counts || !d_cams)
        return set_err(ORBG_EINVAL, "NULL device array (desc, kps, counts and the cameras are read)");
    m->att.kfs = *kfs;
    m->att.cap = cap;
    m->att.cams = d_cams;
    m->attached = true;
    return ORBG_OK;
}

static int map_attached(const orbg_map *m)
{
    return m->attached ? ORBG_OK : set_err(ORBG_EINVAL, "no keyframe data attached (orbg_map_attach_keyframes)");
}

// the workspace of one Fuse / SearchInNeighbors call over up to ncap points
static int map_edit_ws(orbg_ctx *c, orbg_map *m, int ncap)
{
    if (m->d_ws && ncap <= m->W.ncap) return ORBG_OK;
    if (m->d_ws) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(m->d_ws));
        m->d_ws = nullptr;
        m->W = MapEditWs{};
    }
    const size_t n = (size_t)ncap;
    Layout L;
    const size_t o_h = L.take(16 * 4), o_c = L.take(sizeof(orbg_frustum_camera));
    const size_t o_t = L.take((ORBG_MAP_MAX_TARGETS + 8) * 4), o_s = L.take(((size_t)m->D.cap + 1) * 4);
    const size_t o_i = L.take((n + 1) * 4), o_m = L.take(n * sizeof(orbg_map_point)), o_d = L.take(n * 32);
    const size_t o_bi = L.take(n * 4), o_bd = L.take(n * 4), o_st = L.take(n * 4), o_sv = L.take(n * 4);
    const size_t o_do = L.take((n + 1) * 4), o_db = L.take(n * 4), o_dd = L.take(n * 32);
    if (hipMalloc(&m->d_ws, L.total()) != hipSuccess) {
        m->d_ws = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the edit workspace", L.total());
    }
    HIPCHK(hipMemsetAsync(m->d_ws, 0, L.total(), c->stream));
    uint8_t *b = (uint8_t *)m->d_ws;
    MapEditWs &W = m->W;
    W.ncap = ncap;
    W.hdr = L.at<int32_t>(b, o_h);
    W.cam = L.at<orbg_frustum_camera>(b, o_c);
    W.targets = L.at<int32_t>(b, o_t);
    W.snap = L.at<int32_t>(b, o_s);
    W.ids = L.at<int32_t>(b, o_i);
    W.mps = L.at<orbg_map_point>(b, o_m);
    W.mdesc = L.at<uint8_t>(b, o_d);
    W.bidx = L.at<int32_t>(b, o_bi);
    W.bdist = L.at<int32_t>(b, o_bd);
    W.hits = L.at<int32_t>(b, o_st);
    W.surv = L.at<int32_t>(b, o_sv);
    W.dd_off = L.at<int32_t>(b, o_do);
    W.dd_best = L.at<int32_t>(b, o_db);
    W.dd_desc = L.at<uint8_t>(b, o_dd);
    return ORBG_OK;
}

extern "C" int orbg_map_add_observations_device(orbg_ctx *c, orbg_map *m, const int32_t *d_slots,
                                                const int32_t *d_idx, const int32_t *d_point_ids,
                                                int n, int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_slots || !d_idx || !d_point_ids) return set_err(ORBG_EINVAL, "NULL device array");
    if (launch_map_add_observations(c->stream, m->D, d_slots, d_idx, d_point_ids, n, d_status))
        return set_err(ORBG_EIO, "k_map_add_obs launch failed");
    m->dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_add_observations(orbg_ctx *c, orbg_map *m, const int32_t *slots,
                                         const int32_t *idx, const int32_t *point_ids, int n,
                                         int32_t *status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!slots || !idx || !point_ids) return set_err(ORBG_EINVAL, "NULL array");
    const size_t nb = (size_t)n * 4;
    Layout L;
    const size_t o_s = L.take(nb), o_i = L.take(nb), o_p = L.take(nb), o_st = L.take(nb);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_s, slots, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_i, idx, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_p, point_ids, nb, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_add_observations_device(c, m, L.at<int32_t>(b, o_s), L.at<int32_t>(b, o_i),
                                               L.at<int32_t>(b, o_p), n, L.at<int32_t>(b, o_st))))
        return rc;
    if (status) HIPCHK(hipMemcpyAsync(status, b + o_st, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

// ComputeDistinctiveDescriptors of d_ids[i], i < min(n, d_n[0]); the workspace holds n entries
static int map_distinctive(orbg_ctx *c, orbg_map *m, const int32_t *d_ids, int n, const int32_t *d_n)
{
    int rc = orbg_map_rebuild(c, m);
    if (rc) return rc;
    const MapEditWs &W = m->W;
    hipStream_t st = c->stream;
    PROF_LAUNCH(c, "map_distinctive",
                rc = launch_map_distinctive(st, m->D, m->att, d_ids, n, d_n, ++m->epoch, W.dd_off,
                                            W.hdr + MAP_HDR_TOT, W.dd_best, W.dd_desc));
    if (rc) return set_err(rc, "ComputeDistinctiveDescriptors launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_distinctive_descriptors_device(orbg_ctx *c, orbg_map *m,
                                                       const int32_t *d_point_ids, int n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (n == 0) return ORBG_OK;
    if (!d_point_ids) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, n))) return rc;
    return map_distinctive(c, m, d_point_ids, n, nullptr);
}

extern "C" int orbg_map_replace_device(orbg_ctx *c, orbg_map *m, const int32_t *d_old,
                                       const int32_t *d_new, int n, int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (n == 0) return ORBG_OK;
    if (!d_old || !d_new) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, n))) return rc;
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    hipStream_t st = c->stream;
    PROF_LAUNCH(c, "map_replace", rc = launch_map_replace(st, m->D, d_old, d_new, n, ++m->epoch,
                                                         d_status, m->W.surv));
    if (rc) return set_err(rc, "k_map_replace launch failed");
    m->dirty = m->touched = true;
    return map_distinctive(c, m, m->W.surv, n, nullptr);
}

extern "C" int orbg_map_replace(orbg_ctx *c, orbg_map *m, const int32_t *olds, const int32_t *news,
                                int n, int32_t *status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (n == 0) return ORBG_OK;
    if (!olds || !news) return set_err(ORBG_EINVAL, "NULL array");
    const size_t nb = (size_t)n * 4;
    Layout L;
    const size_t o_o = L.take(nb), o_n = L.take(nb), o_st = L.take(nb);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_o, olds, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, news, nb, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_replace_device(c, m, L.at<int32_t>(b, o_o), L.at<int32_t>(b, o_n), n,
                                      L.at<int32_t>(b, o_st))))
        return rc;
    if (status) HIPCHK(hipMemcpyAsync(status, b + o_st, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// One Fuse call: the job (slot >= 0 from the host, else an entry of SearchInNeighbors' device
// lists), the gather, the existing search, the sequential update, the survivors' descriptors.
static int map_fuse_core(orbg_ctx *c, orbg_map *m, int slot, const int32_t *d_ids, int n, int nmax,
                         int entry, int cur, float th, int32_t *d_best_idx, int32_t *d_best_dist,
                         int32_t *d_status, int32_t *d_nfused, int at_ntargets)
{
    int rc = orbg_map_rebuild(c, m);
    if (rc) return rc;
    const MapEditWs &W = m->W;
    hipStream_t st = c->stream;
    if (launch_map_fuse_job(st, m->D, m->att, W, slot, n, entry, cur) ||
        launch_map_fuse_gather(st, m->D, W, d_ids, nmax))
        return set_err(ORBG_EIO, "k_fuse_gather launch failed");
    PROF_LAUNCH(c, "map_fuse_search",
                rc = launch_fuse(st, m->att.kfs, m->att.cap, W.hdr + MAP_HDR_SLOT, W.cam, W.mps,
                                 W.mdesc, W.hdr + MAP_HDR_N, W.ncap, 1, th, c->scale, c->inv_sigma2,
                                 c->p.nlevels, 0, W.bidx, W.bdist, W.hdr + MAP_HDR_SEARCH, c->d_err));
    if (rc == -95) return set_err(ORBG_ENOTSUP, "Fuse: more than 8192 keypoints per KeyFrame");
    if (rc) return set_err(ORBG_EIO, "k_fuse launch failed");
    PROF_LAUNCH(c, "map_fuse_update",
                rc = launch_map_fuse_update(st, m->D, W, d_ids, nmax, ++m->epoch, d_best_idx,
                                            d_best_dist, d_status, d_nfused, at_ntargets));
    if (rc) return set_err(rc, "k_fuse_update launch failed");
    m->dirty = m->touched = true;
    return map_distinctive(c, m, W.surv, nmax, W.hdr + MAP_HDR_N);
}

extern "C" int orbg_map_fuse_device(orbg_ctx *c, orbg_map *m, int slot, const int32_t *d_point_ids,
                                    int n, float th, int32_t *d_best_idx, int32_t *d_best_dist,
                                    int32_t *d_status, int32_t *d_nfused)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (!d_nfused) return set_err(ORBG_EINVAL, "NULL device array");
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_nfused, 0, 4, c->stream));
        return ORBG_OK;
    }
    if (!d_point_ids) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, n))) return rc;
    return map_fuse_core(c, m, slot, d_point_ids, n, n, 0, slot, th, d_best_idx, d_best_dist, d_status,
                         d_nfused, 0);
}

extern "C" int orbg_map_fuse(orbg_ctx *c, orbg_map *m, int slot, const int32_t *point_ids, int n,
                             float th, int32_t *best_idx, int32_t *best_dist, int32_t *status,
                             int32_t *nfused)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || !nfused || (n && !point_ids)) return set_err(ORBG_EINVAL, "negative size / NULL array");
    const size_t nb = (size_t)std::max(n, 1) * 4;
    Layout L;
    const size_t o_p = L.take(nb), o_bi = L.take(nb), o_bd = L.take(nb), o_st = L.take(nb);
    const size_t o_n = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(b + o_p, point_ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_fuse_device(c, m, slot, L.at<int32_t>(b, o_p), n, th, L.at<int32_t>(b, o_bi),
                                   L.at<int32_t>(b, o_bd), L.at<int32_t>(b, o_st),
                                   L.at<int32_t>(b, o_n))))
        return rc;
    HIPCHK(hipMemcpyAsync(nfused, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (n && best_idx) HIPCHK(hipMemcpyAsync(best_idx, b + o_bi, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (n && best_dist) HIPCHK(hipMemcpyAsync(best_dist, b + o_bd, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (n && status) HIPCHK(hipMemcpyAsync(status, b + o_st, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

extern "C" int orbg_map_search_in_neighbors_device(orbg_ctx *c, orbg_map *m, int slot,
                                                   int current_kf_id, int monocular, float th,
                                                   int32_t *d_targets, int target_cap,
                                                   int32_t *d_ntargets, int32_t *d_nfused)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if ((rc = map_attached(m))) return rc;
    if (target_cap < 0 || !d_ntargets || !d_nfused || (target_cap && !d_targets))
        return set_err(ORBG_EINVAL, "bad target_cap / NULL device array");
    const int bound = monocular ? ORBG_MAP_MAX_TARGETS : ORBG_MAP_MAX_TARGETS / 2;  // nn + 5 nn
    if ((rc = map_edit_ws(c, m, ORBG_MAP_MAX_TARGETS * m->D.cap))) return rc;
    const MapEditWs &W = m->W;
    hipStream_t st = c->stream;
    if (launch_map_sin_targets(st, m->D, W, slot, current_kf_id, monocular != 0, d_targets, target_cap,
                               d_ntargets, d_nfused))
        return set_err(ORBG_EIO, "k_sin_targets launch failed");
    m->touched = true;
    for (int t = 0; t < bound; t++)
        if ((rc = map_fuse_core(c, m, -1, W.snap, 0, m->D.cap, t, slot, th, nullptr, nullptr, nullptr,
                                d_nfused + t, 0)))
            return rc;
    if (launch_map_sin_candidates(st, m->D, W)) return set_err(ORBG_EIO, "k_sin_candidates launch failed");
    if ((rc = map_fuse_core(c, m, -1, W.ids, 0, W.ncap, ORBG_MAP_MAX_TARGETS, slot, th, nullptr, nullptr,
                            nullptr, d_nfused, 1)))
        return rc;
    // ComputeDistinctiveDescriptors and UpdateNormalAndDepth of the row as it stands now
    if (launch_map_sin_row(st, m->D, W, slot)) return set_err(ORBG_EIO, "k_sin_row launch failed");
    if ((rc = map_distinctive(c, m, W.snap, m->D.cap, nullptr))) return rc;
    if ((rc = orbg_map_update_normal_and_depth_batch_device(c, m, W.snap, m->D.cap))) return rc;
    return orbg_map_update_connections_batch_device(c, m, W.hdr + MAP_HDR_CUR, 1);
}

extern "C" int orbg_map_search_in_neighbors(orbg_ctx *c, orbg_map *m, int slot, int current_kf_id,
                                            int monocular, float th, int32_t *targets,
                                            int target_cap, int32_t *ntargets, int32_t *nfused)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (target_cap < 0 || !ntargets || !nfused || (target_cap && !targets))
        return set_err(ORBG_EINVAL, "bad target_cap / NULL array");
    Layout L;
    const size_t o_t = L.take((size_t)target_cap * 4), o_n = L.take(4);
    const size_t o_f = L.take((ORBG_MAP_MAX_TARGETS + 1) * 4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    if ((rc = orbg_map_search_in_neighbors_device(c, m, slot, current_kf_id, monocular, th,
                                                  L.at<int32_t>(b, o_t), target_cap,
                                                  L.at<int32_t>(b, o_n), L.at<int32_t>(b, o_f))))
        return rc;
    int32_t nt = 0;
    HIPCHK(hipMemcpyAsync(&nt, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nfused, b + o_f, (ORBG_MAP_MAX_TARGETS + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(nt, target_cap);
    if (nw > 0) HIPCHK(hipMemcpy(targets, b + o_t, (size_t)nw * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *ntargets = nt;
    if (nt > target_cap) return set_err(ORBG_ERANGE, "%d target entries (target_cap %d)", nt, target_cap);
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints / ProcessNewKeyFrame on the Map (map_create_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_map_attach_keyframe_geometry(orbg_ctx *c, orbg_map *m,
                                                 const orbg_keypoint *d_kps_raw,
                                                 const float *d_depth,
                                                 const orbg_kf_camera *d_kf_cams)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (!d_kf_cams && (d_kps_raw || d_depth))
        return set_err(ORBG_EINVAL, "NULL d_kf_cams beside other arrays");
    m->geom.kps_raw = d_kps_raw;
    m->geom.depth = d_depth;
    m->geom.cams = d_kf_cams;
    return ORBG_OK;
}

// the workspace of CreateNewMapPoints / ProcessNewKeyFrame for the attached row length
static int map_create_ws(orbg_ctx *c, orbg_map *m)
{
    const int acap = m->att.cap;
    if (m->d_cw && m->CW.acap == acap) return ORBG_OK;
    if (m->d_cw) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(m->d_cw));
        m->d_cw = nullptr;
        m->CW = MapCreateWs{};
    }
    const size_t K = (size_t)m->D.K, a = (size_t)acap, cap = (size_t)m->D.cap;
    Layout L;
    const size_t o_h = L.take(16 * 4), o_1 = L.take(ORBG_CNP_MAX_NEIGH * 4);
    const size_t o_2 = L.take(ORBG_CNP_MAX_NEIGH * 4), o_s = L.take(ORBG_CNP_MAX_NEIGH * 4);
    const size_t o_c = L.take(K * 4), o_f = L.take(K * 4), o_k = L.take(K * sizeof(orbg_kf_camera));
    const size_t o_m = L.take(K * a), o_g = L.take(ORBG_CNP_MAX_NEIGH * sizeof(orbg_triangulation_pair));
    const size_t o_ma = L.take(a * 4), o_nm = L.take(4), o_x = L.take(a * 12), o_t = L.take(a);
    const size_t o_nn = L.take(4), o_i = L.take((cap + 1) * 4), o_r = L.take(cap * 4), o_ce = L.take(12);
    const size_t o_v = L.take(a);
    if (hipMalloc(&m->d_cw, L.total()) != hipSuccess) {
        m->d_cw = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the CreateNewMapPoints workspace", L.total());
    }
    HIPCHK(hipMemsetAsync(m->d_cw, 0, L.total(), c->stream));
    uint8_t *b = (uint8_t *)m->d_cw;
    MapCreateWs &W = m->CW;
    W.acap = acap;
    W.hdr = L.at<int32_t>(b, o_h);
    W.kf1 = L.at<int32_t>(b, o_1);
    W.kf2 = L.at<int32_t>(b, o_2);
    W.nstat = L.at<int32_t>(b, o_s);
    W.counts = L.at<int32_t>(b, o_c);
    W.nfv = L.at<int32_t>(b, o_f);
    W.cams = L.at<orbg_kf_camera>(b, o_k);
    W.has_mp = b + o_m;
    W.geo = L.at<orbg_triangulation_pair>(b, o_g);
    W.match = L.at<int32_t>(b, o_ma);
    W.nm = L.at<int32_t>(b, o_nm);
    W.x3d = L.at<float>(b, o_x);
    W.tst = L.at<int8_t>(b, o_t);
    W.nnew = L.at<int32_t>(b, o_nn);
    W.ids = L.at<int32_t>(b, o_i);
    W.row = L.at<int32_t>(b, o_r);
    W.centre = L.at<float>(b, o_ce);
    W.virt = b + o_v;
    return ORBG_OK;
}

// ComputeDistinctiveDescriptors and UpdateNormalAndDepth of W.ids (their count behind them)
static int map_create_update(orbg_ctx *c, orbg_map *m)
{
    const MapCreateWs &W = m->CW;
    int rc = map_distinctive(c, m, W.ids, m->D.cap, W.ids + m->D.cap);
    if (rc) return rc;
    return orbg_map_update_normal_and_depth_batch_device(c, m, W.ids, m->D.cap);
}

extern "C" int orbg_map_create_new_points_device(orbg_ctx *c, orbg_map *m, int slot,
                                                 int current_kf_id, int monocular, int first_id,
                                                 const int32_t *d_abort, int32_t *d_recent,
                                                 int recent_cap, int32_t *d_nrecent,
                                                 int32_t *d_neigh, int32_t *d_neigh_status,
                                                 int32_t *d_nmatches, int32_t *d_nnew,
                                                 int8_t *d_tri_status, int32_t *d_out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if ((rc = map_attached(m))) return rc;
    if (!m->geom.cams)
        return set_err(ORBG_EINVAL, "no keyframe geometry attached (orbg_map_attach_keyframe_geometry)");
    const orbg_keyframes &ak = m->att.kfs;
    if (!ak.fv_nodes || !ak.fv_off || !ak.fv_feats || !ak.nfv)
        return set_err(ORBG_EINVAL, "the attached keyframes carry no FeatureVector (fv_* NULL)");
    if (ak.uright && !m->geom.depth) return set_err(ORBG_EINVAL, "mvuRight attached without mvDepth");
    if (first_id < 0 || recent_cap < 0) return set_err(ORBG_EINVAL, "negative first_id / recent_cap");
    if (!d_nrecent || !d_neigh || !d_neigh_status || !d_nmatches || !d_nnew || !d_out ||
        (recent_cap && !d_recent))
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, m->D.cap))) return rc;
    if ((rc = map_create_ws(c, m))) return rc;
    const MapCreateWs &W = m->CW;
    const int acap = W.acap, nn = monocular ? ORBG_CNP_MAX_NEIGH : ORBG_CNP_MAX_NEIGH / 2;
    hipStream_t st = c->stream;
    HIPCHK(hipMemsetAsync(d_nmatches, 0, ORBG_CNP_MAX_NEIGH * 4, st));
    HIPCHK(hipMemsetAsync(d_nnew, 0, ORBG_CNP_MAX_NEIGH * 4, st));
    PROF_LAUNCH(c, "map_cnp_neighbours",
                rc = launch_map_cnp_neighbours(st, m->D, m->att, m->geom, W, slot, monocular != 0,
                                               d_nrecent, d_neigh));
    if (rc) return set_err(rc, "k_cnp_neigh launch failed");
    m->touched = true;
    if (launch_tri_geometry(st, W.cams, W.kf1, W.kf2, ORBG_CNP_MAX_NEIGH, W.geo))
        return set_err(ORBG_EIO, "k_tri_geometry launch failed");
    orbg_keyframes K = ak;  // the attached arrays with the rows' has_mp and the clamped counts
    K.has_mp = W.has_mp;
    K.counts = W.counts;
    K.nfv = W.nfv;
    for (int i = 0; i < nn; i++) {
        if (launch_map_cnp_pair(st, m->D, m->att, W, slot, i, d_abort))
            return set_err(ORBG_EIO, "k_cnp_pair launch failed");
        PROF_LAUNCH(c, "map_cnp_match",
                    rc = launch_tri_match(st, K, acap, W.kf1 + i, W.kf2 + i, W.geo + i, 1, c->scale,
                                          c->sigma2, c->p.nlevels, 0, 0, W.match, W.nm));
        if (rc == -95) return set_err(ORBG_ENOTSUP, "SearchForTriangulation: more than 65535 features");
        if (rc) return set_err(ORBG_EIO, "k_tri_match launch failed");
        PROF_LAUNCH(c, "map_cnp_triangulate",
                    rc = launch_triangulate(st, K, m->geom.kps_raw, m->geom.depth, acap, W.cams,
                                            W.kf1 + i, W.kf2 + i, W.match, 1, c->scale, c->sigma2,
                                            c->p.nlevels, c->p.scale_factor, W.x3d, W.tst, W.nnew));
        if (rc) return set_err(ORBG_EIO, "k_triangulate launch failed");
        PROF_LAUNCH(c, "map_cnp_insert",
                    rc = launch_map_cnp_insert(st, m->D, W, slot, i, current_kf_id, first_id, d_recent,
                                               recent_cap, d_nrecent, d_nmatches, d_nnew,
                                               d_tri_status));
        if (rc) return set_err(rc, "k_cnp_insert launch failed");
    }
    if (d_tri_status && nn < ORBG_CNP_MAX_NEIGH)
        HIPCHK(hipMemsetAsync(d_tri_status + (size_t)nn * m->D.cap, 0,
                              (size_t)(ORBG_CNP_MAX_NEIGH - nn) * m->D.cap, st));
    if (launch_map_cnp_finish(st, m->D, W, first_id, d_neigh_status, d_out))
        return set_err(ORBG_EIO, "k_cnp_finish launch failed");
    m->dirty = true;
    return map_create_update(c, m);
}

extern "C" int orbg_map_create_new_points(orbg_ctx *c, orbg_map *m, int slot, int current_kf_id,
                                          int monocular, int first_id, const int32_t *abort,
                                          int32_t *recent, int recent_cap, int32_t *nrecent,
                                          int32_t *neigh, int32_t *neigh_status, int32_t *nmatches,
                                          int32_t *nnew, int8_t *tri_status, int32_t *out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (recent_cap < 0 || !nrecent || !neigh || !neigh_status || !nmatches || !nnew || !out ||
        (recent_cap && !recent))
        return set_err(ORBG_EINVAL, "bad recent_cap / NULL array");
    const int n0 = *nrecent;
    if (n0 < 0 || n0 > recent_cap) return set_err(ORBG_EINVAL, "*nrecent %d outside [0, %d]", n0, recent_cap);
    const size_t nb = ORBG_CNP_MAX_NEIGH * 4, ts = (size_t)ORBG_CNP_MAX_NEIGH * m->D.cap;
    Layout L;
    const size_t o_r = L.take((size_t)recent_cap * 4), o_n = L.take(4), o_a = L.take(4);
    const size_t o_g = L.take(nb), o_s = L.take(nb), o_m = L.take(nb), o_w = L.take(nb);
    const size_t o_o = L.take(16), o_t = L.take(ts);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t ab = abort ? *abort : 0;
    if (n0) HIPCHK(hipMemcpyAsync(b + o_r, recent, (size_t)n0 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &n0, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_a, &ab, 4, hipMemcpyHostToDevice, c->stream));
    rc = orbg_map_create_new_points_device(
        c, m, slot, current_kf_id, monocular, first_id, abort ? L.at<int32_t>(b, o_a) : nullptr,
        L.at<int32_t>(b, o_r), recent_cap, L.at<int32_t>(b, o_n), L.at<int32_t>(b, o_g),
        L.at<int32_t>(b, o_s), L.at<int32_t>(b, o_m), L.at<int32_t>(b, o_w),
        tri_status ? L.at<int8_t>(b, o_t) : nullptr, L.at<int32_t>(b, o_o));
    if (rc) {
        hipStreamSynchronize(c->stream);  // the copies above read the caller's stack
        return rc;
    }
    int32_t n1 = 0;
    HIPCHK(hipMemcpyAsync(&n1, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(neigh, b + o_g, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(neigh_status, b + o_s, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nmatches, b + o_m, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nnew, b + o_w, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out, b + o_o, 16, hipMemcpyDeviceToHost, c->stream));
    if (tri_status) HIPCHK(hipMemcpyAsync(tri_status, b + o_t, ts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n1 > n0) HIPCHK(hipMemcpy(recent + n0, b + o_r + (size_t)n0 * 4, (size_t)(n1 - n0) * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *nrecent = n1;
    if (out[3] & ORBG_CNP_DEAD) return set_err(ORBG_EINVAL, "slot %d is not live", slot);
    if (out[3] & ORBG_CNP_NO_POSE) return set_err(ORBG_EINVAL, "slot %d has no stored pose", slot);
    if (out[3] & (ORBG_CNP_POINT_RANGE | ORBG_CNP_RECENT_RANGE))
        return set_err(ORBG_ERANGE, "%d new points, %d created (max_points %d, recent_cap %d)", out[2],
                       out[1], m->D.P, recent_cap);
    return ORBG_OK;
}

extern "C" int orbg_map_process_new_keyframe_device(orbg_ctx *c, orbg_map *m, int slot,
                                                    const int32_t *d_point_ids,
                                                    const uint8_t *d_octaves,
                                                    const uint8_t *d_feat_flags, int n,
                                                    const float *d_Tcw, int mnid, int kf_flags,
                                                    const uint8_t *d_in_keyframe, int32_t *d_recent,
                                                    int recent_cap, int32_t *d_nrecent,
                                                    int32_t *d_out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if ((rc = map_attached(m))) return rc;
    if (n < 0 || n > m->D.cap) return set_err(ORBG_EINVAL, "%d features (kf_cap %d)", n, m->D.cap);
    if (recent_cap < 0) return set_err(ORBG_EINVAL, "negative recent_cap");
    if (!d_Tcw || !d_nrecent || !d_out || (recent_cap && !d_recent) || (n && (!d_point_ids || !d_octaves)))
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, m->D.cap))) return rc;
    if ((rc = map_create_ws(c, m))) return rc;
    const MapCreateWs &W = m->CW;
    const MapDev &D = m->D;
    hipStream_t st = c->stream;
    if (launch_map_pnk_prepare(st, D, W, slot, d_point_ids, n, d_Tcw, mnid, kf_flags, d_in_keyframe,
                               d_recent, recent_cap, d_nrecent, d_out))
        return set_err(ORBG_EIO, "k_pnk_prepare launch failed");
    m->touched = true;
    const int32_t *h = W.hdr;
    if (launch_map_set_keyframes(st, D, h + CNP_HDR_SLOT, 1, W.row, n ? d_octaves : (const uint8_t *)W.row,
                                 D.cap, h + CNP_HDR_N, W.centre, h + CNP_HDR_FLAGS))
        return set_err(ORBG_EIO, "k_map_set_kf launch failed");
    if (d_feat_flags && launch_map_set_features(st, D, h + CNP_HDR_SLOT, 1, d_feat_flags, D.cap, h + CNP_HDR_N))
        return set_err(ORBG_EIO, "k_map_set_features launch failed");
    if (launch_map_set_poses(st, D, h + CNP_HDR_SLOT, 1, d_Tcw, h + CNP_HDR_MNID))
        return set_err(ORBG_EIO, "k_loop_set_poses launch failed");
    m->dirty = m->tree_dirty = true;
    if ((rc = map_create_update(c, m))) return rc;
    return orbg_map_update_connections_batch_device(c, m, h + CNP_HDR_SLOT, 1);
}

extern "C" int orbg_map_process_new_keyframe(orbg_ctx *c, orbg_map *m, int slot,
                                             const int32_t *point_ids, const uint8_t *octaves,
                                             const uint8_t *feat_flags, int n, const float *Tcw,
                                             int mnid, int kf_flags, const uint8_t *in_keyframe,
                                             int32_t *recent, int recent_cap, int32_t *nrecent,
                                             int32_t *out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || n > m->D.cap) return set_err(ORBG_EINVAL, "%d features (kf_cap %d)", n, m->D.cap);
    if (recent_cap < 0 || !Tcw || !nrecent || !out || (recent_cap && !recent) ||
        (n && (!point_ids || !octaves)))
        return set_err(ORBG_EINVAL, "bad recent_cap / NULL array");
    const int n0 = *nrecent;
    if (n0 < 0 || n0 > recent_cap) return set_err(ORBG_EINVAL, "*nrecent %d outside [0, %d]", n0, recent_cap);
    const size_t cn = (size_t)std::max(n, 1);
    Layout L;
    const size_t o_p = L.take(cn * 4), o_o = L.take(cn), o_f = L.take(cn), o_k = L.take(cn);
    const size_t o_T = L.take(48), o_r = L.take((size_t)recent_cap * 4), o_n = L.take(4), o_out = L.take(16);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    hipStream_t st = c->stream;
    if (n) {
        HIPCHK(hipMemcpyAsync(b + o_p, point_ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_o, octaves, (size_t)n, hipMemcpyHostToDevice, st));
        if (feat_flags) HIPCHK(hipMemcpyAsync(b + o_f, feat_flags, (size_t)n, hipMemcpyHostToDevice, st));
        if (in_keyframe) HIPCHK(hipMemcpyAsync(b + o_k, in_keyframe, (size_t)n, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(b + o_T, Tcw, 48, hipMemcpyHostToDevice, st));
    if (n0) HIPCHK(hipMemcpyAsync(b + o_r, recent, (size_t)n0 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b + o_n, &n0, 4, hipMemcpyHostToDevice, st));
    rc = orbg_map_process_new_keyframe_device(
        c, m, slot, L.at<int32_t>(b, o_p), b + o_o, (n && feat_flags) ? b + o_f : nullptr, n,
        L.at<float>(b, o_T), mnid, kf_flags, (n && in_keyframe) ? b + o_k : nullptr,
        L.at<int32_t>(b, o_r), recent_cap, L.at<int32_t>(b, o_n), L.at<int32_t>(b, o_out));
    if (rc) {
        hipStreamSynchronize(st);
        return rc;
    }
    int32_t n1 = 0;
    HIPCHK(hipMemcpyAsync(&n1, b + o_n, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out, b + o_out, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n1 > n0) HIPCHK(hipMemcpy(recent + n0, b + o_r + (size_t)n0 * 4, (size_t)(n1 - n0) * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *nrecent = n1;
    if (out[3] & ORBG_CNP_RECENT_RANGE)
        return set_err(ORBG_ERANGE, "%d ids for the recent list, %d appended (recent_cap %d)", out[2],
                       out[0], recent_cap);
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// LoopClosing::CorrectLoop on the Map (map_loop_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_map_set_keyframe_poses_device(orbg_ctx *c, orbg_map *m, const int32_t *d_slots,
                                                  int n, const float *d_Tcw, const int32_t *d_mnid)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_slots || (!d_Tcw && !d_mnid)) return set_err(ORBG_EINVAL, "NULL device array");
    if (launch_map_set_poses(c->stream, m->D, d_slots, n, d_Tcw, d_mnid))
        return set_err(ORBG_EIO, "k_loop_set_poses launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_set_keyframe_poses(orbg_ctx *c, orbg_map *m, const int32_t *slots, int n,
                                           const float *Tcw, const int32_t *mnid)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!slots || (!Tcw && !mnid)) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < n; i++)
        if ((rc = map_slot_ok(m, slots[i]))) return rc;
    Layout L;
    const size_t o_s = L.take((size_t)n * 4), o_t = L.take((size_t)n * 48), o_i = L.take((size_t)n * 4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_s, slots, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (Tcw) HIPCHK(hipMemcpyAsync(b + o_t, Tcw, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
    if (mnid) HIPCHK(hipMemcpyAsync(b + o_i, mnid, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_set_keyframe_poses_device(c, m, L.at<int32_t>(b, o_s), n,
                                                 Tcw ? L.at<float>(b, o_t) : nullptr,
                                                 mnid ? L.at<int32_t>(b, o_i) : nullptr)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_get_keyframe_poses(orbg_ctx *c, orbg_map *m, int first, int n, float *Tcw,
                                           int32_t *has_pose, int32_t *mnid, float *centres)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || first < 0 || (int64_t)first + n > m->D.K)
        return set_err(ORBG_EINVAL, "slots %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.K);
    if (n == 0) return ORBG_OK;
    const MapDev &D = m->D;
    if (Tcw) HIPCHK(hipMemcpyAsync(Tcw, D.kf_Tcw + (size_t)first * 12, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream));
    if (has_pose) HIPCHK(hipMemcpyAsync(has_pose, D.kf_pose + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (mnid) HIPCHK(hipMemcpyAsync(mnid, D.kf_mnid + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (centres) HIPCHK(hipMemcpyAsync(centres, D.kf_centre + (size_t)first * 3, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_add_loop_edge(orbg_ctx *c, orbg_map *m, int a, int b)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, a)) || (rc = map_slot_ok(m, b))) return rc;
    if (a == b) return set_err(ORBG_EINVAL, "a loop edge from slot %d to itself", a);
    Layout L;
    const size_t o_s = L.take(4);
    uint8_t *d;
    if ((rc = L.device(c, &d))) return rc;
    if (launch_map_add_loop_edge(c->stream, m->D, a, b, L.at<int32_t>(d, o_s)))
        return set_err(ORBG_EIO, "k_loop_add_edge launch failed");
    m->touched = true;
    int32_t st = 0;
    HIPCHK(hipMemcpyAsync(&st, d + o_s, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st) return set_err(ORBG_ERANGE, "more than %d loop edges at slot %d or %d", ORBG_MAP_MAX_LOOP_EDGES, a, b);
    return ORBG_OK;
}

extern "C" int orbg_map_get_loop_edges(orbg_ctx *c, orbg_map *m, int slot, int32_t *slots, int cap,
                                       int32_t *n)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (cap < 0 || !n || (cap && !slots)) return set_err(ORBG_EINVAL, "bad cap / NULL array");
    int32_t cnt = 0, e[ORBG_MAP_MAX_LOOP_EDGES];
    HIPCHK(hipMemcpyAsync(&cnt, m->D.le_n + slot, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(e, m->D.le_slot + (size_t)slot * ORBG_MAP_MAX_LOOP_EDGES, sizeof(e),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::sort(e, e + cnt);  // a std::set<KeyFrame*>: ascending slot
    for (int i = 0; i < std::min(cnt, cap); i++) slots[i] = e[i];
    *n = cnt;
    if (cnt > cap) return set_err(ORBG_ERANGE, "%d loop edges (cap %d)", cnt, cap);
    return ORBG_OK;
}

extern "C" int orbg_map_get_point_corrected(orbg_ctx *c, orbg_map *m, int first, int n,
                                            int32_t *corrected_by_kf, int32_t *corrected_reference)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (!corrected_by_kf || !corrected_reference) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(corrected_by_kf, m->D.mp_corr_kf + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(corrected_reference, m->D.mp_corr_ref + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

extern "C" int orbg_map_set_point_corrected(orbg_ctx *c, orbg_map *m, int first, int n,
                                            const int32_t *corrected_by_kf,
                                            const int32_t *corrected_reference)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_range_ok(m, first, n))) return rc;
    if (n == 0) return ORBG_OK;
    if (!corrected_by_kf || !corrected_reference) return set_err(ORBG_EINVAL, "NULL array");
    Layout L;
    const size_t o_a = L.take((size_t)n * 4), o_b = L.take((size_t)n * 4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_a, corrected_by_kf, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_b, corrected_reference, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (launch_map_set_corrected(c->stream, m->D, first, n, L.at<int32_t>(b, o_a), L.at<int32_t>(b, o_b)))
        return set_err(ORBG_EIO, "k_loop_set_corrected launch failed");
    m->touched = true;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

static int map_set_cap_ok(const orbg_map *m, int set_cap)
{
    if (set_cap < 1) return set_err(ORBG_EINVAL, "set_cap < 1");
    if (set_cap > ORBG_MAP_MAX_LOOP_SET)
        return set_err(ORBG_ENOTSUP, "set_cap %d (> %d)", set_cap, ORBG_MAP_MAX_LOOP_SET);
    return ORBG_OK;
}

extern "C" int orbg_map_propagate_device(orbg_ctx *c, orbg_map *m, int cur, const orbg_sim3d *d_Scw,
                                         int32_t *d_set, int set_cap, int32_t *d_nset,
                                         orbg_sim3d *d_corrected, orbg_sim3d *d_noncorrected,
                                         int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur))) return rc;
    if ((rc = map_set_cap_ok(m, set_cap))) return rc;
    if (!d_Scw || !d_set || !d_nset || !d_corrected || !d_noncorrected || !d_status)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    MapScales S{};
    S.nlevels = std::min(std::max(c->p.nlevels, 1), 16);
    for (int i = 0; i < 16; i++) S.scale[i] = c->scale[i];
    if ((rc = launch_map_propagate(c->stream, m->D, cur, d_Scw, d_set, set_cap, d_nset, d_corrected,
                                   d_noncorrected, d_status, S, &m->epoch, &c->prof)))
        return set_err(rc, "Propagate launch failed");
    m->tree_dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_propagate(orbg_ctx *c, orbg_map *m, int cur, const orbg_sim3d *Scw,
                                  int32_t *set, int set_cap, int32_t *nset, orbg_sim3d *corrected,
                                  orbg_sim3d *noncorrected)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur))) return rc;
    if ((rc = map_set_cap_ok(m, set_cap))) return rc;
    if (!Scw || !set || !nset || !corrected || !noncorrected) return set_err(ORBG_EINVAL, "NULL array");
    const size_t K = (size_t)m->D.K;
    Layout L;
    const size_t o_s = L.take(sizeof(orbg_sim3d)), o_e = L.take((size_t)set_cap * 4), o_n = L.take(4);
    const size_t o_c = L.take(K * sizeof(orbg_sim3d)), o_u = L.take(K * sizeof(orbg_sim3d));
    const size_t o_st = L.take(16);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    HIPCHK(hipMemcpyAsync(b + o_s, Scw, sizeof(orbg_sim3d), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(b + o_c, 0, K * sizeof(orbg_sim3d), c->stream));
    HIPCHK(hipMemsetAsync(b + o_u, 0, K * sizeof(orbg_sim3d), c->stream));
    if ((rc = orbg_map_propagate_device(c, m, cur, L.at<orbg_sim3d>(b, o_s), L.at<int32_t>(b, o_e),
                                        set_cap, L.at<int32_t>(b, o_n), L.at<orbg_sim3d>(b, o_c),
                                        L.at<orbg_sim3d>(b, o_u), L.at<int32_t>(b, o_st))))
        return rc;
    int32_t st[4] = {0, 0, 0, 0}, ns = 0;
    HIPCHK(hipMemcpyAsync(st, b + o_st, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&ns, b + o_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    if (st[0] & ORBG_LOOP_DEAD) return set_err(ORBG_EINVAL, "Propagate: slot %d is not a live keyframe", cur);
    if (st[0] & ORBG_LOOP_SET_RANGE)
        return set_err(ORBG_ERANGE, "Propagate: %d connected keyframes (set_cap %d)", st[1], set_cap);
    if (st[0] & ORBG_LOOP_NO_POSE)
        return set_err(ORBG_EINVAL, "Propagate: a connected keyframe has no pose");
    HIPCHK(hipMemcpy(set, b + o_e, (size_t)ns * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(corrected, b + o_c, K * sizeof(orbg_sim3d), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(noncorrected, b + o_u, K * sizeof(orbg_sim3d), hipMemcpyDeviceToHost));
    *nset = ns;
    return ORBG_OK;
}

extern "C" int orbg_map_loop_connections_device(orbg_ctx *c, orbg_map *m, const int32_t *d_set,
                                                int set_cap, const int32_t *d_nset, int32_t *d_pairs,
                                                int pair_cap, int32_t *d_npairs)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_set_cap_ok(m, set_cap))) return rc;
    if (pair_cap < 0 || !d_set || !d_nset || !d_npairs || (pair_cap && !d_pairs))
        return set_err(ORBG_EINVAL, "bad pair_cap / NULL device array");
    const size_t K = (size_t)m->D.K, rows = ORBG_MAP_MAX_LOOP_SET * K * 2;
    if (!m->d_lc) {
        if (hipMalloc(&m->d_lc, rows + ORBG_MAP_MAX_LOOP_SET * 4) != hipSuccess) {
            m->d_lc = nullptr;
            return set_err(ORBG_ENOMEM, "LoopConnections: hipMalloc(%zu bytes)", rows + ORBG_MAP_MAX_LOOP_SET * 4);
        }
    }
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if ((rc = launch_map_loop_connections(c->stream, m->D, d_set, set_cap, d_nset, (uint16_t *)m->d_lc,
                                          (int32_t *)((uint8_t *)m->d_lc + rows), d_pairs, pair_cap,
                                          d_npairs, &m->epoch, &c->prof)))
        return set_err(rc, "LoopConnections launch failed");
    m->tree_dirty = m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_loop_connections(orbg_ctx *c, orbg_map *m, const int32_t *set, int nset,
                                         int32_t *pairs, int pair_cap, int32_t *npairs)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_set_cap_ok(m, nset))) return rc;
    if (pair_cap < 0 || !set || !npairs || (pair_cap && !pairs))
        return set_err(ORBG_EINVAL, "bad pair_cap / NULL array");
    for (int i = 0; i < nset; i++)
        if ((rc = map_slot_ok(m, set[i]))) return rc;
    Layout L;
    const size_t o_e = L.take((size_t)nset * 4), o_n = L.take(8), o_p = L.take((size_t)pair_cap * 8);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[2] = {nset, 0};
    HIPCHK(hipMemcpyAsync(b + o_e, set, (size_t)nset * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, hdr, 8, hipMemcpyHostToDevice, c->stream));
    int32_t *dn = L.at<int32_t>(b, o_n);
    if ((rc = orbg_map_loop_connections_device(c, m, L.at<int32_t>(b, o_e), nset, dn,
                                               L.at<int32_t>(b, o_p), pair_cap, dn + 1)))
        return rc;
    int32_t np = 0;
    HIPCHK(hipMemcpyAsync(&np, dn + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    const int nw = std::min(np, pair_cap);
    if (nw > 0) HIPCHK(hipMemcpy(pairs, b + o_p, (size_t)nw * 8, hipMemcpyDeviceToHost));
    *npairs = np;
    if (np > pair_cap) return set_err(ORBG_ERANGE, "%d LoopConnections pairs (pair_cap %d)", np, pair_cap);
    return ORBG_OK;
}

extern "C" int orbg_map_essential_graph_device(orbg_ctx *c, orbg_map *m, int cur, int loop,
                                               const orbg_sim3d *d_corrected,
                                               const orbg_sim3d *d_noncorrected,
                                               const int32_t *d_set, int set_cap,
                                               const int32_t *d_nset, const int32_t *d_pairs,
                                               int pair_cap, const int32_t *d_npairs,
                                               int32_t *d_vert_slot, int32_t *d_nvert,
                                               int32_t *d_fixed, orbg_sim3d *d_Scw, orbg_sim3d *d_Snc,
                                               orbg_eg_edge *d_edges, int edge_cap, int32_t *d_nedge,
                                               int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur)) || (rc = map_slot_ok(m, loop))) return rc;
    if (cur == loop) return set_err(ORBG_EINVAL, "cur and loop are both slot %d", cur);
    if ((rc = map_set_cap_ok(m, set_cap))) return rc;
    if (pair_cap < 0 || edge_cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!d_corrected || !d_noncorrected || !d_set || !d_nset || !d_npairs || (pair_cap && !d_pairs) ||
        !d_vert_slot || !d_nvert || !d_fixed || !d_Scw || !d_Snc || (edge_cap && !d_edges) ||
        !d_nedge || !d_status)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = launch_map_essential_graph(c->stream, m->D, cur, loop, d_corrected, d_noncorrected, d_set,
                                         set_cap, d_nset, d_pairs, pair_cap, d_npairs, d_vert_slot,
                                         d_nvert, d_fixed, d_Scw, d_Snc, d_edges, edge_cap, d_nedge,
                                         d_status)))
        return set_err(rc, "essential graph assembly launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_essential_graph(orbg_ctx *c, orbg_map *m, int cur, int loop,
                                        const orbg_sim3d *corrected, const orbg_sim3d *noncorrected,
                                        const int32_t *set, int nset, const int32_t *pairs,
                                        int npairs, int32_t *vert_slot, int32_t *nvert,
                                        int32_t *fixed, orbg_sim3d *Scw, orbg_sim3d *Snc,
                                        orbg_eg_edge *edges, int edge_cap, int32_t *nedge,
                                        int32_t *nskipped)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur)) || (rc = map_slot_ok(m, loop))) return rc;
    if (cur == loop) return set_err(ORBG_EINVAL, "cur and loop are both slot %d", cur);
    if ((rc = map_set_cap_ok(m, nset))) return rc;
    if (npairs < 0 || edge_cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (!corrected || !noncorrected || !set || (npairs && !pairs) || !vert_slot || !nvert || !fixed ||
        !Scw || !Snc || (edge_cap && !edges) || !nedge)
        return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < nset; i++)
        if ((rc = map_slot_ok(m, set[i]))) return rc;
    const size_t K = (size_t)m->D.K, sb = K * sizeof(orbg_sim3d);
    Layout L;
    const size_t o_c = L.take(sb), o_u = L.take(sb), o_e = L.take((size_t)nset * 4);
    const size_t o_p = L.take((size_t)npairs * 8), o_h = L.take(32);  // nset, npairs, nvert, fixed, nedge
    const size_t o_v = L.take(K * 4), o_sc = L.take(sb), o_sn = L.take(sb);
    const size_t o_ed = L.take((size_t)edge_cap * sizeof(orbg_eg_edge)), o_st = L.take(16);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[8] = {nset, npairs, 0, -1, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(b + o_c, corrected, sb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_u, noncorrected, sb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_e, set, (size_t)nset * 4, hipMemcpyHostToDevice, c->stream));
    if (npairs) HIPCHK(hipMemcpyAsync(b + o_p, pairs, (size_t)npairs * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_h, hdr, 32, hipMemcpyHostToDevice, c->stream));
    int32_t *h = L.at<int32_t>(b, o_h);
    if ((rc = orbg_map_essential_graph_device(
             c, m, cur, loop, L.at<orbg_sim3d>(b, o_c), L.at<orbg_sim3d>(b, o_u), L.at<int32_t>(b, o_e),
             nset, h, L.at<int32_t>(b, o_p), npairs, h + 1, L.at<int32_t>(b, o_v), h + 2, h + 3,
             L.at<orbg_sim3d>(b, o_sc), L.at<orbg_sim3d>(b, o_sn), L.at<orbg_eg_edge>(b, o_ed), edge_cap,
             h + 4, L.at<int32_t>(b, o_st))))
        return rc;
    int32_t out[8], st[4];
    HIPCHK(hipMemcpyAsync(out, h, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(st, b + o_st, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st[0] & ORBG_LOOP_DEAD) return set_err(ORBG_EINVAL, "essential graph: slot %d (loop) is not a vertex", loop);
    if (st[0] & ORBG_LOOP_NO_POSE) return set_err(ORBG_EINVAL, "essential graph: a keyframe has no pose");
    const int nv = out[2], ne = std::min(out[4], edge_cap);
    HIPCHK(hipMemcpy(vert_slot, b + o_v, (size_t)nv * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Scw, b + o_sc, (size_t)nv * sizeof(orbg_sim3d), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Snc, b + o_sn, (size_t)nv * sizeof(orbg_sim3d), hipMemcpyDeviceToHost));
    if (ne > 0) HIPCHK(hipMemcpy(edges, b + o_ed, (size_t)ne * sizeof(orbg_eg_edge), hipMemcpyDeviceToHost));
    *nvert = nv;
    *fixed = out[3];
    *nedge = out[4];
    if (nskipped) *nskipped = st[1];
    if (out[4] > edge_cap) return set_err(ORBG_ERANGE, "%d edges (edge_cap %d)", out[4], edge_cap);
    return ORBG_OK;
}

extern "C" int orbg_map_apply_correction_device(orbg_ctx *c, orbg_map *m, int cur,
                                                const int32_t *d_vert_slot, const int32_t *d_nvert,
                                                const orbg_sim3d *d_Scw, const orbg_sim3d *d_Siw,
                                                const float *d_Tiw)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur))) return rc;
    if (!d_vert_slot || !d_nvert || !d_Scw || !d_Siw || !d_Tiw) return set_err(ORBG_EINVAL, "NULL device array");
    const size_t P = (size_t)m->D.P;
    if (!m->d_ap && hipMalloc(&m->d_ap, P * 28) != hipSuccess) {
        m->d_ap = nullptr;
        return set_err(ORBG_ENOMEM, "apply correction: hipMalloc(%zu bytes)", P * 28);
    }
    float *pts = (float *)m->d_ap, *moved = pts + P * 3;
    int32_t *ref = (int32_t *)((uint8_t *)m->d_ap + P * 24);
    if (launch_map_apply_poses(c->stream, m->D, cur, d_vert_slot, d_nvert, d_Tiw, pts, ref))
        return set_err(ORBG_EIO, "k_apply_poses launch failed");
    m->touched = true;
    if (launch_eg_correct_points(c->stream, (const Sim3d *)d_Scw, (const Sim3d *)d_Siw, m->D.K, ref, pts,
                                 m->D.P, moved))
        return set_err(ORBG_EIO, "k_eg_correct_points launch failed");
    if (launch_map_scatter_points(c->stream, m->D, moved, ref))
        return set_err(ORBG_EIO, "k_apply_scatter launch failed");
    return orbg_map_update_normal_and_depth_batch_device(c, m, nullptr, m->D.P);
}

extern "C" int orbg_map_apply_correction(orbg_ctx *c, orbg_map *m, int cur, const int32_t *vert_slot,
                                         int nvert, const orbg_sim3d *Scw, const orbg_sim3d *Siw,
                                         const float *Tiw)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur))) return rc;
    if (nvert < 1 || nvert > m->D.K) return set_err(ORBG_EINVAL, "nvert %d outside [1, %d]", nvert, m->D.K);
    if (!vert_slot || !Scw || !Siw || !Tiw) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < nvert; i++)
        if ((rc = map_slot_ok(m, vert_slot[i]))) return rc;
    const size_t n = (size_t)nvert, sb = n * sizeof(orbg_sim3d);
    Layout L;
    const size_t o_v = L.take(n * 4), o_n = L.take(4), o_c = L.take(sb), o_s = L.take(sb);
    const size_t o_t = L.take(n * 48);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t nv = nvert;
    HIPCHK(hipMemcpyAsync(b + o_v, vert_slot, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &nv, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, Scw, sb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_s, Siw, sb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_t, Tiw, n * 48, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_apply_correction_device(c, m, cur, L.at<int32_t>(b, o_v), L.at<int32_t>(b, o_n),
                                               L.at<orbg_sim3d>(b, o_c), L.at<orbg_sim3d>(b, o_s),
                                               L.at<float>(b, o_t))))
        return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// ---- the loop fusion (:848-863) and SearchAndFuse (:944-992) ----
extern "C" int orbg_map_loop_fusion_device(orbg_ctx *c, orbg_map *m, int cur, const int32_t *d_matched,
                                           int n, int32_t *d_counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur))) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (!d_counts || (n && !d_matched)) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_edit_ws(c, m, m->D.cap))) return rc;
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    if (launch_map_loop_fusion(c->stream, m->D, cur, d_matched, n, ++m->epoch, m->W.surv, d_counts))
        return set_err(ORBG_EIO, "k_loop_fusion launch failed");
    m->dirty = m->touched = true;
    return map_distinctive(c, m, m->W.surv, m->D.cap, nullptr);
}

extern "C" int orbg_map_loop_fusion(orbg_ctx *c, orbg_map *m, int cur, const int32_t *matched, int n,
                                    int32_t *counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || !counts || (n && !matched)) return set_err(ORBG_EINVAL, "negative size / NULL array");
    Layout L;
    const size_t o_m = L.take((size_t)n * 4), o_c = L.take(8);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(b + o_m, matched, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_loop_fusion_device(c, m, cur, L.at<int32_t>(b, o_m), n, L.at<int32_t>(b, o_c))))
        return rc;
    HIPCHK(hipMemcpyAsync(counts, b + o_c, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

extern "C" int orbg_map_search_and_fuse_device(orbg_ctx *c, orbg_map *m, const int32_t *d_set,
                                               int set_cap, const int32_t *d_nset,
                                               const orbg_sim3d *d_corrected,
                                               const int32_t *d_loop_points, int n, float th,
                                               int32_t *d_counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_set_cap_ok(m, set_cap))) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if ((rc = map_attached(m))) return rc;
    if (!d_set || !d_nset || !d_corrected || !d_counts || (n && !d_loop_points))
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipMemsetAsync(d_counts, 0, 8, c->stream));
    m->touched = true;
    if (n == 0) return ORBG_OK;
    if ((rc = map_edit_ws(c, m, n))) return rc;
    const MapEditWs &W = m->W;
    hipStream_t st = c->stream;
    for (int r = 0; r < set_cap; r++) {  // the members in slot order, one after another
        if ((rc = orbg_map_rebuild(c, m))) return rc;
        if (launch_map_sf_job(st, m->D, m->att, W, d_set, set_cap, d_nset, r, d_corrected, n) ||
            launch_map_fuse_gather(st, m->D, W, d_loop_points, n))
            return set_err(ORBG_EIO, "k_sf_job launch failed");
        rc = launch_fuse(st, m->att.kfs, m->att.cap, W.hdr + MAP_HDR_SLOT, W.cam, W.mps, W.mdesc,
                         W.hdr + MAP_HDR_N, W.ncap, 1, th, c->scale, c->inv_sigma2, c->p.nlevels, 1,
                         W.bidx, W.bdist, W.hdr + MAP_HDR_SEARCH, c->d_err);
        if (rc == -95) return set_err(ORBG_ENOTSUP, "Fuse: more than 8192 keypoints per KeyFrame");
        if (rc) return set_err(ORBG_EIO, "k_fuse launch failed");
        if (launch_map_sf_update(st, m->D, W, d_loop_points, n, ++m->epoch, d_counts))
            return set_err(ORBG_EIO, "k_sf_update launch failed");
        m->dirty = true;
        if ((rc = map_distinctive(c, m, W.surv, n, W.hdr + MAP_HDR_N))) return rc;
    }
    return ORBG_OK;
}

extern "C" int orbg_map_search_and_fuse(orbg_ctx *c, orbg_map *m, const int32_t *set, int nset,
                                        const orbg_sim3d *corrected, const int32_t *loop_points,
                                        int n, float th, int32_t *counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_set_cap_ok(m, nset))) return rc;
    if (n < 0 || !set || !corrected || !counts || (n && !loop_points))
        return set_err(ORBG_EINVAL, "negative size / NULL array");
    if ((rc = map_attached(m))) return rc;
    for (int i = 0; i < nset; i++)
        if ((rc = map_slot_ok(m, set[i]))) return rc;
    const size_t sb = (size_t)m->D.K * sizeof(orbg_sim3d);
    Layout L;
    const size_t o_e = L.take((size_t)nset * 4), o_n = L.take(4), o_c = L.take(sb);
    const size_t o_p = L.take((size_t)n * 4), o_o = L.take(8);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t ns = nset;
    HIPCHK(hipMemcpyAsync(b + o_e, set, (size_t)nset * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &ns, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, corrected, sb, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(b + o_p, loop_points, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = orbg_map_search_and_fuse_device(c, m, L.at<int32_t>(b, o_e), nset, L.at<int32_t>(b, o_n),
                                              L.at<orbg_sim3d>(b, o_c), L.at<int32_t>(b, o_p), n, th,
                                              L.at<int32_t>(b, o_o))))
        return rc;
    HIPCHK(hipMemcpyAsync(counts, b + o_o, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

// ---- CorrectLoop in one call ----
extern "C" int orbg_map_correct_loop(orbg_ctx *c, orbg_map *m, int cur, int loop, const orbg_sim3d *Scw,
                                     const int32_t *matched, int nmatched, const int32_t *loop_points,
                                     int nloop, int fix_scale, orbg_lm_report *report, int32_t *counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, cur)) || (rc = map_slot_ok(m, loop))) return rc;
    if (cur == loop) return set_err(ORBG_EINVAL, "cur and loop are both slot %d", cur);
    if (nmatched < 0 || nloop < 0 || !Scw || !report || !counts || (nmatched && !matched) ||
        (nloop && !loop_points))
        return set_err(ORBG_EINVAL, "negative size / NULL array");
    if ((rc = map_attached(m))) return rc;
    const size_t K = (size_t)m->D.K, sb = K * sizeof(orbg_sim3d);
    const int set_cap = (int)std::min<size_t>(K, ORBG_MAP_MAX_LOOP_SET);
    const int pair_cap = (int)std::min<size_t>((size_t)set_cap * K, 1u << 20);
    const int edge_cap = (int)std::min<size_t>(K * 64, 1u << 22);
    Layout L;
    const size_t o_s = L.take(sizeof(orbg_sim3d)), o_m = L.take((size_t)nmatched * 4);
    const size_t o_l = L.take((size_t)nloop * 4), o_e = L.take((size_t)set_cap * 4), o_h = L.take(128);
    const size_t o_c = L.take(sb), o_u = L.take(sb), o_p = L.take((size_t)pair_cap * 8);
    const size_t o_v = L.take(K * 4), o_sc = L.take(sb), o_sn = L.take(sb), o_si = L.take(sb);
    const size_t o_t = L.take(K * 48), o_ed = L.take((size_t)edge_cap * sizeof(orbg_eg_edge));
    uint8_t *b = nullptr;
    if (hipMalloc((void **)&b, L.total()) != hipSuccess)
        return set_err(ORBG_ENOMEM, "CorrectLoop: hipMalloc(%zu bytes)", L.total());
    // h: 0 nset, 1 npairs, 2 nvert, 3 fixed, 4 nedge, 8.. propagate status, 12.. graph status,
    //    16.. fusion counts, 18.. SearchAndFuse counts
    int32_t *h = L.at<int32_t>(b, o_h);
    orbg_sim3d *dc = L.at<orbg_sim3d>(b, o_c), *du = L.at<orbg_sim3d>(b, o_u);
    int32_t *dset = L.at<int32_t>(b, o_e), *dp = L.at<int32_t>(b, o_p), *dv = L.at<int32_t>(b, o_v);
    orbg_eg_graph *g = nullptr;
    std::vector<orbg_eg_edge> edges;
    int32_t hh[32] = {0};
    auto body = [&]() -> int {
        int r;
        HIPCHK(hipMemsetAsync(b, 0, o_p, c->stream));
        HIPCHK(hipMemcpyAsync(b + o_s, Scw, sizeof(orbg_sim3d), hipMemcpyHostToDevice, c->stream));
        if (nmatched) HIPCHK(hipMemcpyAsync(b + o_m, matched, (size_t)nmatched * 4, hipMemcpyHostToDevice, c->stream));
        if (nloop) HIPCHK(hipMemcpyAsync(b + o_l, loop_points, (size_t)nloop * 4, hipMemcpyHostToDevice, c->stream));
        if ((r = orbg_map_propagate_device(c, m, cur, L.at<orbg_sim3d>(b, o_s), dset, set_cap, h, dc, du, h + 8))) return r;
        HIPCHK(hipMemcpyAsync(hh + 8, h + 8, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (hh[8] & ORBG_LOOP_DEAD) return set_err(ORBG_EINVAL, "CorrectLoop: slot %d is not a live keyframe", cur);
        if (hh[8] & ORBG_LOOP_SET_RANGE) return set_err(ORBG_ERANGE, "CorrectLoop: %d connected keyframes (at most %d)", hh[9], set_cap);
        if (hh[8] & ORBG_LOOP_NO_POSE) return set_err(ORBG_EINVAL, "CorrectLoop: a connected keyframe has no pose");
        if ((r = orbg_map_loop_fusion_device(c, m, cur, L.at<int32_t>(b, o_m), nmatched, h + 16))) return r;
        if ((r = orbg_map_search_and_fuse_device(c, m, dset, set_cap, h, dc, L.at<int32_t>(b, o_l), nloop, 4.0f, h + 18))) return r;
        if ((r = orbg_map_loop_connections_device(c, m, dset, set_cap, h, dp, pair_cap, h + 1))) return r;
        HIPCHK(hipMemcpyAsync(hh, h, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (hh[1] > pair_cap) return set_err(ORBG_ERANGE, "CorrectLoop: %d LoopConnections pairs (at most %d)", hh[1], pair_cap);
        if ((r = orbg_map_essential_graph_device(c, m, cur, loop, dc, du, dset, set_cap, h, dp, pair_cap, h + 1, dv, h + 2,
                                                 h + 3, L.at<orbg_sim3d>(b, o_sc), L.at<orbg_sim3d>(b, o_sn),
                                                 L.at<orbg_eg_edge>(b, o_ed), edge_cap, h + 4, h + 12)))
            return r;
        HIPCHK(hipMemcpyAsync(hh, h, 128, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (hh[12] & ORBG_LOOP_DEAD) return set_err(ORBG_EINVAL, "CorrectLoop: slot %d (loop) is not a vertex", loop);
        if (hh[12] & ORBG_LOOP_NO_POSE) return set_err(ORBG_EINVAL, "CorrectLoop: a keyframe has no pose");
        if (hh[4] > edge_cap) return set_err(ORBG_ERANGE, "CorrectLoop: %d edges (at most %d)", hh[4], edge_cap);
        edges.resize((size_t)std::max(hh[4], 1));
        if (hh[4]) HIPCHK(hipMemcpy(edges.data(), b + o_ed, (size_t)hh[4] * sizeof(orbg_eg_edge), hipMemcpyDeviceToHost));
        if ((r = orbg_eg_graph_create(c, edges.data(), hh[4], hh[2], hh[3], &g))) return r;
        if ((r = orbg_eg_graph_optimize(c, g, L.at<orbg_sim3d>(b, o_sc), L.at<orbg_sim3d>(b, o_sn), fix_scale, 20,
                                        L.at<orbg_sim3d>(b, o_si), L.at<float>(b, o_t), report)))
            return r;
        if ((r = orbg_map_apply_correction_device(c, m, cur, dv, h + 2, L.at<orbg_sim3d>(b, o_sc),
                                                  L.at<orbg_sim3d>(b, o_si), L.at<float>(b, o_t))))
            return r;
        HIPCHK(hipStreamSynchronize(c->stream));
        return ORBG_OK;
    };
    rc = body();
    if (g) orbg_eg_graph_destroy(g);
    hipStreamSynchronize(c->stream);
    hipFree(b);
    if (rc) return rc;
    if ((rc = orbg_map_add_loop_edge(c, m, loop, cur))) return rc;
    const int32_t out[8] = {hh[0], hh[16], hh[17], hh[18], hh[19], hh[1], hh[2], hh[4]};
    for (int i = 0; i < 8; i++) counts[i] = out[i];
    c->prof.collect();
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// Optimizer::LocalBundleAdjustment on the Map (map_lba_kernels.hip)
// ---------------------------------------------------------------------------
// the marks of one window over up to pcap points
static int map_lba_ws(orbg_ctx *c, orbg_map *m, int pcap)
{
    if (m->d_lw && pcap <= m->LW.pcap) return ORBG_OK;
    if (m->d_lw) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(m->d_lw));
        m->d_lw = nullptr;
        m->LW = MapLbaWs{};
    }
    const size_t K = (size_t)m->D.K, n = (size_t)std::max(pcap, 1);
    Layout L;
    const size_t o_h = L.take(16 * 4), o_r = L.take(K * 4), o_f = L.take(K * 4), o_p = L.take(K * 4);
    const size_t o_s = L.take(K * 4), o_x = L.take(K * 4), o_c = L.take((K + 1) * 4);
    const size_t o_e = L.take((n + 1) * 4), o_i = L.take(n * 4);
    if (hipMalloc(&m->d_lw, L.total()) != hipSuccess) {
        m->d_lw = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the local BA marks", L.total());
    }
    HIPCHK(hipMemsetAsync(m->d_lw, 0, L.total(), c->stream));
    uint8_t *b = (uint8_t *)m->d_lw;
    MapLbaWs &W = m->LW;
    W.pcap = (int32_t)n;
    W.hdr = L.at<int32_t>(b, o_h);
    W.lrank = L.at<int32_t>(b, o_r);
    W.ffirst = L.at<int32_t>(b, o_f);
    W.pidx = L.at<int32_t>(b, o_p);
    W.lslot = L.at<int32_t>(b, o_s);
    W.fixed = L.at<int32_t>(b, o_x);
    W.cnt = L.at<int32_t>(b, o_c);
    W.eoff = L.at<int32_t>(b, o_e);
    W.ids = L.at<int32_t>(b, o_i);
    return ORBG_OK;
}

static int map_lba_caps_ok(int pose_cap, int point_cap, int edge_cap)
{
    if (pose_cap < 0 || point_cap < 0 || edge_cap < 0) return set_err(ORBG_EINVAL, "negative cap");
    if (point_cap > ORBG_LBA_MAX_POINTS)
        return set_err(ORBG_ENOTSUP, "point_cap %d (> %d: a window position is 19 bits of a sort key)",
                       point_cap, ORBG_LBA_MAX_POINTS);
    return ORBG_OK;
}

static int map_lba_status(int bits, int slot, const int32_t *cnt, int pose_cap, int point_cap, int edge_cap)
{
    if (bits & ORBG_LBA_DEAD) return set_err(ORBG_EINVAL, "LocalBundleAdjustment: slot %d is not a live keyframe", slot);
    if (bits & ORBG_LBA_NO_POSE) return set_err(ORBG_EINVAL, "LocalBundleAdjustment: a window keyframe has no pose");
    if (bits & ORBG_LBA_RANGE)
        return set_err(ORBG_ERANGE, "LocalBundleAdjustment: %d poses, %d points, %d edges (caps %d, %d, %d)",
                       cnt[1], cnt[2], cnt[3], pose_cap, point_cap, edge_cap);
    if (bits & ORBG_LBA_FEATURE)
        return set_err(ORBG_EINVAL, "LocalBundleAdjustment: an observation's feature index is past the attached count");
    return ORBG_OK;
}

extern "C" int orbg_map_lba_window_device(orbg_ctx *c, orbg_map *m, int slot, int32_t *d_kf_slots,
                                          orbg_pose *d_poses, int pose_cap, int32_t *d_point_ids,
                                          double *d_points, int point_cap, orbg_edge *d_edges,
                                          int32_t *d_edge_feat, int edge_cap, int32_t *d_counts,
                                          int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot)) || (rc = map_lba_caps_ok(pose_cap, point_cap, edge_cap))) return rc;
    if ((pose_cap && (!d_kf_slots || !d_poses)) || (point_cap && (!d_point_ids || !d_points)) ||
        (edge_cap && (!d_edges || !d_edge_feat)) || !d_counts || !d_status)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_attached(m))) return rc;
    if ((rc = map_lba_ws(c, m, point_cap))) return rc;
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    MapLbaWindow O{};
    O.kf_slots = d_kf_slots;
    O.poses = d_poses;
    O.point_ids = d_point_ids;
    O.points = d_points;
    O.edges = d_edges;
    O.edge_feat = d_edge_feat;
    O.pose_cap = pose_cap;
    O.point_cap = point_cap;
    O.edge_cap = edge_cap;
    O.counts = d_counts;
    MapLbaConst C{};
    for (int i = 0; i < 16; i++) C.inv_sigma2[i] = c->inv_sigma2[i];
    const float hm = std::sqrt(5.991), hs = std::sqrt(7.815);  // float in the reference (Optimizer.cc:758-759)
    C.huber_mono = hm;
    C.huber_stereo = hs;
    if ((rc = launch_map_lba_window(c->stream, m->D, m->att, m->LW, slot, O, C, d_status, &c->prof)))
        return set_err(rc, "k_lba window launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_lba_window(orbg_ctx *c, orbg_map *m, int slot, int32_t *kf_slots,
                                   orbg_pose *poses, int pose_cap, int32_t *point_ids, double *points,
                                   int point_cap, orbg_edge *edges, int32_t *edge_feat, int edge_cap,
                                   int32_t *counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot)) || (rc = map_lba_caps_ok(pose_cap, point_cap, edge_cap))) return rc;
    if ((pose_cap && (!kf_slots || !poses)) || (point_cap && (!point_ids || !points)) ||
        (edge_cap && (!edges || !edge_feat)) || !counts)
        return set_err(ORBG_EINVAL, "NULL array");
    const size_t np = (size_t)pose_cap, nq = (size_t)point_cap, ne = (size_t)edge_cap;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_e = L.take(ne * sizeof(orbg_edge)), o_f = L.take(ne * 4);
    const size_t o_h = L.take(32);  // counts [4], status [4]
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    int32_t *h = L.at<int32_t>(b, o_h);
    HIPCHK(hipMemsetAsync(h, 0, 32, c->stream));
    if ((rc = orbg_map_lba_window_device(c, m, slot, L.at<int32_t>(b, o_k), L.at<orbg_pose>(b, o_p),
                                         pose_cap, L.at<int32_t>(b, o_i), L.at<double>(b, o_x),
                                         point_cap, L.at<orbg_edge>(b, o_e), L.at<int32_t>(b, o_f),
                                         edge_cap, h, h + 4)))
        return rc;
    int32_t out[8];
    HIPCHK(hipMemcpyAsync(out, h, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    for (int i = 0; i < 4; i++) counts[i] = out[i];
    if ((rc = map_lba_status(out[4], slot, out, pose_cap, point_cap, edge_cap))) return rc;
    if (out[1]) {
        HIPCHK(hipMemcpy(kf_slots, b + o_k, (size_t)out[1] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(poses, b + o_p, (size_t)out[1] * sizeof(orbg_pose), hipMemcpyDeviceToHost));
    }
    if (out[2]) {
        HIPCHK(hipMemcpy(point_ids, b + o_i, (size_t)out[2] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(points, b + o_x, (size_t)out[2] * 24, hipMemcpyDeviceToHost));
    }
    if (out[3]) {
        HIPCHK(hipMemcpy(edges, b + o_e, (size_t)out[3] * sizeof(orbg_edge), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(edge_feat, b + o_f, (size_t)out[3] * 4, hipMemcpyDeviceToHost));
    }
    return ORBG_OK;
}

extern "C" int orbg_map_lba_apply_device(orbg_ctx *c, orbg_map *m, const int32_t *d_kf_slots,
                                         int pose_cap, const int32_t *d_point_ids, int point_cap,
                                         const orbg_edge *d_edges, const int32_t *d_edge_feat,
                                         int edge_cap, const int32_t *d_counts,
                                         const orbg_pose *d_poses, const double *d_points,
                                         const uint8_t *d_erase, orbg_frustum_camera *d_cams_out,
                                         int32_t *d_out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_lba_caps_ok(pose_cap, point_cap, edge_cap))) return rc;
    if ((pose_cap && (!d_kf_slots || !d_poses)) || (point_cap && (!d_point_ids || !d_points)) ||
        (edge_cap && (!d_edges || !d_edge_feat || !d_erase)) || !d_counts || !d_out)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_lba_ws(c, m, point_cap))) return rc;
    if ((rc = orbg_map_rebuild(c, m))) return rc;  // the erasures read Observations() from the index
    MapLbaWindow O{};
    O.kf_slots = const_cast<int32_t *>(d_kf_slots);
    O.poses = const_cast<orbg_pose *>(d_poses);
    O.point_ids = const_cast<int32_t *>(d_point_ids);
    O.points = const_cast<double *>(d_points);
    O.edges = const_cast<orbg_edge *>(d_edges);
    O.edge_feat = const_cast<int32_t *>(d_edge_feat);
    O.pose_cap = pose_cap;
    O.point_cap = point_cap;
    O.edge_cap = edge_cap;
    O.counts = const_cast<int32_t *>(d_counts);
    if ((rc = launch_map_lba_apply(c->stream, m->D, m->LW, O, d_erase, d_cams_out, d_out, &c->prof)))
        return set_err(rc, "k_lba apply launch failed");
    m->dirty = m->touched = true;  // an erased observation is still in the index
    if (point_cap == 0) return ORBG_OK;
    return orbg_map_update_normal_and_depth_batch_device(c, m, m->LW.ids, point_cap);
}

extern "C" int orbg_map_lba_apply(orbg_ctx *c, orbg_map *m, const int32_t *kf_slots, int nlocal,
                                  int npose, const int32_t *point_ids, int npoint,
                                  const orbg_edge *edges, const int32_t *edge_feat, int nedge,
                                  const orbg_pose *poses, const double *points, const uint8_t *erase,
                                  orbg_frustum_camera *d_cams_out, int32_t *out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (nlocal < 0 || npose < nlocal || npose > m->D.K)
        return set_err(ORBG_EINVAL, "nlocal %d / npose %d outside 0 <= nlocal <= npose <= %d", nlocal, npose, m->D.K);
    if ((rc = map_lba_caps_ok(npose, npoint, nedge))) return rc;
    if ((npose && (!kf_slots || !poses)) || (npoint && (!point_ids || !points)) ||
        (nedge && (!edges || !edge_feat || !erase)))
        return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < npose; i++)
        if ((rc = map_slot_ok(m, kf_slots[i]))) return rc;
    for (int i = 0; i < npoint; i++)
        if (point_ids[i] < 0 || point_ids[i] >= m->D.P)
            return set_err(ORBG_EINVAL, "point id %d outside [0, %d)", point_ids[i], m->D.P);
    for (int e = 0; e < nedge; e++)
        if (edges[e].point < 0 || edges[e].point >= npoint || edges[e].pose < 0 ||
            edges[e].pose >= npose || edge_feat[e] < 0 || edge_feat[e] >= m->D.cap)
            return set_err(ORBG_EINVAL, "edge %d: point %d, pose %d or feature %d out of range", e,
                           edges[e].point, edges[e].pose, edge_feat[e]);
    const size_t np = (size_t)npose, nq = (size_t)npoint, ne = (size_t)nedge;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_e = L.take(ne * sizeof(orbg_edge)), o_f = L.take(ne * 4);
    const size_t o_r = L.take(ne), o_h = L.take(32);  // counts [4], out [2]
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[8] = {nlocal, npose, npoint, nedge, 0, 0, 0, 0};
    hipStream_t st = c->stream;
    if (np) {
        HIPCHK(hipMemcpyAsync(b + o_k, kf_slots, np * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_p, poses, np * sizeof(orbg_pose), hipMemcpyHostToDevice, st));
    }
    if (nq) {
        HIPCHK(hipMemcpyAsync(b + o_i, point_ids, nq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_x, points, nq * 24, hipMemcpyHostToDevice, st));
    }
    if (ne) {
        HIPCHK(hipMemcpyAsync(b + o_e, edges, ne * sizeof(orbg_edge), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_f, edge_feat, ne * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_r, erase, ne, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(b + o_h, hdr, 32, hipMemcpyHostToDevice, st));
    int32_t *h = L.at<int32_t>(b, o_h);
    if ((rc = orbg_map_lba_apply_device(c, m, L.at<int32_t>(b, o_k), npose, L.at<int32_t>(b, o_i), npoint,
                                        L.at<orbg_edge>(b, o_e), L.at<int32_t>(b, o_f), nedge, h,
                                        L.at<orbg_pose>(b, o_p), L.at<double>(b, o_x), b + o_r,
                                        d_cams_out, h + 4)))
        return rc;
    int32_t o2[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(o2, h + 4, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    if (out) {
        out[0] = o2[0];
        out[1] = o2[1];
    }
    return ORBG_OK;
}

// orbg_map_local_ba's window arrays, grown to the caps asked for
static int map_lba_chain_ws(orbg_ctx *c, orbg_map *m, int pose_cap, int point_cap, int edge_cap)
{
    MapLbaWindow &B = m->LB;
    if (m->d_lb && pose_cap <= B.pose_cap && point_cap <= B.point_cap && edge_cap <= B.edge_cap)
        return ORBG_OK;
    pose_cap = std::max(pose_cap, B.pose_cap);
    point_cap = std::max(point_cap, B.point_cap);
    edge_cap = std::max(edge_cap, B.edge_cap);
    if (m->d_lb) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(m->d_lb));
        m->d_lb = nullptr;
        B = MapLbaWindow{};
    }
    const size_t np = (size_t)pose_cap, nq = (size_t)point_cap, ne = (size_t)edge_cap;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_e = L.take(ne * sizeof(orbg_edge)), o_f = L.take(ne * 4);
    const size_t o_r = L.take(ne), o_h = L.take(64);  // counts [4], status [4], out [2]
    if (hipMalloc(&m->d_lb, L.total()) != hipSuccess) {
        m->d_lb = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the local BA window", L.total());
    }
    uint8_t *b = (uint8_t *)m->d_lb;
    B.kf_slots = L.at<int32_t>(b, o_k);
    B.poses = L.at<orbg_pose>(b, o_p);
    B.point_ids = L.at<int32_t>(b, o_i);
    B.points = L.at<double>(b, o_x);
    B.edges = L.at<orbg_edge>(b, o_e);
    B.edge_feat = L.at<int32_t>(b, o_f);
    B.counts = L.at<int32_t>(b, o_h);
    B.pose_cap = pose_cap;
    B.point_cap = point_cap;
    B.edge_cap = edge_cap;
    m->d_lb_erase = b + o_r;
    return ORBG_OK;
}

extern "C" int orbg_map_local_ba(orbg_ctx *c, orbg_map *m, int slot, const orbg_lm_control *control,
                                 orbg_frustum_camera *d_cams_out, orbg_map_lba_report *report)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if ((rc = map_slot_ok(m, slot))) return rc;
    if (!report) return set_err(ORBG_EINVAL, "report is NULL");
    if ((rc = map_attached(m))) return rc;
    *report = orbg_map_lba_report{};
    const MapDev &D = m->D;
    const int64_t rows = (int64_t)D.K * D.cap;
    if (!m->d_lb &&
        (rc = map_lba_chain_ws(c, m, std::min(D.K, 128), (int)std::min<int64_t>({(int64_t)D.P, rows, 1 << 16}),
                               (int)std::min<int64_t>(rows, 1 << 18))))
        return rc;
    hipStream_t st = c->stream;
    int32_t h[8] = {0};
    for (int pass = 0;; pass++) {
        const MapLbaWindow &B = m->LB;
        if ((rc = orbg_map_lba_window_device(c, m, slot, B.kf_slots, B.poses, B.pose_cap, B.point_ids,
                                             B.points, B.point_cap, B.edges, B.edge_feat, B.edge_cap,
                                             B.counts, B.counts + 4)))
            return rc;
        HIPCHK(hipMemcpyAsync(h, B.counts, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!(h[4] & ORBG_LBA_RANGE) || (h[4] & (ORBG_LBA_DEAD | ORBG_LBA_NO_POSE)) || pass) break;
        if (h[2] > ORBG_LBA_MAX_POINTS) break;
        if ((rc = map_lba_chain_ws(c, m, h[1] + h[1] / 4, std::min(h[2] + h[2] / 4, ORBG_LBA_MAX_POINTS),
                                   h[3] + h[3] / 4)))
            return rc;
    }
    const MapLbaWindow &B = m->LB;
    if ((rc = map_lba_status(h[4], slot, h, B.pose_cap, B.point_cap, B.edge_cap))) return rc;
    report->nlocal = h[0];
    report->nfixed = h[1] - h[0];
    report->npoints = h[2];
    report->nedges = h[3];
    if (control && control->force_stop && *control->force_stop != 0) {  // Optimizer.cc:853-855
        report->stopped = 1;
        c->prof.collect();
        return ORBG_OK;
    }
    const int npose = h[1], npoint = h[2], nedge = h[3];
    m->lb_erase.assign((size_t)std::max(nedge, 1), 0);
    if (nedge) {
        m->lb_edges.resize((size_t)nedge);
        m->lb_fixed.resize((size_t)npose);
        m->lb_fixed8.resize((size_t)npose);
        HIPCHK(hipMemcpyAsync(m->lb_edges.data(), B.edges, (size_t)nedge * sizeof(orbg_edge), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(m->lb_fixed.data(), m->LW.fixed, (size_t)npose * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < npose; i++) m->lb_fixed8[i] = m->lb_fixed[i] ? 1 : 0;
        orbg_lm_control K{};
        if (control) K = *control;
        K.d_last_chi2 = nullptr;
        if ((rc = lba_optimize_device(c, B.poses, npose, B.points, npoint, m->lb_edges.data(), nedge,
                                      m->lb_fixed8.data(), &K, nullptr, nullptr, m->lb_erase.data(),
                                      &report->lba)))
            return rc;
    }
    uint8_t *d_erase = m->d_lb_erase;  // the two counts go behind the window's status
    if (nedge) HIPCHK(hipMemcpyAsync(d_erase, m->lb_erase.data(), (size_t)nedge, hipMemcpyHostToDevice, st));
    if ((rc = orbg_map_lba_apply_device(c, m, B.kf_slots, B.pose_cap, B.point_ids, B.point_cap, B.edges,
                                        B.edge_feat, B.edge_cap, B.counts, B.poses, B.points, d_erase,
                                        d_cams_out, B.counts + 8)))
        return rc;
    int32_t o2[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(o2, B.counts + 8, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    report->nerased = o2[0];
    report->npoints_bad = o2[1];
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// Optimizer::GlobalBundleAdjustemnt and LoopClosing::RunGlobalBundleAdjustment on the Map
// (map_gba_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_map_set_gba_state(orbg_ctx *c, orbg_map *m, int first_slot, int nslots,
                                      const float *TcwGBA, const float *TcwBefGBA,
                                      const int32_t *kf_ba_global, int first_point, int npoints,
                                      const float *PosGBA, const int32_t *mp_ba_global)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (nslots < 0 || first_slot < 0 || (int64_t)first_slot + nslots > m->D.K)
        return set_err(ORBG_EINVAL, "slots %d .. %lld outside [0, %d)", first_slot,
                       (long long)first_slot + nslots, m->D.K);
    if ((rc = map_range_ok(m, first_point, npoints))) return rc;
    const MapDev &D = m->D;
    hipStream_t st = c->stream;
    const size_t s0 = (size_t)first_slot, ns = (size_t)nslots, p0 = (size_t)first_point, np = (size_t)npoints;
    if (ns && TcwGBA) HIPCHK(hipMemcpyAsync(D.kf_TcwGBA + s0 * 12, TcwGBA, ns * 48, hipMemcpyHostToDevice, st));
    if (ns && TcwBefGBA) HIPCHK(hipMemcpyAsync(D.kf_TcwBef + s0 * 12, TcwBefGBA, ns * 48, hipMemcpyHostToDevice, st));
    if (ns && kf_ba_global) HIPCHK(hipMemcpyAsync(D.kf_gba + s0, kf_ba_global, ns * 4, hipMemcpyHostToDevice, st));
    if (np && PosGBA) HIPCHK(hipMemcpyAsync(D.mp_posGBA + p0 * 3, PosGBA, np * 12, hipMemcpyHostToDevice, st));
    if (np && mp_ba_global) HIPCHK(hipMemcpyAsync(D.mp_gba + p0, mp_ba_global, np * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_get_gba_state(orbg_ctx *c, orbg_map *m, int first_slot, int nslots,
                                      float *TcwGBA, float *TcwBefGBA, int32_t *kf_ba_global,
                                      int first_point, int npoints, float *PosGBA,
                                      int32_t *mp_ba_global)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (nslots < 0 || first_slot < 0 || (int64_t)first_slot + nslots > m->D.K)
        return set_err(ORBG_EINVAL, "slots %d .. %lld outside [0, %d)", first_slot,
                       (long long)first_slot + nslots, m->D.K);
    if ((rc = map_range_ok(m, first_point, npoints))) return rc;
    const MapDev &D = m->D;
    hipStream_t st = c->stream;
    const size_t s0 = (size_t)first_slot, ns = (size_t)nslots, p0 = (size_t)first_point, np = (size_t)npoints;
    if (ns && TcwGBA) HIPCHK(hipMemcpyAsync(TcwGBA, D.kf_TcwGBA + s0 * 12, ns * 48, hipMemcpyDeviceToHost, st));
    if (ns && TcwBefGBA) HIPCHK(hipMemcpyAsync(TcwBefGBA, D.kf_TcwBef + s0 * 12, ns * 48, hipMemcpyDeviceToHost, st));
    if (ns && kf_ba_global) HIPCHK(hipMemcpyAsync(kf_ba_global, D.kf_gba + s0, ns * 4, hipMemcpyDeviceToHost, st));
    if (np && PosGBA) HIPCHK(hipMemcpyAsync(PosGBA, D.mp_posGBA + p0 * 3, np * 12, hipMemcpyDeviceToHost, st));
    if (np && mp_ba_global) HIPCHK(hipMemcpyAsync(mp_ba_global, D.mp_gba + p0, np * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ORBG_OK;
}

extern "C" int orbg_map_get_keyframe_flags(orbg_ctx *c, orbg_map *m, int first, int n, int32_t *flags)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (n < 0 || first < 0 || (int64_t)first + n > m->D.K)
        return set_err(ORBG_EINVAL, "slots %d .. %lld outside [0, %d)", first, (long long)first + n, m->D.K);
    if (n == 0) return ORBG_OK;
    if (!flags) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(flags, m->D.kf_flags + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

// the marks of a window, a store or an update: sized by K and P, allocated once
static int map_gba_ws(orbg_ctx *c, orbg_map *m)
{
    if (m->d_gw) return ORBG_OK;
    const size_t K = (size_t)m->D.K, P = (size_t)m->D.P;
    Layout L;
    const size_t o_h = L.take(16 * 4), o_x = L.take(K * 4), o_f = L.take(K * 4), o_n = L.take(P * 4);
    const size_t o_p = L.take(P * 4), o_e = L.take(P * 4), o_i = L.take(P * 4), o_o = L.take(K * 4);
    const size_t o_v = L.take(K * 4), o_g = L.take(K * 48);
    if (hipMalloc(&m->d_gw, L.total()) != hipSuccess) {
        m->d_gw = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the global BA marks", L.total());
    }
    HIPCHK(hipMemsetAsync(m->d_gw, 0, L.total(), c->stream));
    uint8_t *b = (uint8_t *)m->d_gw;
    MapGbaWs &W = m->GW;
    W.hdr = L.at<int32_t>(b, o_h);
    W.pidx = L.at<int32_t>(b, o_x);
    W.fixed = L.at<int32_t>(b, o_f);
    W.ne = L.at<int32_t>(b, o_n);
    W.pi = L.at<int32_t>(b, o_p);
    W.eoff = L.at<int32_t>(b, o_e);
    W.ids = L.at<int32_t>(b, o_i);
    W.org = L.at<int32_t>(b, o_o);
    W.vis = L.at<int32_t>(b, o_v);
    W.gT = L.at<float>(b, o_g);
    return ORBG_OK;
}

static int map_gba_window_status(int bits, const int32_t *cnt, int pose_cap, int point_cap, int edge_cap)
{
    if (bits & ORBG_LBA_NO_POSE) return set_err(ORBG_EINVAL, "GlobalBundleAdjustment: a keyframe that is not bad has no pose");
    if (bits & ORBG_LBA_RANGE)
        return set_err(ORBG_ERANGE, "GlobalBundleAdjustment: %d poses, %d points, %d edges (caps %d, %d, %d)",
                       cnt[0], cnt[1], cnt[2], pose_cap, point_cap, edge_cap);
    if (bits & ORBG_LBA_FEATURE)
        return set_err(ORBG_EINVAL, "GlobalBundleAdjustment: an observation's feature index is past the attached count");
    return ORBG_OK;
}

extern "C" int orbg_map_gba_window_device(orbg_ctx *c, orbg_map *m, int robust, int32_t *d_kf_slots,
                                          orbg_pose *d_poses, int pose_cap, int32_t *d_point_ids,
                                          double *d_points, int point_cap, orbg_edge *d_edges,
                                          int32_t *d_edge_feat, int edge_cap, int32_t *d_counts,
                                          int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (pose_cap < 0 || point_cap < 0 || edge_cap < 0) return set_err(ORBG_EINVAL, "negative cap");
    if ((pose_cap && (!d_kf_slots || !d_poses)) || (point_cap && (!d_point_ids || !d_points)) ||
        (edge_cap && (!d_edges || !d_edge_feat)) || !d_counts || !d_status)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_attached(m))) return rc;
    if ((rc = map_gba_ws(c, m))) return rc;
    if ((rc = orbg_map_rebuild(c, m))) return rc;
    MapLbaWindow O{};
    O.kf_slots = d_kf_slots;
    O.poses = d_poses;
    O.point_ids = d_point_ids;
    O.points = d_points;
    O.edges = d_edges;
    O.edge_feat = d_edge_feat;
    O.pose_cap = pose_cap;
    O.point_cap = point_cap;
    O.edge_cap = edge_cap;
    O.counts = d_counts;
    MapLbaConst C{};
    for (int i = 0; i < 16; i++) C.inv_sigma2[i] = c->inv_sigma2[i];
    const float hm = std::sqrt(5.99), hs = std::sqrt(7.815);  // float in the reference (Optimizer.cc:157-158)
    C.huber_mono = hm;
    C.huber_stereo = hs;
    if ((rc = launch_map_gba_window(c->stream, m->D, m->att, m->GW, robust ? 1 : 0, O, C, d_status, &c->prof)))
        return set_err(rc, "k_gba window launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_gba_window(orbg_ctx *c, orbg_map *m, int robust, int32_t *kf_slots,
                                   orbg_pose *poses, int pose_cap, int32_t *point_ids, double *points,
                                   int point_cap, orbg_edge *edges, int32_t *edge_feat, int edge_cap,
                                   int32_t *counts)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (pose_cap < 0 || point_cap < 0 || edge_cap < 0) return set_err(ORBG_EINVAL, "negative cap");
    if ((pose_cap && (!kf_slots || !poses)) || (point_cap && (!point_ids || !points)) ||
        (edge_cap && (!edges || !edge_feat)) || !counts)
        return set_err(ORBG_EINVAL, "NULL array");
    const size_t np = (size_t)pose_cap, nq = (size_t)point_cap, ne = (size_t)edge_cap;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_e = L.take(ne * sizeof(orbg_edge)), o_f = L.take(ne * 4);
    const size_t o_h = L.take(32);  // counts [4], status [4]
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    int32_t *h = L.at<int32_t>(b, o_h);
    HIPCHK(hipMemsetAsync(h, 0, 32, c->stream));
    if ((rc = orbg_map_gba_window_device(c, m, robust, L.at<int32_t>(b, o_k), L.at<orbg_pose>(b, o_p),
                                         pose_cap, L.at<int32_t>(b, o_i), L.at<double>(b, o_x),
                                         point_cap, L.at<orbg_edge>(b, o_e), L.at<int32_t>(b, o_f),
                                         edge_cap, h, h + 4)))
        return rc;
    int32_t out[8];
    HIPCHK(hipMemcpyAsync(out, h, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    for (int i = 0; i < 4; i++) counts[i] = out[i];
    if ((rc = map_gba_window_status(out[4], out, pose_cap, point_cap, edge_cap))) return rc;
    if (out[0]) {
        HIPCHK(hipMemcpy(kf_slots, b + o_k, (size_t)out[0] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(poses, b + o_p, (size_t)out[0] * sizeof(orbg_pose), hipMemcpyDeviceToHost));
    }
    if (out[1]) {
        HIPCHK(hipMemcpy(point_ids, b + o_i, (size_t)out[1] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(points, b + o_x, (size_t)out[1] * 24, hipMemcpyDeviceToHost));
    }
    if (out[2]) {
        HIPCHK(hipMemcpy(edges, b + o_e, (size_t)out[2] * sizeof(orbg_edge), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(edge_feat, b + o_f, (size_t)out[2] * 4, hipMemcpyDeviceToHost));
    }
    return ORBG_OK;
}

extern "C" int orbg_map_gba_store_device(orbg_ctx *c, orbg_map *m, const int32_t *d_kf_slots,
                                         int pose_cap, const int32_t *d_point_ids, int point_cap,
                                         const int32_t *d_counts, const orbg_pose *d_poses,
                                         const double *d_points, int loop_kf,
                                         orbg_frustum_camera *d_cams_out, int32_t *d_out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (pose_cap < 0 || point_cap < 0) return set_err(ORBG_EINVAL, "negative cap");
    if ((pose_cap && (!d_kf_slots || !d_poses)) || (point_cap && (!d_point_ids || !d_points)) ||
        !d_counts || !d_out)
        return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_gba_ws(c, m))) return rc;
    HIPCHK(hipMemsetAsync(d_out, 0, 8, c->stream));
    if ((rc = launch_map_gba_store(c->stream, m->D, m->GW, d_counts, d_kf_slots, pose_cap, d_point_ids,
                                   point_cap, d_poses, d_points, loop_kf, d_cams_out, d_out, &c->prof)))
        return set_err(rc, "k_gba_store launch failed");
    m->touched = true;
    const int n = std::min(point_cap, m->D.P);
    if (loop_kf != 0 || n == 0) return ORBG_OK;
    return orbg_map_update_normal_and_depth_batch_device(c, m, m->GW.ids, n);
}

extern "C" int orbg_map_gba_store(orbg_ctx *c, orbg_map *m, const int32_t *kf_slots, int npose,
                                  const int32_t *point_ids, int npoint, const orbg_pose *poses,
                                  const double *points, int loop_kf, orbg_frustum_camera *d_cams_out,
                                  int32_t *out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (npose < 0 || npose > m->D.K || npoint < 0 || npoint > m->D.P)
        return set_err(ORBG_EINVAL, "npose %d / npoint %d outside [0, %d] / [0, %d]", npose, npoint, m->D.K, m->D.P);
    if ((npose && (!kf_slots || !poses)) || (npoint && (!point_ids || !points)))
        return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < npose; i++)
        if ((rc = map_slot_ok(m, kf_slots[i]))) return rc;
    for (int i = 0; i < npoint; i++)
        if (point_ids[i] < 0 || point_ids[i] >= m->D.P)
            return set_err(ORBG_EINVAL, "point id %d outside [0, %d)", point_ids[i], m->D.P);
    const size_t np = (size_t)npose, nq = (size_t)npoint;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_h = L.take(32);  // counts [4], out [2]
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t hdr[8] = {npose, npoint, 0, 0, 0, 0, 0, 0};
    hipStream_t st = c->stream;
    if (np) {
        HIPCHK(hipMemcpyAsync(b + o_k, kf_slots, np * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_p, poses, np * sizeof(orbg_pose), hipMemcpyHostToDevice, st));
    }
    if (nq) {
        HIPCHK(hipMemcpyAsync(b + o_i, point_ids, nq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b + o_x, points, nq * 24, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(b + o_h, hdr, 32, hipMemcpyHostToDevice, st));
    int32_t *h = L.at<int32_t>(b, o_h);
    if ((rc = orbg_map_gba_store_device(c, m, L.at<int32_t>(b, o_k), npose, L.at<int32_t>(b, o_i), npoint,
                                        h, L.at<orbg_pose>(b, o_p), L.at<double>(b, o_x), loop_kf,
                                        d_cams_out, h + 4)))
        return rc;
    int32_t o2[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(o2, h + 4, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    if (out) {
        out[0] = o2[0];
        out[1] = o2[1];
    }
    return ORBG_OK;
}

static int map_gba_update_status(int bits)
{
    if (bits & ORBG_GBA_ORIGIN)
        return set_err(ORBG_EINVAL, "RunGlobalBundleAdjustment: an origin is dead, has no pose or was not in the global BA");
    if (bits & ORBG_GBA_CYCLE) return set_err(ORBG_EINVAL, "RunGlobalBundleAdjustment: the parents form a cycle");
    if (bits & ORBG_GBA_NO_POSE) return set_err(ORBG_EINVAL, "RunGlobalBundleAdjustment: a visited keyframe has no pose");
    return ORBG_OK;
}

extern "C" int orbg_map_gba_update_device(orbg_ctx *c, orbg_map *m, const int32_t *d_origins,
                                          int norigins, int loop_kf, orbg_frustum_camera *d_cams_out,
                                          int32_t *d_out, int32_t *d_status)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (norigins < 0) return set_err(ORBG_EINVAL, "negative size");
    if (loop_kf == 0) return set_err(ORBG_EINVAL, "loop_kf is 0");
    if ((norigins && !d_origins) || !d_out || !d_status) return set_err(ORBG_EINVAL, "NULL device array");
    if ((rc = map_gba_ws(c, m))) return rc;
    HIPCHK(hipMemsetAsync(d_out, 0, 24, c->stream));
    HIPCHK(hipMemsetAsync(d_status, 0, 16, c->stream));
    if ((rc = launch_map_gba_update(c->stream, m->D, m->GW, d_origins, norigins, loop_kf, d_cams_out,
                                    d_out, d_status, &c->prof)))
        return set_err(rc, "k_gba update launch failed");
    m->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_map_gba_update(orbg_ctx *c, orbg_map *m, const int32_t *origins, int norigins,
                                   int loop_kf, orbg_frustum_camera *d_cams_out, int32_t *out)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (norigins < 0) return set_err(ORBG_EINVAL, "negative size");
    if (loop_kf == 0) return set_err(ORBG_EINVAL, "loop_kf is 0");
    if (norigins && !origins) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < norigins; i++)
        if ((rc = map_slot_ok(m, origins[i]))) return rc;
    Layout L;
    const size_t o_o = L.take((size_t)norigins * 4), o_h = L.take(48);  // out [6], pad [2], status [4]
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    hipStream_t st = c->stream;
    if (norigins) HIPCHK(hipMemcpyAsync(b + o_o, origins, (size_t)norigins * 4, hipMemcpyHostToDevice, st));
    int32_t *h = L.at<int32_t>(b, o_h);
    if ((rc = orbg_map_gba_update_device(c, m, L.at<int32_t>(b, o_o), norigins, loop_kf, d_cams_out, h, h + 8)))
        return rc;
    int32_t o[12] = {0};
    HIPCHK(hipMemcpyAsync(o, h, 48, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    if ((rc = map_gba_update_status(o[8]))) return rc;
    if (out)
        for (int i = 0; i < 6; i++) out[i] = o[i];
    return ORBG_OK;
}

// orbg_map_global_ba's window arrays: poses and points by K and P, the edges grown to edge_cap
static int map_gba_chain_ws(orbg_ctx *c, orbg_map *m, int edge_cap)
{
    MapLbaWindow &B = m->GB;
    if (m->d_gb && edge_cap <= B.edge_cap) return ORBG_OK;
    edge_cap = std::max(edge_cap, B.edge_cap);
    if (m->d_gb) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(m->d_gb));
        m->d_gb = nullptr;
        B = MapLbaWindow{};
    }
    const size_t np = (size_t)m->D.K, nq = (size_t)m->D.P, ne = (size_t)edge_cap;
    Layout L;
    const size_t o_k = L.take(np * 4), o_p = L.take(np * sizeof(orbg_pose)), o_i = L.take(nq * 4);
    const size_t o_x = L.take(nq * 24), o_e = L.take(ne * sizeof(orbg_edge)), o_f = L.take(ne * 4);
    const size_t o_h = L.take(64);  // counts [4], status [4], the store's out [2]
    if (hipMalloc(&m->d_gb, L.total()) != hipSuccess) {
        m->d_gb = nullptr;
        return set_err(ORBG_ENOMEM, "Map: hipMalloc(%zu bytes) for the global BA window", L.total());
    }
    uint8_t *b = (uint8_t *)m->d_gb;
    B.kf_slots = L.at<int32_t>(b, o_k);
    B.poses = L.at<orbg_pose>(b, o_p);
    B.point_ids = L.at<int32_t>(b, o_i);
    B.points = L.at<double>(b, o_x);
    B.edges = L.at<orbg_edge>(b, o_e);
    B.edge_feat = L.at<int32_t>(b, o_f);
    B.counts = L.at<int32_t>(b, o_h);
    B.pose_cap = m->D.K;
    B.point_cap = m->D.P;
    B.edge_cap = edge_cap;
    return ORBG_OK;
}

extern "C" int orbg_map_global_ba(orbg_ctx *c, orbg_map *m, int iterations, int robust, int loop_kf,
                                  const orbg_lm_control *control, orbg_frustum_camera *d_cams_out,
                                  orbg_map_gba_report *report)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (!report) return set_err(ORBG_EINVAL, "report is NULL");
    if (iterations < 0) return set_err(ORBG_EINVAL, "negative iterations");
    if ((rc = map_attached(m))) return rc;
    *report = orbg_map_gba_report{};
    const MapDev &D = m->D;
    const int64_t rows = (int64_t)D.K * D.cap;
    if (!m->d_gb && (rc = map_gba_chain_ws(c, m, (int)std::min<int64_t>(rows, 1 << 18)))) return rc;
    hipStream_t st = c->stream;
    int32_t h[8] = {0};
    for (int pass = 0;; pass++) {
        const MapLbaWindow &B = m->GB;
        if ((rc = orbg_map_gba_window_device(c, m, robust, B.kf_slots, B.poses, B.pose_cap, B.point_ids,
                                             B.points, B.point_cap, B.edges, B.edge_feat, B.edge_cap,
                                             B.counts, B.counts + 4)))
            return rc;
        HIPCHK(hipMemcpyAsync(h, B.counts, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!(h[4] & ORBG_LBA_RANGE) || (h[4] & ORBG_LBA_NO_POSE) || pass) break;
        if ((rc = map_gba_chain_ws(c, m, h[2]))) return rc;  // the poses and points always fit
    }
    const MapLbaWindow &B = m->GB;
    if ((rc = map_gba_window_status(h[4], h, B.pose_cap, B.point_cap, B.edge_cap))) return rc;
    report->nposes = h[0];
    report->npoints = h[1];
    report->nedges = h[2];
    report->nleft_out = h[3];
    const int npose = h[0], npoint = h[1], nedge = h[2];
    if (nedge == 0) {  // initializeOptimization of an empty graph fails: nothing optimised or stored
        c->prof.collect();
        return ORBG_OK;
    }
    m->gb_edges.resize((size_t)nedge);
    m->gb_fixed.resize((size_t)npose);
    m->gb_fixed8.resize((size_t)npose);
    HIPCHK(hipMemcpyAsync(m->gb_edges.data(), B.edges, (size_t)nedge * sizeof(orbg_edge), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(m->gb_fixed.data(), m->GW.fixed, (size_t)npose * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < npose; i++) m->gb_fixed8[i] = m->gb_fixed[i] ? 1 : 0;
    if ((rc = gba_optimize_device(c, B.poses, npose, B.points, npoint, m->gb_edges.data(), nedge,
                                  m->gb_fixed8.data(), iterations, control, &report->gba)))
        return rc;
    if ((rc = orbg_map_gba_store_device(c, m, B.kf_slots, B.pose_cap, B.point_ids, B.point_cap, B.counts,
                                        B.poses, B.points, loop_kf, d_cams_out, B.counts + 8)))
        return rc;
    HIPCHK(hipMemcpyAsync(report->store, B.counts + 8, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->prof.collect();
    return ORBG_OK;
}

extern "C" int orbg_map_run_global_ba(orbg_ctx *c, orbg_map *m, const int32_t *origins, int norigins,
                                      int loop_kf, const orbg_lm_control *control,
                                      orbg_frustum_camera *d_cams_out, orbg_map_gba_report *report)
{
    int rc = map_enter(c, m);
    if (rc) return rc;
    if (!report) return set_err(ORBG_EINVAL, "report is NULL");
    if (norigins < 0) return set_err(ORBG_EINVAL, "negative size");
    if (loop_kf == 0) return set_err(ORBG_EINVAL, "loop_kf is 0");
    if (norigins && !origins) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < norigins; i++)
        if ((rc = map_slot_ok(m, origins[i]))) return rc;
    // Optimizer::GlobalBundleAdjustemnt(mpMap, 10, &mbStopGBA, nLoopKF, false); the cameras follow SetPose only
    if ((rc = orbg_map_global_ba(c, m, 10, 0, loop_kf, control, nullptr, report))) return rc;
    if (control && control->force_stop && *control->force_stop != 0) {  // LoopClosing.cc:1040
        report->stopped = 1;
        return ORBG_OK;
    }
    if ((rc = orbg_map_gba_update(c, m, origins, norigins, loop_kf, d_cams_out, report->update))) return rc;
    return ORBG_OK;
}
