// api_place.hip -- orbg_bow_score*, orbg_kfdb_*
#include "orbg_ctx.h"
#include "place_args.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// place recognition: TemplatedVocabulary::score + KeyFrameDatabase (place_kernels.hip)
// ---------------------------------------------------------------------------
struct orbg_kfdb {
    int device = 0;
    PlaceDb D{};
    void *d_mem = nullptr;       // one allocation behind every PlaceDb array
    bool dirty = true;           // the inverted file is stale (add / erase / clear since)
    bool touched = false;        // any device work issued yet
    hipStream_t stream = nullptr;  // the context stream of the last call
};

static int place_l1_only(const orbg_vocab *v)
{
    if (v->scoring != ORBG_L1_NORM)
        return set_err(ORBG_ENOTSUP, "scoring type %d: only L1_NORM (0) is supported", v->scoring);
    return ORBG_OK;
}

extern "C" int orbg_bow_score_batch_device(orbg_ctx *c, const orbg_vocab *v,
                                           const orbg_bow_vectors *a, const orbg_bow_vectors *b,
                                           int cap, const int32_t *d_a_index,
                                           const int32_t *d_b_index, int npairs, double *d_score)
{
    if (!c || !v || !a || !b) return set_err(ORBG_EINVAL, "NULL argument");
    if (v->device != c->device) return set_err(ORBG_EINVAL, "vocabulary lives on another device");
    int rc = place_l1_only(v);
    if (rc) return rc;
    if (npairs < 0 || cap < 1 || cap > ORBG_KFDB_MAX_CAP) return set_err(ORBG_EINVAL, "bad npairs / cap");
    if (npairs == 0) return ORBG_OK;
    if (!a->words || !a->weights || !a->nbow || !b->words || !b->weights || !b->nbow || !d_score)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = launch_place_score(c->stream, *a, *b, cap, d_a_index, d_b_index, npairs, d_score,
                                 &c->prof)))
        return set_err(rc, "k_place_score launch failed");
    return ORBG_OK;
}

extern "C" int orbg_bow_score(orbg_ctx *c, const orbg_vocab *v, const int32_t *words1,
                              const double *weights1, int n1, const int32_t *words2,
                              const double *weights2, int n2, double *score)
{
    if (!c || !v || !score) return set_err(ORBG_EINVAL, "NULL argument");
    int rc = place_l1_only(v);
    if (rc) return rc;
    if (n1 < 0 || n2 < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n1 > ORBG_KFDB_MAX_CAP || n2 > ORBG_KFDB_MAX_CAP)
        return set_err(ORBG_ENOTSUP, "a BowVector with more than %d entries", ORBG_KFDB_MAX_CAP);
    if ((n1 && (!words1 || !weights1)) || (n2 && (!words2 || !weights2)))
        return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipSetDevice(c->device));
    const int cap = std::max(std::max(n1, n2), 1);
    Layout L;
    const size_t o_w = L.take((size_t)2 * cap * 4), o_x = L.take((size_t)2 * cap * 8);
    const size_t o_n = L.take(8), o_i = L.take(8), o_s = L.take(8);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t nb[2] = {n1, n2}, idx[2] = {0, 1};
    if (n1) HIPCHK(hipMemcpyAsync(b + o_w, words1, (size_t)n1 * 4, hipMemcpyHostToDevice, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(b + o_x, weights1, (size_t)n1 * 8, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPCHK(hipMemcpyAsync(b + o_w + (size_t)cap * 4, words2, (size_t)n2 * 4, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPCHK(hipMemcpyAsync(b + o_x + (size_t)cap * 8, weights2, (size_t)n2 * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, nb, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_i, idx, 8, hipMemcpyHostToDevice, c->stream));
    orbg_bow_vectors V{L.at<int32_t>(b, o_w), L.at<double>(b, o_x),
                       L.at<int32_t>(b, o_n)};
    if ((rc = launch_place_score(c->stream, V, V, cap, L.at<int32_t>(b, o_i),
                                 L.at<int32_t>(b, o_i) + 1, 1, L.at<double>(b, o_s), &c->prof)))
        return set_err(rc, "k_place_score launch failed");
    HIPCHK(hipMemcpyAsync(score, b + o_s, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}

extern "C" int orbg_kfdb_create(orbg_ctx *c, const orbg_vocab *v, int max_keyframes, int cap,
                                orbg_kfdb **out)
{
    if (!c || !v || !out) return set_err(ORBG_EINVAL, "NULL argument");
    *out = nullptr;
    if (v->device != c->device) return set_err(ORBG_EINVAL, "vocabulary lives on another device");
    int rc = place_l1_only(v);
    if (rc) return rc;
    if (max_keyframes < 1 || cap < 1) return set_err(ORBG_EINVAL, "max_keyframes / cap < 1");
    if (max_keyframes > ORBG_KFDB_MAX_KEYFRAMES)
        return set_err(ORBG_ENOTSUP, "max_keyframes %d (> %d: a query's per-slot state lives in LDS)",
                       max_keyframes, ORBG_KFDB_MAX_KEYFRAMES);
    if (cap > ORBG_KFDB_MAX_CAP) return set_err(ORBG_ENOTSUP, "cap %d (> %d)", cap, ORBG_KFDB_MAX_CAP);
    HIPCHK(hipSetDevice(c->device));
    const size_t K = (size_t)max_keyframes, kc = K * (size_t)cap, nw = (size_t)v->nwords;
    Layout L;
    const size_t o_wt = L.take(kc * 8), o_wd = L.take(kc * 4), o_nb = L.take(K * 4);
    const size_t o_lv = L.take(K * 4), o_sq = L.take(K * 8), o_rl = L.take(K * 4);
    const size_t o_ct = L.take(8), o_nl = L.take(4), o_rk = L.take(K * 4);
    const size_t o_io = L.take((nw + 1) * 4), o_ic = L.take(nw * 4), o_po = L.take(kc * 2);
    const size_t o_pe = L.take(K * 8), o_pt = L.take((nw / 4096 + 1) * 4);
    auto *db = new orbg_kfdb();
    db->device = c->device;
    if (hipMalloc(&db->d_mem, L.total()) != hipSuccess) {
        delete db;
        return set_err(ORBG_ENOMEM, "KeyFrameDatabase: hipMalloc(%zu bytes)", L.total());
    }
    uint8_t *b = (uint8_t *)db->d_mem;
    PlaceDb &D = db->D;
    D.K = max_keyframes;
    D.cap = cap;
    D.nwords = v->nwords;
    D.weights = L.at<double>(b, o_wt);
    D.words = L.at<int32_t>(b, o_wd);
    D.nbow = L.at<int32_t>(b, o_nb);
    D.live = L.at<int32_t>(b, o_lv);
    D.seq = L.at<int64_t>(b, o_sq);
    D.reloc = L.at<float>(b, o_rl);
    D.counter = L.at<int64_t>(b, o_ct);
    D.nlive = L.at<int32_t>(b, o_nl);
    D.rank = L.at<int32_t>(b, o_rk);
    D.inv_off = L.at<int32_t>(b, o_io);
    D.inv_cur = L.at<int32_t>(b, o_ic);
    D.post = L.at<uint16_t>(b, o_po);
    D.pending = L.at<unsigned long long>(b, o_pe);
    D.part = L.at<int32_t>(b, o_pt);
    // everything from nbow on starts at zero (no live slot, counter 0, no pending score)
    hipError_t e = hipMemsetAsync(b + o_nb, 0, L.total() - o_nb, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hipFree(db->d_mem);
        delete db;
        return set_err(ORBG_EIO, "KeyFrameDatabase: %s", hipGetErrorString(e));
    }
    db->stream = c->stream;
    *out = db;
    return ORBG_OK;
}

extern "C" void orbg_kfdb_destroy(orbg_kfdb *db)
{
    if (!db) return;
    hipSetDevice(db->device);
    if (db->d_mem) hipFree(db->d_mem);
    delete db;
}

extern "C" int orbg_kfdb_info(orbg_kfdb *db, int32_t *nlive, int32_t *max_keyframes, int32_t *cap,
                              int32_t *limit)
{
    if (!db) return set_err(ORBG_EINVAL, "database is NULL");
    if (max_keyframes) *max_keyframes = db->D.K;
    if (cap) *cap = db->D.cap;
    if (limit) *limit = ORBG_KFDB_MAX_KEYFRAMES;
    if (nlive) {
        *nlive = 0;
        if (db->touched) {
            HIPCHK(hipSetDevice(db->device));
            if (launch_place_count(db->stream, db->D)) return set_err(ORBG_EIO, "k_place_count launch failed");
            HIPCHK(hipMemcpyAsync(nlive, db->D.nlive, 4, hipMemcpyDeviceToHost, db->stream));
            HIPCHK(hipStreamSynchronize(db->stream));
        }
    }
    return ORBG_OK;
}

static int kfdb_enter(orbg_ctx *c, orbg_kfdb *db)
{
    if (!c || !db) return set_err(ORBG_EINVAL, "NULL context or database");
    if (db->device != c->device) return set_err(ORBG_EINVAL, "database lives on another device");
    HIPCHK(hipSetDevice(c->device));
    if (db->stream != c->stream) {  // the context's stream changed: finish what the old one holds
        if (db->touched) HIPCHK(hipStreamSynchronize(db->stream));
        db->stream = c->stream;
    }
    return ORBG_OK;
}

extern "C" int orbg_kfdb_add_batch_device(orbg_ctx *c, orbg_kfdb *db, const int32_t *d_slots,
                                          const orbg_bow_vectors *v, int vcap,
                                          const int32_t *d_index, int n)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!d_slots || !v || !v->words || !v->weights || !v->nbow)
        return set_err(ORBG_EINVAL, "NULL device array");
    if (vcap < 1 || vcap > db->D.cap)
        return set_err(ORBG_EINVAL, "vcap %d outside 1..%d (the database's cap)", vcap, db->D.cap);
    if ((rc = launch_place_add(c->stream, db->D, d_slots, *v, vcap, d_index, n, &c->prof)))
        return set_err(rc, "k_place_add launch failed");
    db->dirty = db->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_kfdb_add(orbg_ctx *c, orbg_kfdb *db, int slot, const int32_t *words,
                             const double *weights, int n)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    const PlaceDb &D = db->D;
    if (slot < 0 || slot >= D.K) return set_err(ORBG_EINVAL, "slot %d outside [0, %d)", slot, D.K);
    if (n < 0 || n > D.cap) return set_err(ORBG_EINVAL, "%d entries (cap %d)", n, D.cap);
    if (n && (!words || !weights)) return set_err(ORBG_EINVAL, "NULL array");
    for (int i = 0; i < n; i++) {
        if (words[i] < 0 || words[i] >= D.nwords)
            return set_err(ORBG_EINVAL, "word id %d outside [0, %d)", words[i], D.nwords);
        if (i && words[i] <= words[i - 1])
            return set_err(ORBG_EINVAL, "word ids not strictly ascending at entry %d", i);
    }
    int32_t live = 0;
    if (db->touched) {
        HIPCHK(hipMemcpyAsync(&live, D.live + slot, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (live) return set_err(ORBG_EINVAL, "slot %d is already live", slot);
    const int cap = std::max(n, 1);
    Layout L;
    const size_t o_w = L.take((size_t)cap * 4), o_x = L.take((size_t)cap * 8), o_n = L.take(4);
    const size_t o_s = L.take(4);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t nb = n, sl = slot;
    if (n) HIPCHK(hipMemcpyAsync(b + o_w, words, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(b + o_x, weights, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &nb, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_s, &sl, 4, hipMemcpyHostToDevice, c->stream));
    orbg_bow_vectors V{L.at<int32_t>(b, o_w), L.at<double>(b, o_x),
                       L.at<int32_t>(b, o_n)};
    if ((rc = launch_place_add(c->stream, D, L.at<int32_t>(b, o_s), V, cap, nullptr, 1, &c->prof)))
        return set_err(rc, "k_place_add launch failed");
    db->dirty = db->touched = true;
    HIPCHK(hipStreamSynchronize(c->stream));  // the scratch is the next host call's too
    c->prof.collect();
    return ORBG_OK;
}

extern "C" int orbg_kfdb_erase(orbg_ctx *c, orbg_kfdb *db, int slot)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (slot < 0 || slot >= db->D.K)
        return set_err(ORBG_EINVAL, "slot %d outside [0, %d)", slot, db->D.K);
    if (launch_place_erase(c->stream, db->D, slot)) return set_err(ORBG_EIO, "k_place_erase launch failed");
    db->dirty = db->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_kfdb_clear(orbg_ctx *c, orbg_kfdb *db)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(db->D.live, 0, (size_t)db->D.K * 4, c->stream));
    db->dirty = db->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_kfdb_rebuild(orbg_ctx *c, orbg_kfdb *db)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (!db->dirty) return ORBG_OK;
    if ((rc = launch_place_rebuild(c->stream, db->D, &c->prof)))
        return set_err(rc, "inverted file rebuild launch failed");
    db->dirty = false;
    db->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_kfdb_reloc_scores(orbg_ctx *c, orbg_kfdb *db, float *reloc_score)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (!reloc_score) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipMemcpyAsync(reloc_score, db->D.reloc, (size_t)db->D.K * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ORBG_OK;
}

static int kfdb_detect(orbg_ctx *c, orbg_kfdb *db, PlaceQuery &Q)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (Q.nq < 0 || Q.cand_cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (Q.nq == 0) return ORBG_OK;
    if (Q.qcap < 1 || Q.qcap > ORBG_KFDB_MAX_CAP)
        return set_err(ORBG_ENOTSUP, "qcap %d outside 1..%d", Q.qcap, ORBG_KFDB_MAX_CAP);
    if (!Q.q.words || !Q.q.weights || !Q.q.nbow || !Q.neigh || !Q.ncand || (Q.cand_cap && !Q.cand))
        return set_err(ORBG_EINVAL, "NULL device array");
    if (Q.loop) {
        if (Q.conn_cap < 0) return set_err(ORBG_EINVAL, "negative size");
        if (!Q.nconn || !Q.min_score || (Q.conn_cap && !Q.conn))
            return set_err(ORBG_EINVAL, "NULL device array");
    }
    if ((rc = orbg_kfdb_rebuild(c, db))) return rc;
    if ((rc = launch_place_query(c->stream, db->D, Q, &c->prof)))
        return set_err(rc, "k_place_query launch failed");
    db->touched = true;
    return ORBG_OK;
}

extern "C" int orbg_kfdb_detect_reloc_batch_device(orbg_ctx *c, orbg_kfdb *db,
                                                   const orbg_bow_vectors *q, int qcap,
                                                   const int32_t *d_qindex, int nq,
                                                   const int32_t *d_neigh, int32_t *d_cand,
                                                   int cand_cap, int32_t *d_ncand,
                                                   int32_t *d_max_common, int32_t *d_nscored)
{
    if (!c || !db || !q) return set_err(ORBG_EINVAL, "NULL argument");
    PlaceQuery Q{};
    Q.q = *q;
    Q.qcap = qcap;
    Q.nq = nq;
    Q.qindex = d_qindex;
    Q.neigh = d_neigh;
    Q.cand = d_cand;
    Q.cand_cap = cand_cap;
    Q.ncand = d_ncand;
    Q.max_common = d_max_common;
    Q.nscored = d_nscored;
    return kfdb_detect(c, db, Q);
}

extern "C" int orbg_kfdb_detect_loop_batch_device(orbg_ctx *c, orbg_kfdb *db,
                                                  const orbg_bow_vectors *q, int qcap,
                                                  const int32_t *d_qindex, int nq,
                                                  const int32_t *d_conn, int conn_cap,
                                                  const int32_t *d_nconn, const float *d_min_score,
                                                  const int32_t *d_neigh, int32_t *d_cand,
                                                  int cand_cap, int32_t *d_ncand,
                                                  int32_t *d_max_common, int32_t *d_nscored)
{
    if (!c || !db || !q) return set_err(ORBG_EINVAL, "NULL argument");
    PlaceQuery Q{};
    Q.q = *q;
    Q.qcap = qcap;
    Q.nq = nq;
    Q.qindex = d_qindex;
    Q.neigh = d_neigh;
    Q.conn = d_conn;
    Q.conn_cap = conn_cap;
    Q.nconn = d_nconn;
    Q.min_score = d_min_score;
    Q.loop = 1;
    Q.cand = d_cand;
    Q.cand_cap = cand_cap;
    Q.ncand = d_ncand;
    Q.max_common = d_max_common;
    Q.nscored = d_nscored;
    return kfdb_detect(c, db, Q);
}

// one query from host arrays: uploads, runs the batched form with nq = 1, downloads
static int kfdb_detect_host(orbg_ctx *c, orbg_kfdb *db, const int32_t *words,
                            const double *weights, int n, bool loop, const int32_t *conn,
                            int nconn, float min_score, const int32_t *neigh, int32_t *cand,
                            int cand_cap, int32_t *ncand, int32_t *max_common, int32_t *nscored)
{
    int rc = kfdb_enter(c, db);
    if (rc) return rc;
    if (!ncand || !neigh) return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0 || cand_cap < 0 || nconn < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n > ORBG_KFDB_MAX_CAP)
        return set_err(ORBG_ENOTSUP, "a BowVector with more than %d entries", ORBG_KFDB_MAX_CAP);
    if ((n && (!words || !weights)) || (nconn && !conn) || (cand_cap && !cand))
        return set_err(ORBG_EINVAL, "NULL array");
    const int cap = std::max(n, 1), K = db->D.K;
    Layout L;
    const size_t o_w = L.take((size_t)cap * 4), o_x = L.take((size_t)cap * 8), o_n = L.take(4);
    const size_t o_ng = L.take((size_t)K * ORBG_KFDB_NEIGH * 4), o_cn = L.take((size_t)nconn * 4);
    const size_t o_nc = L.take(4), o_ms = L.take(4), o_cd = L.take((size_t)cand_cap * 4);
    const size_t o_out = L.take(12);
    uint8_t *b;
    if ((rc = L.device(c, &b))) return rc;
    const int32_t nb = n, ncn = nconn;
    if (n) HIPCHK(hipMemcpyAsync(b + o_w, words, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(b + o_x, weights, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &nb, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_ng, neigh, (size_t)K * ORBG_KFDB_NEIGH * 4, hipMemcpyHostToDevice, c->stream));
    if (nconn) HIPCHK(hipMemcpyAsync(b + o_cn, conn, (size_t)nconn * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_nc, &ncn, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_ms, &min_score, 4, hipMemcpyHostToDevice, c->stream));
    PlaceQuery Q{};
    Q.q = orbg_bow_vectors{L.at<int32_t>(b, o_w), L.at<double>(b, o_x),
                           L.at<int32_t>(b, o_n)};
    Q.qcap = cap;
    Q.nq = 1;
    Q.neigh = L.at<int32_t>(b, o_ng);
    Q.conn = L.at<int32_t>(b, o_cn);
    Q.conn_cap = nconn;
    Q.nconn = L.at<int32_t>(b, o_nc);
    Q.min_score = L.at<float>(b, o_ms);
    Q.loop = loop ? 1 : 0;
    Q.cand = L.at<int32_t>(b, o_cd);
    Q.cand_cap = cand_cap;
    Q.ncand = L.at<int32_t>(b, o_out);
    Q.max_common = Q.ncand + 1;
    Q.nscored = Q.ncand + 2;
    if ((rc = kfdb_detect(c, db, Q))) return rc;
    int32_t out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, b + o_out, 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nw = std::min(out[0], cand_cap);
    if (nw > 0) HIPCHK(hipMemcpy(cand, b + o_cd, (size_t)nw * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *ncand = out[0];
    if (max_common) *max_common = out[1];
    if (nscored) *nscored = out[2];
    return ORBG_OK;
}

extern "C" int orbg_kfdb_detect_reloc(orbg_ctx *c, orbg_kfdb *db, const int32_t *words,
                                      const double *weights, int n, const int32_t *neigh,
                                      int32_t *cand, int cand_cap, int32_t *ncand,
                                      int32_t *max_common, int32_t *nscored)
{
    return kfdb_detect_host(c, db, words, weights, n, false, nullptr, 0, 0.0f, neigh, cand,
                            cand_cap, ncand, max_common, nscored);
}

extern "C" int orbg_kfdb_detect_loop(orbg_ctx *c, orbg_kfdb *db, const int32_t *words,
                                     const double *weights, int n, const int32_t *conn, int nconn,
                                     float min_score, const int32_t *neigh, int32_t *cand,
                                     int cand_cap, int32_t *ncand, int32_t *max_common,
                                     int32_t *nscored)
{
    return kfdb_detect_host(c, db, words, weights, n, true, conn, nconn, min_score, neigh, cand,
                            cand_cap, ncand, max_common, nscored);
}
