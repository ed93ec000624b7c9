// api_bow.hip -- orbg_vocab_*, orbg_bow_transform*, orbg_search_by_bow*
#include "orbg_ctx.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// DBoW2 vocabulary (TemplatedVocabulary::loadFromTextFile) + transform (Frame::ComputeBoW)
// ---------------------------------------------------------------------------
extern "C" int orbg_vocab_create(orbg_ctx *c, int k, int L, int scoring, int weighting,
                                 int nnodes, const int32_t *parent, const uint8_t *is_leaf,
                                 const uint8_t *desc, const double *weight, orbg_vocab **out)
{
    if (!c || !out) return set_err(ORBG_EINVAL, "NULL argument");
    *out = nullptr;
    // header checks of loadFromTextFile (TemplatedVocabulary.h:1359-1363)
    if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 ||
        weighting > 3)
        return set_err(ORBG_EINVAL, "k %d L %d scoring %d weighting %d outside the text format",
                       k, L, scoring, weighting);
    if (nnodes < 1) return set_err(ORBG_EINVAL, "a vocabulary has at least the root node");
    if (nnodes > 1 && (!parent || !is_leaf || !desc || !weight))
        return set_err(ORBG_EINVAL, "NULL node array");
    std::vector<int32_t> off(nnodes + 1, 0), word(nnodes, 0);
    int nwords = 0;
    for (int i = 1; i < nnodes; i++) {
        if (parent[i] < 0 || parent[i] >= i)
            return set_err(ORBG_EINVAL, "node %d: parent %d is not an earlier node", i, parent[i]);
        off[parent[i] + 1]++;
        if (is_leaf[i]) word[i] = nwords++;
    }
    int maxc = 0;
    for (int i = 0; i < nnodes; i++) {
        maxc = std::max(maxc, off[i + 1]);
        off[i + 1] += off[i];
    }
    if (maxc > 64) return set_err(ORBG_ENOTSUP, "a node with %d children (> 64)", maxc);
    std::vector<BowSlot> slots(std::max(nnodes - 1, 1));
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (int i = 1; i < nnodes; i++) {  // children in node (file) order
        BowSlot &s = slots[fill[parent[i]]++];
        memset(&s, 0, sizeof(s));
        memcpy(s.d, desc + (size_t)i * 32, 32);
        s.c0 = off[i];
        s.c1 = off[i + 1];
        s.node = i;
        s.word = word[i];
        s.weight = weight[i];
    }
    auto *v = new orbg_vocab();
    v->device = c->device;
    v->k = k;
    v->L = L;
    v->scoring = scoring;
    v->weighting = weighting;
    v->nnodes = nnodes;
    v->nwords = nwords;
    v->group = maxc <= 16 ? 16 : maxc <= 32 ? 32 : 64;
    v->root_c0 = off[0];
    v->root_c1 = off[1];
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMalloc(&v->d_slots, slots.size() * sizeof(BowSlot));
    if (e == hipSuccess)
        e = hipMemcpy(v->d_slots, slots.data(), slots.size() * sizeof(BowSlot), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (v->d_slots) hipFree(v->d_slots);
        delete v;
        return set_err(ORBG_ENOMEM, "vocabulary upload: %s", hipGetErrorString(e));
    }
    *out = v;
    return ORBG_OK;
}

extern "C" int orbg_vocab_load_text(orbg_ctx *c, const char *path, orbg_vocab **out)
{
    if (!c || !path || !out) return set_err(ORBG_EINVAL, "NULL argument");
    FILE *fp = fopen(path, "r");
    if (!fp) return set_err(ORBG_EINVAL, "cannot open %s", path);
    char *line = nullptr;
    size_t cap = 0;
    int k = 0, L = 0, n1 = 0, n2 = 0, rc = ORBG_OK;
    std::vector<int32_t> parent(1, 0);
    std::vector<uint8_t> leaf(1, 0), desc(32, 0);
    std::vector<double> weight(1, 0.0);
    if (getline(&line, &cap, fp) < 0 || sscanf(line, "%d %d %d %d", &k, &L, &n1, &n2) != 4) {
        rc = set_err(ORBG_EINVAL, "%s: missing header line", path);
    } else {
        long lineno = 1;
        while (getline(&line, &cap, fp) >= 0) {
            lineno++;
            char *p = line, *e;
            while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
            if (!*p) continue;  // blank line
            long vals[34];
            int nv = 0;
            for (; nv < 34; nv++) {
                vals[nv] = strtol(p, &e, 10);
                if (e == p) break;
                p = e;
            }
            const double w = strtod(p, &e);
            if (nv < 34 || e == p) {
                rc = set_err(ORBG_EINVAL, "%s:%ld: expected parent isLeaf 32 bytes weight", path,
                             lineno);
                break;
            }
            parent.push_back((int32_t)vals[0]);
            leaf.push_back(vals[1] > 0);
            for (int j = 0; j < 32; j++) desc.push_back((uint8_t)vals[2 + j]);
            weight.push_back(w);
        }
    }
    free(line);
    fclose(fp);
    if (rc) return rc;
    return orbg_vocab_create(c, k, L, n1, n2, (int)parent.size(), parent.data(), leaf.data(),
                             desc.data(), weight.data(), out);
}

extern "C" void orbg_vocab_destroy(orbg_vocab *v)
{
    if (!v) return;
    if (v->d_slots) {
        hipSetDevice(v->device);
        hipFree(v->d_slots);
    }
    delete v;
}

extern "C" int orbg_vocab_info(const orbg_vocab *v, int32_t *k, int32_t *L, int32_t *scoring,
                               int32_t *weighting, int32_t *nnodes, int32_t *nwords)
{
    if (!v) return set_err(ORBG_EINVAL, "vocabulary is NULL");
    if (k) *k = v->k;
    if (L) *L = v->L;
    if (scoring) *scoring = v->scoring;
    if (weighting) *weighting = v->weighting;
    if (nnodes) *nnodes = v->nnodes;
    if (nwords) *nwords = v->nwords;
    return ORBG_OK;
}

#define ORBG_BOW_MAX_CAP 8192   // k_bow_vectors sorts a frame's keys in LDS

static BowArgs bow_args(const orbg_vocab *v, int levelsup)
{
    BowArgs A{};
    A.slots = v->d_slots;
    A.root_c0 = v->root_c0;
    A.root_c1 = v->root_c1;
    A.group = v->group;
    A.nid_level = v->L - levelsup;
    A.scoring = v->scoring;
    A.weighting = v->weighting;
    A.empty = v->nwords == 0;
    return A;
}

extern "C" int orbg_bow_transform_batch_device(orbg_ctx *c, const orbg_vocab *v,
                                               const uint8_t *desc, const int32_t *counts,
                                               int cap, int nframes, int levelsup,
                                               int32_t *bow_words, double *bow_weights,
                                               int32_t *nbow, int32_t *fv_nodes,
                                               int32_t *fv_off, int32_t *fv_feats, int32_t *nfv,
                                               int32_t *word_of, int32_t *node_of)
{
    if (!c || !v) return set_err(ORBG_EINVAL, "NULL context or vocabulary");
    if (v->device != c->device) return set_err(ORBG_EINVAL, "vocabulary lives on another device");
    if (nframes <= 0) return ORBG_OK;
    if (cap < 1 || cap > ORBG_BOW_MAX_CAP)
        return set_err(ORBG_ENOTSUP, "cap %d outside 1..%d", cap, ORBG_BOW_MAX_CAP);
    if (!desc || !counts || !bow_words || !bow_weights || !nbow || !fv_nodes || !fv_off ||
        !fv_feats || !nfv)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    const size_t per = (size_t)nframes * cap;
    const size_t o_w = 0, o_n = al256(per * 4), o_x = o_n + al256(per * 4);
    void *s;
    int rc = scratch(c, o_x + al256(per * 8), &s);
    if (rc) return rc;
    BowArgs A = bow_args(v, levelsup);
    A.desc = desc;
    A.counts = counts;
    A.cap = cap;
    A.nframes = nframes;
    A.fword = word_of ? word_of : (int32_t *)((uint8_t *)s + o_w);
    A.fnode = node_of ? node_of : (int32_t *)((uint8_t *)s + o_n);
    A.fweight = (double *)((uint8_t *)s + o_x);
    A.bow_words = bow_words;
    A.bow_weights = bow_weights;
    A.nbow = nbow;
    A.fv_nodes = fv_nodes;
    A.fv_off = fv_off;
    A.fv_feats = fv_feats;
    A.nfv = nfv;
    if ((rc = launch_bow(c->stream, A, &c->prof))) return set_err(rc, "bow launch failed");
    return ORBG_OK;
}

extern "C" int orbg_bow_transform(orbg_ctx *c, const orbg_vocab *v, const uint8_t *desc, int n,
                                  int levelsup, int32_t *bow_words, double *bow_weights,
                                  int *nbow, int32_t *fv_nodes, int32_t *fv_off,
                                  int32_t *fv_feats, int *nfv)
{
    if (!c || !v || !nbow || !nfv || !fv_off) return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n > ORBG_BOW_MAX_CAP) return set_err(ORBG_ENOTSUP, "%d descriptors (> %d)", n, ORBG_BOW_MAX_CAP);
    if (n > 0 && (!desc || !bow_words || !bow_weights || !fv_nodes || !fv_feats))
        return set_err(ORBG_EINVAL, "NULL array");
    *nbow = *nfv = 0;
    fv_off[0] = 0;
    if (n == 0) return ORBG_OK;
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_d = L.take((size_t)n * 32), o_c = L.take(4), o_fw = L.take((size_t)n * 4);
    const size_t o_fn = L.take((size_t)n * 4), o_fx = L.take((size_t)n * 8);
    const size_t o_bw = L.take((size_t)n * 4), o_bx = L.take((size_t)n * 8), o_nb = L.take(4);
    const size_t o_vn = L.take((size_t)n * 4), o_vo = L.take((size_t)(n + 1) * 4);
    const size_t o_vf = L.take((size_t)n * 4), o_nf = L.take(4);
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    const int32_t cnt = n;
    HIPCHK(hipMemcpyAsync(b + o_d, desc, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, &cnt, 4, hipMemcpyHostToDevice, c->stream));
    BowArgs A = bow_args(v, levelsup);
    A.desc = b + o_d;
    A.counts = L.at<int32_t>(b, o_c);
    A.cap = n;
    A.nframes = 1;
    A.fword = L.at<int32_t>(b, o_fw);
    A.fnode = L.at<int32_t>(b, o_fn);
    A.fweight = L.at<double>(b, o_fx);
    A.bow_words = L.at<int32_t>(b, o_bw);
    A.bow_weights = L.at<double>(b, o_bx);
    A.nbow = L.at<int32_t>(b, o_nb);
    A.fv_nodes = L.at<int32_t>(b, o_vn);
    A.fv_off = L.at<int32_t>(b, o_vo);
    A.fv_feats = L.at<int32_t>(b, o_vf);
    A.nfv = L.at<int32_t>(b, o_nf);
    if ((rc = launch_bow(c->stream, A, &c->prof))) return set_err(rc, "bow launch failed");
    int32_t nb = 0, nf = 0;
    HIPCHK(hipMemcpyAsync(&nb, b + o_nb, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&nf, b + o_nf, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // outputs are at most n long; copy what was produced
    HIPCHK(hipMemcpyAsync(bow_words, b + o_bw, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(bow_weights, b + o_bx, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(fv_nodes, b + o_vn, (size_t)nf * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(fv_off, b + o_vo, (size_t)(nf + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    int32_t m = 0;
    HIPCHK(hipMemcpyAsync(&m, b + o_vo + (size_t)nf * 4, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (m) HIPCHK(hipMemcpy(fv_feats, b + o_vf, (size_t)m * 4, hipMemcpyDeviceToHost));
    c->prof.collect();
    *nbow = nb;
    *nfv = nf;
    return ORBG_OK;
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (bow_match_kernels.hip)
// ---------------------------------------------------------------------------
extern "C" int orbg_search_by_bow_kf_batch_device(orbg_ctx *c, const orbg_bow_frames *kf1,
                                                  const orbg_bow_frames *kf2, int cap,
                                                  const int32_t *d_kf1_index,
                                                  const int32_t *d_kf2_index, int npairs,
                                                  float nnratio, int check_ori,
                                                  int32_t *d_match12, int32_t *d_nmatch)
{
    if (!c || !kf1 || !kf2) return set_err(ORBG_EINVAL, "NULL argument");
    if (npairs < 0 || cap <= 0 || cap > 8192) return set_err(ORBG_EINVAL, "bad npairs / cap");
    if (npairs == 0) return ORBG_OK;
    if (!d_kf1_index || !d_kf2_index || !d_match12 || !d_nmatch || !kf1->desc || !kf1->kps ||
        !kf1->counts || !kf1->fv_nodes || !kf1->fv_off || !kf1->fv_feats || !kf1->nfv ||
        !kf2->desc || !kf2->kps || !kf2->fv_nodes || !kf2->fv_off || !kf2->fv_feats || !kf2->nfv)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(order_after_caller(c));
    hipStream_t st = c->mstream;  // PROF_LAUNCH records on `st`
    int rc = 0;
    PROF_LAUNCH(c, "bow_match_kf",
                rc = launch_bow_match(st, *kf1, *kf2, cap, d_kf1_index, d_kf2_index, npairs,
                                      nnratio, check_ori, d_match12, d_nmatch, true));
    if (rc == ORBG_ENOTSUP) return set_err(ORBG_ENOTSUP, "SearchByBoW: more than 4096 features per frame");
    if (rc) return set_err(ORBG_EIO, "k_bow_match launch failed");
    return ORBG_OK;
}

extern "C" int orbg_search_by_bow_batch_device(orbg_ctx *c, const orbg_bow_frames *kf,
                                               const orbg_bow_frames *f, int cap,
                                               const int32_t *d_kf_index, const int32_t *d_f_index,
                                               int npairs, float nnratio, int check_ori,
                                               int32_t *d_match, int32_t *d_nmatch)
{
    if (!c || !kf || !f) return set_err(ORBG_EINVAL, "NULL argument");
    if (npairs < 0 || cap <= 0 || cap > 8192) return set_err(ORBG_EINVAL, "bad npairs / cap");
    if (npairs == 0) return ORBG_OK;
    if (!d_kf_index || !d_f_index || !d_match || !d_nmatch || !kf->desc || !kf->kps ||
        !kf->fv_nodes || !kf->fv_off || !kf->fv_feats || !kf->nfv || !f->desc || !f->kps ||
        !f->counts || !f->fv_nodes || !f->fv_off || !f->fv_feats || !f->nfv)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(order_after_caller(c));
    hipStream_t st = c->mstream;  // PROF_LAUNCH records on `st`
    int rc = 0;
    PROF_LAUNCH(c, "bow_match",
                rc = launch_bow_match(st, *kf, *f, cap, d_kf_index, d_f_index, npairs, nnratio,
                                      check_ori, d_match, d_nmatch));
    if (rc == ORBG_ENOTSUP) return set_err(ORBG_ENOTSUP, "SearchByBoW: more than 4096 features per frame");
    if (rc) return set_err(ORBG_EIO, "k_bow_match launch failed");
    return ORBG_OK;
}

static int search_by_bow_host(orbg_ctx *c, const uint8_t *kf_desc, const float *kf_angle,
                                  const uint8_t *kf_valid, int n_kf, const int32_t *kf_fv_nodes,
                                  const int32_t *kf_fv_off, const int32_t *kf_fv_feats, int kf_nfv,
                                  const uint8_t *f_desc, const float *f_angle,
                                  const uint8_t *f_valid, int n_f,
                                  const int32_t *f_fv_nodes, const int32_t *f_fv_off,
                                  const int32_t *f_fv_feats, int f_nfv, float nnratio,
                                  int check_ori, int32_t *match, int *nmatches, bool kfkf)
{
    const int n_out = kfkf ? n_kf : n_f;  // KeyFrame-KeyFrame: vpMatches12 over pKF1
    if (!c || !match || !nmatches) return set_err(ORBG_EINVAL, "NULL argument");
    if (n_kf < 0 || n_f < 0 || kf_nfv < 0 || f_nfv < 0 || kf_nfv > std::max(n_kf, 0) ||
        f_nfv > std::max(n_f, 0))
        return set_err(ORBG_EINVAL, "bad sizes");
    if ((n_kf && (!kf_desc || !kf_angle)) || (n_f && (!f_desc || !f_angle)) ||
        (kf_nfv && (!kf_fv_nodes || !kf_fv_off || !kf_fv_feats)) ||
        (f_nfv && (!f_fv_nodes || !f_fv_off || !f_fv_feats)))
        return set_err(ORBG_EINVAL, "NULL input array");
    *nmatches = 0;
    for (int i = 0; i < n_out; i++) match[i] = -1;
    if (!n_f || !n_kf || !kf_nfv || !f_nfv) return ORBG_OK;
    for (int j = 0; j < kf_nfv; j++)
        for (int k = kf_fv_off[j]; k < kf_fv_off[j + 1]; k++)
            if (kf_fv_feats[k] < 0 || kf_fv_feats[k] >= n_kf)
                return set_err(ORBG_EINVAL, "KF feature index out of range");
    for (int j = 0; j < f_nfv; j++)
        for (int k = f_fv_off[j]; k < f_fv_off[j + 1]; k++)
            if (f_fv_feats[k] < 0 || f_fv_feats[k] >= n_f)
                return set_err(ORBG_EINVAL, "F feature index out of range");
    HIPCHK(hipSetDevice(c->device));
    // one buffer: two frames (KF = 0, F = 1) at cap = max(n_kf, n_f)
    const int cap = std::max(n_kf, n_f);
    if (cap > 8192) return set_err(ORBG_ENOTSUP, "more than 8192 features");
    const size_t cp = (size_t)cap;
    Layout L;
    const size_t o_desc = L.take(2 * cp * 32), o_kps = L.take(2 * cp * sizeof(orbg_keypoint)),
                 o_cnt = L.take(2 * 4), o_nodes = L.take(2 * cp * 4), o_off = L.take(2 * (cp + 1) * 4),
                 o_feats = L.take(2 * cp * 4), o_nfv = L.take(2 * 4), o_val = L.take(2 * cp),
                 o_idx = L.take(2 * 4), o_match = L.take(cp * 4), o_nm = L.take(4);
    uint8_t *hs, *db;
    int rc = L.host(c, &hs);
    if (rc) return rc;
    memset(hs, 0, L.total());
    memcpy(hs + o_desc, kf_desc, (size_t)n_kf * 32);
    memcpy(hs + o_desc + cp * 32, f_desc, (size_t)n_f * 32);
    orbg_keypoint *hk = L.at<orbg_keypoint>(hs, o_kps);
    for (int i = 0; i < n_kf; i++) hk[i].angle = kf_angle[i];
    for (int i = 0; i < n_f; i++) hk[cp + i].angle = f_angle[i];
    int32_t *hc = L.at<int32_t>(hs, o_cnt);
    hc[0] = n_kf;
    hc[1] = n_f;
    memcpy(hs + o_nodes, kf_fv_nodes, (size_t)kf_nfv * 4);
    memcpy(hs + o_nodes + cp * 4, f_fv_nodes, (size_t)f_nfv * 4);
    memcpy(hs + o_off, kf_fv_off, (size_t)(kf_nfv + 1) * 4);
    memcpy(hs + o_off + (cp + 1) * 4, f_fv_off, (size_t)(f_nfv + 1) * 4);
    memcpy(hs + o_feats, kf_fv_feats, (size_t)kf_fv_off[kf_nfv] * 4);
    memcpy(hs + o_feats + cp * 4, f_fv_feats, (size_t)f_fv_off[f_nfv] * 4);
    int32_t *hn = L.at<int32_t>(hs, o_nfv);
    hn[0] = kf_nfv;
    hn[1] = f_nfv;
    if (kf_valid)
        memcpy(hs + o_val, kf_valid, (size_t)n_kf);
    else
        memset(hs + o_val, 1, (size_t)n_kf);
    if (f_valid)
        memcpy(hs + o_val + cp, f_valid, (size_t)n_f);
    else
        memset(hs + o_val + cp, 1, (size_t)n_f);
    int32_t *hi = L.at<int32_t>(hs, o_idx);
    hi[0] = 0;
    hi[1] = 1;
    if ((rc = L.device(c, &db))) return rc;
    HIPCHK(hipMemcpyAsync(db, hs, L.total(), hipMemcpyHostToDevice, c->stream));
    orbg_bow_frames K{}, F{};
    K.desc = F.desc = db + o_desc;
    K.kps = F.kps = L.at<orbg_keypoint>(db, o_kps);
    K.counts = F.counts = L.at<int32_t>(db, o_cnt);
    K.fv_nodes = F.fv_nodes = L.at<int32_t>(db, o_nodes);
    K.fv_off = F.fv_off = L.at<int32_t>(db, o_off);
    K.fv_feats = F.fv_feats = L.at<int32_t>(db, o_feats);
    K.nfv = F.nfv = L.at<int32_t>(db, o_nfv);
    K.valid = F.valid = db + o_val;  // frame 0 (KF / pKF1) and frame 1 (F / pKF2) at + cap
    const int32_t *di = L.at<int32_t>(db, o_idx);
    rc = launch_bow_match(c->stream, K, F, cap, di, di + 1, 1, nnratio, check_ori,
                          L.at<int32_t>(db, o_match), L.at<int32_t>(db, o_nm), kfkf);
    if (rc == ORBG_ENOTSUP) return set_err(ORBG_ENOTSUP, "SearchByBoW: more than 4096 features per frame");
    if (rc) return set_err(ORBG_EIO, "k_bow_match launch failed");
    HIPCHK(hipMemcpyAsync(hs + o_match, db + o_match, cp * 4 + 256, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(match, hs + o_match, (size_t)n_out * 4);
    memcpy(nmatches, hs + o_nm, 4);
    return ORBG_OK;
}

extern "C" int orbg_search_by_bow(orbg_ctx *c, const uint8_t *kf_desc, const float *kf_angle,
                                  const uint8_t *kf_valid, int n_kf, const int32_t *kf_fv_nodes,
                                  const int32_t *kf_fv_off, const int32_t *kf_fv_feats, int kf_nfv,
                                  const uint8_t *f_desc, const float *f_angle, int n_f,
                                  const int32_t *f_fv_nodes, const int32_t *f_fv_off,
                                  const int32_t *f_fv_feats, int f_nfv, float nnratio,
                                  int check_ori, int32_t *match, int *nmatches)
{
    return search_by_bow_host(c, kf_desc, kf_angle, kf_valid, n_kf, kf_fv_nodes, kf_fv_off,
                              kf_fv_feats, kf_nfv, f_desc, f_angle, nullptr, n_f, f_fv_nodes,
                              f_fv_off, f_fv_feats, f_nfv, nnratio, check_ori, match, nmatches,
                              false);
}

extern "C" int orbg_search_by_bow_kf(orbg_ctx *c, const uint8_t *desc1, const float *angle1,
                                     const uint8_t *valid1, int n1, const int32_t *fv_nodes1,
                                     const int32_t *fv_off1, const int32_t *fv_feats1, int nfv1,
                                     const uint8_t *desc2, const float *angle2,
                                     const uint8_t *valid2, int n2, const int32_t *fv_nodes2,
                                     const int32_t *fv_off2, const int32_t *fv_feats2, int nfv2,
                                     float nnratio, int check_ori, int32_t *match12,
                                     int *nmatches)
{
    return search_by_bow_host(c, desc1, angle1, valid1, n1, fv_nodes1, fv_off1, fv_feats1, nfv1,
                              desc2, angle2, valid2, n2, fv_nodes2, fv_off2, fv_feats2, nfv2,
                              nnratio, check_ori, match12, nmatches, true);
}
