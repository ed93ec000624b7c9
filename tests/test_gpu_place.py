"""GPU: place recognition through the C ABI (orbg_bow_score*, orbg_kfdb_*) against
tests/ref_place.py, the independent pure-Python statement of L1Scoring::score
(ScoringObject.cpp:23-68) and KeyFrameDatabase (KeyFrameDatabase.cc:106-419).  Everything is
compared exactly: scores as uint64 views (the sign of zero included), candidate lists with
their order, ncand / maxCommonWords / nscores, and every slot's stored mRelocScore.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from orb_slam2_test_amd import KeyFrameDatabase, ORBVocabulary, synthetic as S
from orb_slam2_test_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_place as R  # noqa: E402

pytestmark = pytest.mark.gpu

NKF, CAP, NQ, SEEDS = 40, 64, 8, (0, 1, 2)


def gpu_vocab(voc):
    return ORBVocabulary.from_tree(voc["k"], voc["L"], voc["scoring"], voc["weighting"],
                                   voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])


@pytest.fixture(scope="module")
def voc():
    v = gpu_vocab(S.vocabulary(10, 3, seed=S.DEFAULT_SEED + 5))
    assert v.size() == 1000
    return v


@pytest.fixture(scope="module")
def voc20():
    v = gpu_vocab(S.vocabulary(20, 1, seed=S.DEFAULT_SEED + 6))
    assert v.size() == R.HAND_NWORDS
    return v


def ctx():
    from orb_slam2_test_amd.orbmatcher import _ctx
    return _ctx(0)


def pack(bows, cap):
    """BowVectors (dicts) -> orbg_bow_vectors layout as host arrays."""
    w = np.full((len(bows), cap), -1, np.int32)
    x = np.zeros((len(bows), cap), np.float64)
    n = np.zeros(len(bows), np.int32)
    for i, b in enumerate(bows):
        k = sorted(b)
        n[i] = len(k)
        w[i, :len(k)] = k
        x[i, :len(k)] = [b[j] for j in k]
    return w, x, n


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def dev_vectors(bows, cap):
    t = [dev(a) for a in pack(bows, cap)]
    return t, {"words": t[0].data_ptr(), "weights": t[1].data_ptr(), "nbow": t[2].data_ptr()}


def u64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def scored_slots(info):
    return [s for s, c in info["counts"].items() if c > info["min_common"]]


# ---------------------------------------------------------------------------
# the reference results, computed once
# ---------------------------------------------------------------------------
def ref_db(kfs, neigh):
    db = R.RefKeyFrameDatabase(1000, NKF)
    for s, b in enumerate(kfs):
        db.add(s, b)
    db.set_neighbours(neigh)
    return db


@pytest.fixture(scope="module")
def cases():
    out = {}
    for seed in SEEDS:
        kfs, neigh, qs = R.place_dataset(seed, nkf=NKF, nq=NQ)
        c = {"kfs": kfs, "neigh": neigh, "qs": qs}
        # one call of NQ queries: each reads the scores as they were at the start (all 0);
        # afterwards a slot holds the score from the highest-indexed query that scored it
        stored = np.zeros(NKF, np.float32)
        c["batch"] = []
        reads = 0
        for q in qs:
            db, info = ref_db(kfs, neigh), {}
            cand = db.DetectRelocalizationCandidates(q, info)
            c["batch"].append((cand, info))
            reads += db.stored_reads
            sc = db.reloc_scores()
            for s in scored_slots(info):
                stored[s] = sc[s]
        c["batch_stored"], c["batch_reads"] = stored, reads
        # NQ single-query calls in sequence: the reference's own use
        db = ref_db(kfs, neigh)
        c["seq"] = []
        for q in qs:
            info = {}
            cand = db.DetectRelocalizationCandidates(q, info)
            c["seq"].append((cand, info, db.reloc_scores().copy()))
        c["seq_reads"] = db.stored_reads
        # loop detection: connected sets of 0..12 slots, minScore as LoopClosing::DetectLoop
        rng = np.random.default_rng(seed + 100)
        c["conn"] = [rng.choice(NKF, int(rng.integers(0, 13)), replace=False).tolist() for _ in qs]
        c["conn_scores"] = [[R.l1_score(q, kfs[s]) for s in cn] for q, cn in zip(qs, c["conn"])]
        c["min_score"] = [min([np.float32(1)] + [np.float32(v) for v in sc])
                          for sc in c["conn_scores"]]
        db = ref_db(kfs, neigh)
        c["loop"] = []
        for q, cn, ms in zip(qs, c["conn"], c["min_score"]):
            info = {}
            c["loop"].append((db.DetectLoopCandidates(q, cn, ms, info), info))
        out[seed] = c
    return out


def gpu_db(voc, kfs, max_keyframes=NKF, cap=CAP):
    db = KeyFrameDatabase(voc, max_keyframes, cap=cap)
    for s, b in enumerate(kfs):
        db.add(s, b)
    return db


def run_reloc_batch(db, qs, neigh, cand_cap=NKF, qindex=None):
    import torch
    keep, v = dev_vectors(qs, CAP)
    nq = len(qs) if qindex is None else len(qindex)
    t_ng = dev(neigh)
    t_qi = None if qindex is None else dev(np.asarray(qindex, np.int32))
    t_c = torch.full((max(nq, 1) * cand_cap,), -7, dtype=torch.int32, device="cuda")
    t_n, t_m, t_s = (torch.full((max(nq, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    db.detect_reloc_batch_device(v, CAP, None if t_qi is None else t_qi.data_ptr(), nq,
                                 t_ng.data_ptr(), t_c.data_ptr(), cand_cap, t_n.data_ptr(),
                                 t_m.data_ptr(), t_s.data_ptr(), ctx())
    ctx().sync()
    del keep
    return (t_c.cpu().numpy().reshape(-1, cand_cap) if cand_cap else None, t_n.cpu().numpy(),
            t_m.cpu().numpy(), t_s.cpu().numpy())


# ---------------------------------------------------------------------------
# score
# ---------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 700)


def test_score_bits_host_and_batch(voc):
    import torch
    rng = np.random.default_rng(11)

    def vec(n):
        w = rng.choice(1000, n, replace=False)
        x = rng.uniform(0.01, 1.0, n)
        return {int(a): float(b) for a, b in zip(w, x / max(x.sum(), 1e-300))}

    va, vb = [vec(n) for n in SIZES], [vec(n) for n in SIZES]
    pairs = [(i, j) for i in range(6) for j in range(6)]
    ref = np.array([R.l1_score(va[i], vb[j]) for i, j in pairs])
    assert (u64(ref) == 1 << 63).any() and (ref > 0).sum() >= 16       # -0.0 and real overlaps
    host = np.array([voc.score(va[i], vb[j]) for i, j in pairs])
    assert np.array_equal(u64(host), u64(ref))
    ka, a = dev_vectors(va, 700)
    kb, b = dev_vectors(vb, 700)
    ia, ib = dev(np.array([p[0] for p in pairs], np.int32)), dev(np.array([p[1] for p in pairs], np.int32))
    out = torch.full((36,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    voc.score_batch_device(a, b, 700, ia.data_ptr(), ib.data_ptr(), 36, out.data_ptr(), ctx())
    ctx().sync()
    assert np.array_equal(u64(out.cpu().numpy()), u64(ref))
    # a vector against itself, through the same kernel (NULL index arrays: pair p = (p, p))
    voc.score_batch_device(a, a, 700, None, None, 6, out.data_ptr(), ctx())
    ctx().sync()
    assert np.array_equal(u64(out.cpu().numpy()[:6]), u64([R.l1_score(v, v) for v in va]))


# ---------------------------------------------------------------------------
# relocalization
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_reloc_parity(voc, cases, seed):
    c = cases[seed]
    # the reference alone: the recipe reaches the cases this test is about
    cands = [x[0] for x in c["batch"]]
    assert all(len(x) >= 1 for x in cands) and any(len(x) >= 2 for x in cands)
    infos = [x[1] for x in c["batch"]]
    assert any(i["min_common"] in i["counts"].values() for i in infos)
    assert any(i["min_common"] + 1 in i["counts"].values() for i in infos)
    assert c["batch_reads"] > 0 and c["seq_reads"] > 0

    # NQ queries in one call
    db = gpu_db(voc, c["kfs"])
    assert db.info() == (NKF, NKF, CAP, db.info()[3]) and db.info()[3] >= 8192
    assert np.array_equal(db.reloc_scores(), np.zeros(NKF, np.float32))
    cand, ncand, maxc, nsc = run_reloc_batch(db, c["qs"], c["neigh"])
    for q, (rc, info) in enumerate(c["batch"]):
        print("seed", seed, "query", q, "ref", rc, "gpu", cand[q, :max(ncand[q], 0)].tolist())
        assert ncand[q] == len(rc) and cand[q, :len(rc)].tolist() == rc
        assert (cand[q, len(rc):] == -7).all()
        assert maxc[q] == info["max_common"] and nsc[q] == info["nscored"]
    assert np.array_equal(db.reloc_scores().view(np.uint32), c["batch_stored"].view(np.uint32))

    # the same queries as NQ single-query calls in sequence (host form)
    db = gpu_db(voc, c["kfs"])
    for q, (rc, info, stored) in zip(c["qs"], c["seq"]):
        got = db.detect_reloc(q, c["neigh"])
        assert got == (rc, len(rc), info["max_common"], info["nscored"])
        assert np.array_equal(db.reloc_scores().view(np.uint32), stored.view(np.uint32))


def test_reloc_parity_300_keyframes_10k_words():
    """More slots than a workgroup has threads (300, no multiple of 64) and a vocabulary the
    rebuild's scan needs several passes for (10^4 words): one batched call and one loop call
    against the reference."""
    K = 300
    v = gpu_vocab(S.vocabulary(10, 4, seed=S.DEFAULT_SEED + 7))
    assert v.size() == 10 ** 4
    kfs, neigh, qs = R.place_dataset(5, nwords=10 ** 4, nkf=K, nq=NQ)
    db = gpu_db(v, kfs, max_keyframes=K)
    cand, ncand, maxc, nsc = run_reloc_batch(db, qs, neigh, cand_cap=K)
    stored = np.zeros(K, np.float32)
    for q, bow in enumerate(qs):
        ref, info = R.RefKeyFrameDatabase(10 ** 4, K), {}
        for s, b in enumerate(kfs):
            ref.add(s, b)
        ref.set_neighbours(neigh)
        rc = ref.DetectRelocalizationCandidates(bow, info)
        assert len(rc) >= 1
        assert ncand[q] == len(rc) and cand[q, :len(rc)].tolist() == rc
        assert maxc[q] == info["max_common"] and nsc[q] == info["nscored"]
        sc = ref.reloc_scores()
        for s in scored_slots(info):
            stored[s] = sc[s]
        conn = list(range(q, K, 7))
        rl = ref.DetectLoopCandidates(bow, conn, 0.01, info)
        assert db.detect_loop(bow, conn, 0.01, neigh) == (rl, len(rl), info["max_common"],
                                                          info["nscored"])
    assert np.array_equal(db.reloc_scores().view(np.uint32), stored.view(np.uint32))


def test_reloc_determinism(voc, cases):
    c = cases[1]
    a, b = gpu_db(voc, c["kfs"]), gpu_db(voc, c["kfs"])
    ra, rb = run_reloc_batch(a, c["qs"], c["neigh"]), run_reloc_batch(b, c["qs"], c["neigh"])
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    s1 = a.reloc_scores()
    assert np.array_equal(s1.view(np.uint32), b.reloc_scores().view(np.uint32))
    # the second and third call on one database both start from the first call's scores
    r2 = run_reloc_batch(a, c["qs"], c["neigh"])
    s2 = a.reloc_scores()
    r3 = run_reloc_batch(a, c["qs"], c["neigh"])
    assert all(np.array_equal(x, y) for x, y in zip(r2, r3))
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    assert np.array_equal(s2.view(np.uint32), a.reloc_scores().view(np.uint32))


# ---------------------------------------------------------------------------
# loop detection
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_loop_parity(voc, cases, seed):
    import torch
    c = cases[seed]
    db = gpu_db(voc, c["kfs"])
    # minScore as LoopClosing::DetectLoop (LoopClosing.cc:162-177): the minimum float score
    # over the connected KeyFrames, through orbg_bow_score_batch_device
    keep_q, vq = dev_vectors(c["qs"], CAP)
    keep_k, vk = dev_vectors(c["kfs"], CAP)
    pa = [q for q, cn in enumerate(c["conn"]) for _ in cn]
    pb = [s for cn in c["conn"] for s in cn]
    assert len(pa) > 0
    ia, ib = dev(np.array(pa, np.int32)), dev(np.array(pb, np.int32))
    sc = torch.zeros(len(pa), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    voc.score_batch_device(vq, vk, CAP, ia.data_ptr(), ib.data_ptr(), len(pa), sc.data_ptr(), ctx())
    ctx().sync()
    sc = sc.cpu().numpy()
    assert np.array_equal(u64(sc), u64([v for row in c["conn_scores"] for v in row]))
    min_score = np.ones(NQ, np.float32)
    for q, v in zip(pa, sc):
        min_score[q] = min(min_score[q], np.float32(v))
    assert np.array_equal(min_score, np.array(c["min_score"], np.float32))

    conn = np.full((NQ, 12), -1, np.int32)
    nconn = np.array([len(cn) for cn in c["conn"]], np.int32)
    for q, cn in enumerate(c["conn"]):
        conn[q, :len(cn)] = cn
    t_conn, t_nconn, t_ms, t_ng = dev(conn), dev(nconn), dev(min_score), dev(c["neigh"])
    t_c = torch.full((NQ * NKF,), -7, dtype=torch.int32, device="cuda")
    t_n, t_m, t_s = (torch.full((NQ,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    db.detect_loop_batch_device(vq, CAP, None, NQ, t_conn.data_ptr(), 12, t_nconn.data_ptr(),
                                t_ms.data_ptr(), t_ng.data_ptr(), t_c.data_ptr(), NKF,
                                t_n.data_ptr(), t_m.data_ptr(), t_s.data_ptr(), ctx())
    ctx().sync()
    cand, ncand = t_c.cpu().numpy().reshape(NQ, NKF), t_n.cpu().numpy()
    maxc, nsc = t_m.cpu().numpy(), t_s.cpu().numpy()
    assert any(len(x[0]) >= 1 for x in c["loop"])
    for q, (rc, info) in enumerate(c["loop"]):
        print("seed", seed, "query", q, "ref", rc, "gpu", cand[q, :max(ncand[q], 0)].tolist())
        assert ncand[q] == len(rc) and cand[q, :len(rc)].tolist() == rc
        assert maxc[q] == info["max_common"] and nsc[q] == info["nscored"]
        # host form, one query
        got = db.detect_loop(c["qs"][q], c["conn"][q], min_score[q], c["neigh"])
        assert got == (rc, len(rc), info["max_common"], info["nscored"])
    assert np.array_equal(db.reloc_scores(), np.zeros(NKF, np.float32))   # no stored state
    # every sharing KeyFrame connected; minScore above every score
    assert db.detect_loop(c["qs"][0], list(range(NKF)), 0.0, c["neigh"]) == ([], 0, 0, 0)
    got = db.detect_loop(c["qs"][0], [], 2.0, c["neigh"])
    assert got[:2] == ([], 0) and got[3] > 0
    del keep_q, keep_k


# ---------------------------------------------------------------------------
# the hand-worked database (figures in ref_place.py), order and maintenance
# ---------------------------------------------------------------------------
def hand_pair(voc20):
    db = KeyFrameDatabase(voc20, 5, cap=16)
    ref = R.RefKeyFrameDatabase(R.HAND_NWORDS, 5)
    for s, b in enumerate(R.HAND_KFS):
        db.add(s, b)
        ref.add(s, b)
    ref.set_neighbours(R.HAND_NEIGH)
    return db, ref


def test_hand_database(voc20):
    db, ref = hand_pair(voc20)
    assert db.detect_reloc(R.HAND_Q, R.HAND_NEIGH) == ([0], 1, 10, 3)     # C: 8 == minCommonWords
    assert db.reloc_scores().tolist() == [0.625, 0.28125, 0.0, 0.5625, 0.0]
    db, ref = hand_pair(voc20)
    assert db.DetectRelocalizationCandidates(R.HAND_Q0, R.HAND_NEIGH) == [2]
    assert db.DetectRelocalizationCandidates(R.HAND_Q, R.HAND_NEIGH) == [2]  # C's stored 1.0
    assert db.reloc_scores().tolist() == [0.625, 0.28125, 1.0, 0.5625, 0.0]
    # loop: connected KeyFrame; a neighbour with count <= minCommonWords is ignored (A's C)
    assert db.detect_loop(R.HAND_Q, [0], 0.3, R.HAND_NEIGH) == ([2], 1, 9, 3)
    assert db.detect_loop(R.HAND_Q, [], 0.3, R.HAND_NEIGH) == ([0], 1, 10, 3)
    assert ref.DetectLoopCandidates(R.HAND_Q, [], 0.3) == [0]
    assert db.DetectLoopCandidates(R.HAND_Q, [0, 1, 2, 3], 0.0, R.HAND_NEIGH) == []
    assert db.DetectLoopCandidates(R.HAND_Q, [], 2.0, R.HAND_NEIGH) == []


def test_erase_readd_moves_the_order_and_clear(voc20):
    db, ref = hand_pair(voc20)
    none = np.full((5, 10), -1, np.int32)
    ref.set_neighbours(none)
    assert db.DetectRelocalizationCandidates(R.HAND_Q, none) == [0, 3]
    assert ref.DetectRelocalizationCandidates(R.HAND_Q) == [0, 3]
    db.erase(0)
    ref.erase(0)
    assert len(db) == 4
    assert db.DetectRelocalizationCandidates(R.HAND_Q, none) == ref.DetectRelocalizationCandidates(R.HAND_Q) == [3, 2]
    db.add(0, R.HAND_KFS[0])
    ref.add(0, R.HAND_KFS[0])
    ref.set_neighbours(none)
    assert db.DetectRelocalizationCandidates(R.HAND_Q, none) == ref.DetectRelocalizationCandidates(R.HAND_Q) == [3, 0]
    assert db.reloc_scores()[0] == np.float32(0.625)
    db.clear()
    assert len(db) == 0
    assert db.detect_reloc(R.HAND_Q, none) == ([], 0, 0, 0)


def test_add_batch_device_from_transform_outputs(voc):
    """3 frames of random descriptors: transform_batch_device's outputs go into the database
    and serve as the queries, with no host copy of the vectors."""
    import torch
    rng = np.random.default_rng(21)
    counts = np.array([300, 180, 420], np.int32)
    cap, B = 512, 3
    hd = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    t_d, t_cnt = dev(hd.reshape(-1)), dev(counts)
    out = {k: torch.zeros(B * cap, dtype=torch.int32, device="cuda")
           for k in ("bow_words", "fv_nodes", "fv_feats")}
    out["bow_weights"] = torch.zeros(B * cap, dtype=torch.float64, device="cuda")
    out["fv_off"] = torch.zeros(B * (cap + 1), dtype=torch.int32, device="cuda")
    out["nbow"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    out["nfv"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    slots = np.array([5, 2, 7], np.int32)
    t_slots = dev(slots)
    t_ng = dev(np.full((8, 10), -1, np.int32))
    t_c = torch.full((B * 8,), -7, dtype=torch.int32, device="cuda")
    t_n = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    t_sc = torch.zeros(B, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    voc.transform_batch_device(t_d.data_ptr(), t_cnt.data_ptr(), cap, B, 4, ptrs, ctx())
    db = KeyFrameDatabase(voc, 8, cap=cap)
    db.add_batch_device(t_slots.data_ptr(), ptrs, cap, None, B, ctx())
    db.detect_reloc_batch_device(ptrs, cap, None, B, t_ng.data_ptr(), t_c.data_ptr(), 8,
                                 t_n.data_ptr(), ctx=ctx())
    voc.score_batch_device(ptrs, ptrs, cap, None, None, B, t_sc.data_ptr(), ctx())
    ctx().sync()
    assert len(db) == 3
    nb = out["nbow"].cpu().numpy()
    bw = out["bow_words"].cpu().numpy().reshape(B, cap)
    bx = out["bow_weights"].cpu().numpy().reshape(B, cap)
    bows = [dict(zip(bw[f, :nb[f]].tolist(), bx[f, :nb[f]].tolist())) for f in range(B)]
    assert all(n > 100 for n in nb)
    ref = R.RefKeyFrameDatabase(1000, 8)
    for f in range(B):
        ref.add(int(slots[f]), bows[f])
    cand, ncand, stored = t_c.cpu().numpy().reshape(B, 8), t_n.cpu().numpy(), db.reloc_scores()
    self_scores = [R.l1_score(b, b) for b in bows]
    assert np.array_equal(u64(t_sc.cpu().numpy()), u64(self_scores))
    for f in range(B):
        rc = R.RefKeyFrameDatabase.DetectRelocalizationCandidates(_fresh(ref), bows[f])
        assert rc[0] == slots[f]
        assert ncand[f] == len(rc) and cand[f, :len(rc)].tolist() == rc
    # each frame scored itself last among the queries that scored it (query f is the only one
    # whose gate a full self-match can pass): the stored score is the self score as a float
    assert [stored[s] for s in slots] == [np.float32(v) for v in self_scores]


def _fresh(ref):
    """the reference database with every stored score back at 0 (a call's starting state)"""
    for k in ref.kfs:
        if k is not None:
            k.mRelocScore = np.float32(0)
    return ref


# ---------------------------------------------------------------------------
# limits and errors
# ---------------------------------------------------------------------------
def test_limits_and_errors(voc, voc20):
    lib, h = L.lib(), C.c_void_p()
    limit = KeyFrameDatabase(voc20, 4, cap=4).info()[3]
    assert limit >= 8192
    assert lib.orbg_kfdb_create(ctx().handle, voc.handle, limit + 1, 16, C.byref(h)) == L.ORBG_ENOTSUP
    assert lib.orbg_kfdb_create(ctx().handle, voc.handle, 16, 8193, C.byref(h)) == L.ORBG_ENOTSUP
    l2 = gpu_vocab(S.vocabulary(4, 2, seed=3, scoring=1))
    assert lib.orbg_kfdb_create(ctx().handle, l2.handle, 16, 16, C.byref(h)) == L.ORBG_ENOTSUP
    with pytest.raises(L.OrbgError) as e:
        l2.score({1: 1.0}, {1: 1.0})
    assert e.value.code == L.ORBG_ENOTSUP
    big = KeyFrameDatabase(voc20, limit, cap=16)                  # the limit itself is accepted
    big.add(limit - 1, R.HAND_KFS[0])
    assert big.DetectRelocalizationCandidates(R.HAND_Q) == [limit - 1] and len(big) == 1

    db = KeyFrameDatabase(voc20, 5, cap=4)
    for bad in (lambda: db.add(5, {1: 1.0}), lambda: db.add(-1, {1: 1.0}),
                lambda: db.add(0, ([3, 2], [.5, .5])), lambda: db.add(0, ([2, 2], [.5, .5])),
                lambda: db.add(0, {R.HAND_NWORDS: 1.0}), lambda: db.add(0, ([-1], [1.0])),
                lambda: db.add(0, {w: .2 for w in range(5)}), lambda: db.erase(5)):
        with pytest.raises(L.OrbgError) as e:
            bad()
        assert e.value.code == L.ORBG_EINVAL
    db.add(0, {1: 1.0})
    with pytest.raises(L.OrbgError) as e:
        db.add(0, {2: 1.0})                                       # already live
    assert e.value.code == L.ORBG_EINVAL
    db.erase(3)                                                   # not live: no effect
    assert len(db) == 1


def test_cand_cap_and_empty_queries(voc, cases):
    c = cases[0]
    q3 = next(q for q, x in enumerate(c["batch"]) if len(x[0]) == 3)
    rc = c["batch"][q3][0]
    # fresh databases: each call below starts from stored scores of 0, as the reference run
    cand, ncand, _, _ = run_reloc_batch(gpu_db(voc, c["kfs"]), c["qs"], c["neigh"], cand_cap=1,
                                        qindex=[q3, q3])
    assert ncand.tolist() == [3, 3] and cand.reshape(-1).tolist() == [rc[0], rc[0]]
    got = gpu_db(voc, c["kfs"]).detect_reloc(c["qs"][q3], c["neigh"], cand_cap=1)
    assert got[:2] == ([rc[0]], 3)
    # nq == 0: nothing is written; an empty query vector: zero candidates
    db = gpu_db(voc, c["kfs"])
    cand, ncand, maxc, nsc = run_reloc_batch(db, c["qs"], c["neigh"], qindex=[])
    assert ncand.tolist() == [-7]
    cand, ncand, maxc, nsc = run_reloc_batch(db, [{}, c["qs"][q3]], c["neigh"])
    assert ncand.tolist() == [0, 3] and maxc[0] == 0 and nsc[0] == 0
    assert db.detect_reloc({}, c["neigh"]) == ([], 0, 0, 0)
    assert db.detect_loop({}, [], 0.0, c["neigh"]) == ([], 0, 0, 0)
