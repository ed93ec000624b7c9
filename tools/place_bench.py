#!/usr/bin/env python3
"""Place recognition (KeyFrameDatabase::DetectRelocalizationCandidates) and the inverted-file
rebuild, timed at K keyframes beside the bytes each kernel must move.

Workload: B synthetic 1241x376 frames of one panning sequence extracted on the GPU (2000
features, 8 levels) and transformed with an ORBvoc.txt-shaped vocabulary
(synthetic.vocabulary(10, 6): k = 10, L = 6, 10^6 words, TF_IDF + L1).  The K keyframes are
those B BowVectors added K / B times each in turn (a place visited K / B times: every copy of
a query's own frame passes the 0.8 maxCommonWords gate and is scored), straight from the
transform's device outputs (orbg_kfdb_add_batch_device); each slot's 10 neighbours are the
slots added just before and after it.  One step = nq relocalization queries (the B vectors in
turn) in one orbg_kfdb_detect_reloc_batch_device call.  The rebuild is timed by erasing and
re-adding one slot, which marks the inverted file stale.

Algorithmic bytes (what the kernels must move, no cache reuse counted):
  query    per query: its vector (12 B / word), two CSR offsets per word (8 B), its words'
           postings (2 B each), per scored keyframe that keyframe's vector (12 B / word) and
           neighbour row (40 B), 16 B of counters out
  rebuild  per live entry: the word id read twice (histogram, fill), two 4 B counter
           updates and the 2 B posting; per vocabulary word: 4 B zeroed, 4 B read and 8 B
           written by the scan; per slot 16 B (live flag, sequence number, rank)

Prints one JSON line per K.

    python tools/place_bench.py [--keyframes 2048,8192] [--queries 1024] [--batch 256]
                                [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1241, 376
HBM_BPS = 8e12   # MI355X HBM3E peak, as DESIGN.md section 3 prices every kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="2048,8192")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import KeyFrameDatabase, ORBextractor, ORBVocabulary, synthetic as S

    B, nq = args.batch, args.queries
    seq = S.sequence(B, H, W, seed=S.DEFAULT_SEED + 41)
    ext = ORBextractor(2000, 1.2, 8, 20, 7, max_batch=B)
    ctx = ext.ctx
    d_img = torch.from_numpy(seq).cuda()
    ext.extract_batch_device(d_img.data_ptr(), B, W, H)
    d_kps, d_desc, d_cnt, fc = ext.batch_outputs()
    ctx.sync()
    voc = S.vocabulary(10, 6, seed=S.DEFAULT_SEED + 2)
    gv = ORBVocabulary.from_tree(voc["k"], voc["L"], voc["scoring"], voc["weighting"],
                                 voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    dev = "cuda"
    out = {k: torch.empty(B * fc, dtype=torch.int32, device=dev)
           for k in ("bow_words", "fv_nodes", "fv_feats")}
    out["bow_weights"] = torch.empty(B * fc, dtype=torch.float64, device=dev)
    out["fv_off"] = torch.empty(B * (fc + 1), dtype=torch.int32, device=dev)
    out["nbow"] = torch.empty(B, dtype=torch.int32, device=dev)
    out["nfv"] = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    torch.cuda.synchronize()
    gv.transform_batch_device(d_desc, d_cnt, fc, B, 4, ptrs, ctx)
    ctx.sync()
    nb = out["nbow"].cpu().numpy().astype(np.int64)
    words = out["bow_words"].cpu().numpy().reshape(B, fc)

    for K in [int(x) for x in args.keyframes.split(",")]:
        db = KeyFrameDatabase(gv, K, cap=fc)
        slots = np.arange(K, dtype=np.int32)
        index = (slots % B).astype(np.int32)
        neigh = np.stack([(slots + d) % K for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)], 1)
        qindex = (np.arange(nq) % B).astype(np.int32)
        t_slots, t_index = torch.from_numpy(slots).cuda(), torch.from_numpy(index).cuda()
        t_neigh = torch.from_numpy(np.ascontiguousarray(neigh, np.int32)).cuda()
        t_qi = torch.from_numpy(qindex).cuda()
        cand_cap = 32
        t_c = torch.empty(nq * cand_cap, dtype=torch.int32, device=dev)
        t_n, t_m, t_s = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(3))
        torch.cuda.synchronize()
        db.add_batch_device(t_slots.data_ptr(), ptrs, fc, t_index.data_ptr(), K, ctx)
        db.rebuild(ctx)

        def query():
            db.detect_reloc_batch_device(ptrs, fc, t_qi.data_ptr(), nq, t_neigh.data_ptr(),
                                         t_c.data_ptr(), cand_cap, t_n.data_ptr(), t_m.data_ptr(),
                                         t_s.data_ptr(), ctx)

        def rebuild():
            db.erase(K - 1)
            db.add_batch_device(t_slots[K - 1:].data_ptr(), ptrs, fc, t_index[K - 1:].data_ptr(),
                                1, ctx)
            db.rebuild(ctx)

        for _ in range(args.warmup):
            query()
            rebuild()
        ctx.sync()
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            query()
        ctx.sync()
        q_wall = (time.perf_counter() - t0) / args.steps
        for _ in range(args.steps):
            rebuild()
        ctx.sync()
        kern = ctx.profile_read()
        ctx.profile(False)
        q_ms = kern["place_reloc"][0] / kern["place_reloc"][1]
        parts = {k: kern[k][0] / kern[k][1]
                 for k in ("place_hist", "place_scan", "place_fill", "place_rank")}
        r_ms = sum(parts.values())

        nscored = t_s.cpu().numpy().astype(np.int64)
        ncand = t_n.cpu().numpy()
        hist = np.zeros(10 ** 6, np.int64)
        for f in range(B):
            hist[words[f, :nb[f]]] += K // B + (1 if f < K % B else 0)
        post = np.array([hist[words[f, :nb[f]]].sum() for f in range(B)])
        mean_kf_words = float(nb.mean())
        q_bytes = 0
        for i in range(nq):
            f = qindex[i]
            q_bytes += nb[f] * (12 + 8) + 2 * post[f] + nscored[i] * (12 * mean_kf_words + 40) + 16
        entries = int(nb[index].sum())
        r_bytes = entries * (4 + 4 + 4 + 4 + 2) + 10 ** 6 * 16 + K * 16
        res = {
            "metric": "relocalization queries/s (DetectRelocalizationCandidates), K=%d keyframes" % K,
            "value": round(nq / (q_ms * 1e-3), 1), "unit": "queries/s", "higher_is_better": True,
            "dtype": "i32/f64", "data": "synthetic",
            "config": {"keyframes": K, "queries": nq, "frames": B, "cap": int(fc),
                       "words_per_vector": round(mean_kf_words, 1),
                       "scored_per_query": round(float(nscored.mean()), 1),
                       "candidates_per_query": round(float(ncand.mean()), 2),
                       "postings_per_query": round(float(post[qindex].mean()), 1)},
            "query": {"ms": round(q_ms, 4), "wall_ms": round(q_wall * 1e3, 4),
                      "bytes": int(q_bytes), "gbs": round(q_bytes / (q_ms * 1e-3) / 1e9, 1),
                      "hbm_frac": round(q_bytes / (q_ms * 1e-3) / HBM_BPS, 4)},
            "rebuild": {"ms": round(r_ms, 4),
                        "kernels_ms": {k[6:]: round(v, 4) for k, v in parts.items()},
                        "entries": entries, "bytes": int(r_bytes),
                        "gbs": round(r_bytes / (r_ms * 1e-3) / 1e9, 1),
                        "hbm_frac": round(r_bytes / (r_ms * 1e-3) / HBM_BPS, 4)},
        }
        print(json.dumps(res), flush=True)
        del db


if __name__ == "__main__":
    main()
