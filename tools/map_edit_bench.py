#!/usr/bin/env python3
"""ORBmatcher::Fuse, LocalMapping::SearchInNeighbors and MapPoint::Replace on the device Map,
timed at DESIGN.md's map size beside tools/culling_bench.py: K keyframes of N features on a
trajectory (keyframe s observes the landmarks [step * s, step * s + N), step = N / 40: about 40
observations per landmark).  Cameras stand on a line and look along +z; a feature lies where its
keyframe sees its landmark, with the landmark's octave and its descriptor a few bits apart.
Every fourth landmark owns a second map point id in the later half of its keyframes (the
duplicates Fuse merges), and a quarter of the features hold no point (AddObservation).

Every call edits the map, so each figure is the median of single runs on slots far apart: the
wall time from a drained stream to a drained stream, the profiler off (the launches of a call
are part of its cost: SearchInNeighbors issues its launches for the bounds, not for the list it
finds).

  fuse                 one orbg_map_fuse_device call: slot t with the row of slot t + 3
  search_in_neighbors  one call, monocular
  replace              orbg_map_replace_device of `--pairs` (first id -> second id) pairs
  host_path            what one Fuse cost before: orbg_fuse_batch_device on the same inputs, the
                       download of best_idx / best_dist, and orbg_map_set_keyframe for as many
                       rows as the device Fuse changed (the host replay itself is not counted)

Prints one JSON line.

    python tools/map_edit_bench.py [--keyframes 2000] [--features 2000] [--pairs 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FX, CX, CY, BF, W_IMG, H_IMG = 500.0, 320.0, 240.0, 40.0, 640.0, 480.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--slots", type=int, nargs="*", default=[300, 700, 1100, 1500, 1850])
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    K, N = args.keyframes, args.features
    Kmax = 1 << (K - 1).bit_length()
    step = max(N // 40, 1)
    nland = step * (K - 1) + N
    P = 2 * nland
    ctx = _ctx(0)
    m = Map(Kmax, N, P)
    rng = np.random.default_rng(9)

    def cuda(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to("cuda")

    # landmarks and cameras
    span = 12.0 / 40.0
    lx = span * (np.arange(nland) / step) - 6.0
    land = np.stack([lx, rng.uniform(-4, 4, nland), rng.uniform(8, 12, nland)], 1)
    loct = rng.integers(0, 6, nland)
    base = rng.integers(0, 256, (nland, 32), dtype=np.uint8)
    cx_s = span * np.arange(K)
    centres = np.stack([cx_s, np.zeros(K), np.zeros(K)], 1).astype(np.float32)
    lidx = np.arange(K)[:, None] * step + np.arange(N)[None]                 # [K][N] landmark
    # landmark l is seen by the keyframes (l / step - 40, l / step]: the later half hold the second id
    dup = (lidx % 4 == 0) & (np.arange(K)[:, None] >= lidx // step - 19)
    rows = np.where(dup, nland + lidx, lidx)
    rows[rng.random((K, N)) < 0.25] = -1
    rows = rows.astype(np.int32)
    z = land[lidx, 2]
    kps = np.zeros((Kmax, N), L.KP_DTYPE)
    kps["x"][:K] = FX * (land[lidx, 0] - cx_s[:, None]) / z + CX + rng.normal(0, 0.25, (K, N))
    kps["y"][:K] = FX * land[lidx, 1] / z + CY + rng.normal(0, 0.25, (K, N))
    kps["octave"][:K] = loct[lidx]
    kps["size"], kps["response"] = 31, 20
    kdesc = np.zeros((Kmax, N, 32), np.uint8)
    kdesc[:K] = base[lidx] ^ (np.uint8(1) << rng.integers(0, 8, (K, N, 1)).astype(np.uint8)) * \
        (rng.random((K, N, 32), dtype=np.float32) < 0.1)     # about three bits apart
    cams = np.zeros(Kmax, L.FRUSTUM_DTYPE)
    T = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32), (K, 1, 1))
    T[:, :, 3] = -centres
    cams["Tcw"][:K] = T.reshape(K, 12)
    for k, v in (("fx", FX), ("fy", FX), ("cx", CX), ("cy", CY), ("bf", BF), ("nlevels", 8),
                 ("log_scale_factor", np.float32(np.log(np.float64(np.float32(1.2))))),
                 ("max_x", W_IMG), ("max_y", H_IMG)):
        cams[k] = v
    counts = np.zeros(Kmax, np.int32)
    counts[:K] = N
    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    for a, k in enumerate(("x", "y", "z")):
        rec[k][:nland] = rec[k][nland:] = land[:, a]
    rec["flags"] = L.MP_VALID
    pdesc = np.concatenate([base, base])
    # mpRefKF: an observer of the id (the first id in the earlier half of its keyframes)
    last_kf = np.minimum(np.arange(nland) // step, K - 1)
    ref = np.concatenate([np.maximum(last_kf - 30, 0), np.maximum(last_kf - 5, 0)]).astype(np.int32)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    t = [cuda(a) for a in (rec, ref, np.arange(K, dtype=np.int32), rows, loct[lidx].astype(np.uint8),
                           np.full(K, N, np.int32), centres, flags, pdesc)]
    att = [cuda(a) for a in (kdesc, kps, counts, cams)]
    torch.cuda.synchronize()
    m.set_points_device(None, 0, P, t[0].data_ptr(), t[8].data_ptr(), t[1].data_ptr(), ctx)
    m.set_keyframes_device(t[2].data_ptr(), K, t[3].data_ptr(), t[4].data_ptr(), N,
                           t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), ctx)
    m.AttachKeyFrames(att[0].data_ptr(), att[1].data_ptr(), None, att[2].data_ptr(), N,
                      att[3].data_ptr())
    m.update_connections_batch_device(t[2].data_ptr(), K, ctx)
    m.update_normal_and_depth_batch_device(None, P, ctx)
    ctx.sync()

    t_out = torch.zeros(3 * N + 8, dtype=torch.int32, device="cuda")
    t_tg = torch.zeros(128, dtype=torch.int32, device="cuda")
    t_nf = torch.zeros(128, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def changed_rows(slot, before):
        return sum(not np.array_equal(before[s], m.keyframe_points(s)) for s in before)

    # warm-up on a slot of its own (the workspace is allocated by the first call)
    m.fuse_device(60, t[3][63].data_ptr(), N, 3.0, None, None, None, t_nf.data_ptr(), ctx)
    m.search_in_neighbors_device(100, 100, True, 3.0, t_tg.data_ptr(), 120, t_nf[1:].data_ptr(),
                                 t_nf[2:].data_ptr(), ctx)
    ctx.sync()

    fuse, host, sin = [], [], []
    lib, c = L.lib(), ctx.handle
    kfs = L.KeyFrames(att[0].data_ptr(), att[1].data_ptr(), None, None, att[2].data_ptr(), None,
                      None, None, None)
    import ctypes as C
    for slot in args.slots:
        slot = min(slot, K - 110)
        src = slot + 3
        win = range(max(slot - 45, 0), min(slot + 45, K))
        before = {s: m.keyframe_points(s) for s in win}
        ids = t[3][src]
        # the path before: the search on the same points, the download, the row rewrites
        pts = rows[src].clip(0)
        t_mps, t_md = cuda(rec[pts]), cuda(pdesc[pts])
        t_kf = cuda(np.array([slot], np.int32))
        t_mc = cuda(np.array([N], np.int32))
        torch.cuda.synchronize()
        w_search = timed(lambda: L.check(lib.orbg_fuse_batch_device(
            c, C.byref(kfs), N, t_kf.data_ptr(), att[3][slot * L.FRUSTUM_DTYPE.itemsize:].data_ptr(),
            t_mps.data_ptr(), t_md.data_ptr(), t_mc.data_ptr(), N, 1, 3.0, t_out.data_ptr(),
            t_out[N:].data_ptr(), t_out[2 * N:].data_ptr()), "orbg_fuse_batch_device"))
        t0 = time.perf_counter()
        t_out[:2 * N].cpu()
        w_down = (time.perf_counter() - t0) * 1e3
        w = timed(lambda: m.fuse_device(slot, ids.data_ptr(), N, 3.0, None, None, None,
                                           t_nf.data_ptr(), ctx))
        nrows = changed_rows(slot, before)
        fuse.append({"slot": slot, "wall_ms": round(w, 3),
                     "nfused": int(t_nf[0].item()), "rows_changed": nrows})
        cur = {s: m.keyframe_points(s) for s in list(win)[:nrows]}
        t0 = time.perf_counter()
        for s, row in cur.items():      # the rows as they stand: the map does not change
            m.AddKeyFrame(s, row, loct[lidx[s]].astype(np.uint8), centres[s], root=(s == 0))
        w_rows = (time.perf_counter() - t0) * 1e3
        host.append({"search_ms": round(w_search, 3),
                     "download_ms": round(w_down, 3), "row_rewrites_ms": round(w_rows, 3),
                     "rows": nrows})
        s2 = slot + 100
        w = timed(lambda: m.search_in_neighbors_device(
            s2, s2, True, 3.0, t_tg.data_ptr(), 120, t_nf[1:].data_ptr(), t_nf[2:].data_ptr(), ctx))
        nt = int(t_nf[1].item())
        sin.append({"slot": s2, "wall_ms": round(w, 3), "targets": nt,
                    "nfused_first": int(t_nf[2:2 + nt].sum().item()),
                    "nfused_second": int(t_nf[2 + nt].item())})

    # Replace: first id -> second id of landmarks far from the slots above, both still good
    good = (m.points()["flags"] & L.MP_VALID) != 0
    cand = np.arange(0, nland, 4)
    cand = cand[good[cand] & good[nland + cand]]
    cand = cand[((cand // step) % 400 >= 120) & ((cand // step) % 400 < 200)][:args.pairs]
    t_old, t_new = cuda(cand.astype(np.int32)), cuda((nland + cand).astype(np.int32))
    t_st = torch.zeros(len(cand), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    w = timed(lambda: m.replace_device(t_old.data_ptr(), t_new.data_ptr(), len(cand),
                                          t_st.data_ptr(), ctx))
    rep = {"pairs": len(cand), "wall_ms": round(w, 3),
           "replaced": int((t_st == 0).sum().item())}

    def med(rs, key):
        return round(float(np.median([r[key] for r in rs])), 3) if rs else None

    res = {
        "metric": "SearchInNeighbors on the device Map, K=%d keyframes x %d features (median wall "
                  "ms of %d single runs)" % (K, N, len(sin)),
        "value": med(sin, "wall_ms"), "unit": "ms", "higher_is_better": False,
        "dtype": "i32/u8/f32", "data": "synthetic",
        "config": {"keyframes": K, "max_keyframes": Kmax, "features": N, "points": int(P)},
        "fuse": {"wall_ms": med(fuse, "wall_ms"), "runs": fuse},
        "search_in_neighbors": {"wall_ms": med(sin, "wall_ms"), "runs": sin},
        "replace": rep,
        "host_path_per_fuse": {"search_ms": med(host, "search_ms"),
                               "download_ms": med(host, "download_ms"),
                               "row_rewrites_ms": med(host, "row_rewrites_ms"), "runs": host},
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
