#!/usr/bin/env python3
"""The covisibility Map's batched calls (KeyFrame::UpdateConnections, Tracking::UpdateLocalMap,
MapPoint::UpdateNormalAndDepth) and the observation-index rebuild, timed on a synthetic map
beside the bytes each call must move.

Workload: K keyframes of N features each on a trajectory: keyframe s observes the points
[step * s, step * s + N) (step = N / 40), so a point has about 40 observations and a keyframe
shares N - step * d points with the keyframes d slots away: 78 connected keyframes, all above
the threshold of 15.  Every keyframe is uploaded from device memory
(orbg_map_set_keyframes_device), the graph is built by one UpdateConnections batch over all
slots, and the timed calls are
  update_connections   one batch of `--update` distinct slots spread over the map (the
                       CorrectLoop / local BA pattern), after their rows lost their last ten
                       points so that every weight changes and every neighbour row is re-sorted
  local_keyframes      B frames; frame f holds half of the points of one keyframe's window
  local_points         the same B frames with the lists local_keyframes gave (about 80 each)
  normal_and_depth     every point of the map
  rebuild              the observation index and the children lists, marked stale by
                       re-uploading one row

Algorithmic bytes (what the kernels must move, no cache reuse counted):
  update_connections   per slot: the row (4 B / feature), each point's flags and two CSR
                       offsets (12 B), its observations (4 B each), the W row written (2 B /
                       slot), per connected keyframe one W entry read and written (4 B), the own
                       list (4 B / entry) and neigh (40 B); per re-sorted row: the W row read
                       (2 B / slot) and its list written (4 B / entry) and neigh (40 B)
  local_keyframes      per frame: the slot flags (4 B / slot), per frame point its id, flags
                       and two offsets (16 B) and its observations (4 B each), per initial
                       keyframe 48 B of neighbours, child and parent, the list written
  local_points         per frame and local keyframe, twice (count, gather): the list (4 B /
                       entry), the row (4 B / feature), each point's flags and offsets (12 B)
                       and observations (4 B each); per gathered point 36 + 32 B read and 72 B
                       written; the frame's own points once per local keyframe (4 B each)
  normal_and_depth     per point: the record read and written (72 B), the reference slot and
                       two offsets (12 B), per observation the entry and the centre (16 B),
                       the octave (1 B)
  rebuild              per row entry: the id read three times (12 B), two counter updates
                       (8 B), the entry written twice and read once in the placing pass plus
                       its segment read (4 B x observations); per point 4 B zeroed twice and
                       12 B of scan; per slot 12 B of tree

Prints one JSON line.

    python tools/map_bench.py [--keyframes 2000] [--features 2000] [--frames 64] [--update 32]
                              [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8e12   # MI355X HBM3E peak, as DESIGN.md section 3 prices every kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--update", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    K, N, B, U = args.keyframes, args.features, args.frames, args.update
    Kmax = 1 << (K - 1).bit_length()
    step = max(N // 40, 1)
    P = step * (K - 1) + N
    ctx = _ctx(0)
    m = Map(Kmax, N, P)
    rng = np.random.default_rng(5)
    dev = "cuda"

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # points: a band in front of a camera path along x; centres on the path
    pos = np.stack([np.arange(P) * (40.0 / P) + rng.uniform(-1, 1, P), rng.uniform(-2, 2, P),
                    rng.uniform(6, 12, P)], 1).astype(np.float32)
    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    rec["x"], rec["y"], rec["z"], rec["flags"] = pos[:, 0], pos[:, 1], pos[:, 2], L.MP_VALID
    ref = np.minimum(np.arange(P) // step, K - 1).astype(np.int32)
    t_rec = cuda(rec.view(np.uint8).reshape(-1))
    t_desc = torch.randint(0, 256, (P, 32), dtype=torch.uint8, device=dev)
    t_ref = cuda(ref)
    rows = (np.arange(K, dtype=np.int32)[:, None] * step + np.arange(N, dtype=np.int32)[None])
    t_rows = cuda(rows)
    t_oct = torch.randint(0, 8, (K, N), dtype=torch.uint8, device=dev)
    t_slots = cuda(np.arange(K, dtype=np.int32))
    t_counts = cuda(np.full(K, N, np.int32))
    centres = np.stack([np.arange(K) * (40.0 / K), np.zeros(K), np.zeros(K)], 1).astype(np.float32)
    t_cen = cuda(centres)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    t_flags = cuda(flags)
    torch.cuda.synchronize()
    m.set_points_device(None, 0, P, t_rec.data_ptr(), t_desc.data_ptr(), t_ref.data_ptr(), ctx)
    m.set_keyframes_device(t_slots.data_ptr(), K, t_rows.data_ptr(), t_oct.data_ptr(), N,
                           t_counts.data_ptr(), t_cen.data_ptr(), t_flags.data_ptr(), ctx)
    m.update_connections_batch_device(t_slots.data_ptr(), K, ctx)
    ctx.sync()

    # the timed UpdateConnections batch: U slots, rows alternating between full and ten short
    upd = np.linspace(50, K - 51, U).astype(np.int32)
    t_upd = cuda(upd)
    t_upd_counts = [cuda(np.full(U, N - 10, np.int32)), cuda(np.full(U, N, np.int32))]
    t_upd_rows = cuda(rows[upd])
    t_upd_oct = torch.randint(0, 8, (U, N), dtype=torch.uint8, device=dev)
    t_upd_cen, t_upd_flags = cuda(centres[upd]), cuda(np.zeros(U, np.int32))

    # frames: half of one keyframe's window each
    kf_of = rng.integers(60, K - 60, B)
    fcap = N
    fp = np.full((B, fcap), -1, np.int32)
    for f in range(B):
        ids = kf_of[f] * step + rng.choice(N, N // 2, replace=False)
        fp[f, :len(ids)] = ids
    t_fp0 = cuda(fp)
    t_fp = t_fp0.clone()
    t_fcnt = cuda(np.full(B, N // 2, np.int32))
    lkf_cap, lp_cap = 128, 16384
    t_lk = torch.full((B, lkf_cap), -1, dtype=torch.int32, device=dev)
    t_nl, t_rf, t_nlp = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    t_ids = torch.empty((B, lp_cap), dtype=torch.int32, device=dev)
    t_mps = torch.empty(B * lp_cap * L.MAPPOINT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    t_qd = torch.empty((B, lp_cap, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    state = {"i": 0}

    def shorten():
        c = t_upd_counts[state["i"] & 1]
        state["i"] += 1
        m.set_keyframes_device(t_upd.data_ptr(), U, t_upd_rows.data_ptr(), t_upd_oct.data_ptr(), N,
                               c.data_ptr(), t_upd_cen.data_ptr(), t_upd_flags.data_ptr(), ctx)
        m.rebuild(ctx)

    def update():
        m.update_connections_batch_device(t_upd.data_ptr(), U, ctx)

    def local_kfs():
        m.local_keyframes_batch_device(t_fp.data_ptr(), fcap, t_fcnt.data_ptr(), B, t_lk.data_ptr(),
                                       lkf_cap, t_nl.data_ptr(), t_rf.data_ptr(), ctx)

    def local_pts():
        m.local_points_batch_device(t_lk.data_ptr(), lkf_cap, t_nl.data_ptr(), t_fp.data_ptr(),
                                    fcap, t_fcnt.data_ptr(), B, t_ids.data_ptr(), t_mps.data_ptr(),
                                    t_qd.data_ptr(), lp_cap, t_nlp.data_ptr(), ctx)

    def normals():
        m.update_normal_and_depth_batch_device(None, P, ctx)

    def step_all():
        shorten()
        update()
        local_kfs()
        local_pts()
        normals()

    for _ in range(args.warmup):
        step_all()
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(args.steps):
        step_all()
    ctx.sync()
    kern = ctx.profile_read()
    ctx.profile(False)
    ms = {k[4:]: v[0] / v[1] for k, v in kern.items() if k.startswith("map_")}

    nl = t_nl.cpu().numpy().astype(np.int64)
    nlp = t_nlp.cpu().numpy().astype(np.int64)
    assert (nl > 0).all() and (nl <= lkf_cap).all() and (nlp <= lp_cap).all()
    nobs = np.zeros(P, np.int64)
    for s in range(K):
        nobs[s * step:s * step + N] += 1
    conn = np.array([len(m.GetConnectedKeyFrames(int(s))) for s in upd])
    nord = np.array([len(m.connections(int(s))[0]) for s in upd])
    row_obs = np.array([nobs[s * step:s * step + N].sum() for s in upd])
    b_update = int((N * (4 + 12) + row_obs * 4 + Kmax * 2 + conn * 4 + nord * 4 + 40).sum()
                   + (conn * (Kmax * 2 + 40) + conn * nord * 4).sum())
    f_obs = np.array([nobs[fp[f, :N // 2]].sum() for f in range(B)])
    b_lkf = int((Kmax * 4 + (N // 2) * 16 + f_obs * 4 + np.minimum(nl, 81) * 48 + nl * 4).sum())
    mean_row_obs = float(nobs.mean()) * N
    b_lp = int((nl * 2 * (nl * 4 + N * 16 + mean_row_obs * 4) + nlp * (36 + 32 + 72)
                + nl * (N // 2) * 4).sum())
    b_nd = int(P * (72 + 12 + 1) + nobs.sum() * 16)
    entries = int(K * N)
    b_rebuild = int(entries * (12 + 8 + 12) + (nobs * nobs).sum() * 4 + P * 20 + Kmax * 12)

    def row(name, nbytes):
        t = ms[name]
        frac = nbytes / (t * 1e-3) / HBM_BPS
        return {"ms": round(t, 4), "bytes": int(nbytes), "gbs": round(nbytes / (t * 1e-3) / 1e9, 1),
                "hbm_frac": round(frac, 4), "bound": "bytes" if frac > 0.3 else "latency"}

    res = {
        "metric": "local map frames/s (UpdateLocalKeyFrames + UpdateLocalPoints), K=%d keyframes" % K,
        "value": round(B / ((ms["local_keyframes"] + ms["local_points"]) * 1e-3), 1),
        "unit": "frames/s", "higher_is_better": True, "dtype": "i32/u16/f32", "data": "synthetic",
        "config": {"keyframes": K, "max_keyframes": Kmax, "features": N, "points": int(P),
                   "observations_per_point": round(float(nobs.mean()), 1), "frames": B,
                   "frame_points": N // 2, "update_slots": U,
                   "connected_per_keyframe": round(float(conn.mean()), 1),
                   "local_keyframes_per_frame": round(float(nl.mean()), 1),
                   "local_points_per_frame": round(float(nlp.mean()), 1)},
        "update_connections": row("update_connections", b_update),
        "local_keyframes": row("local_keyframes", b_lkf),
        "local_points": row("local_points", b_lp),
        "normal_and_depth": row("normal_depth", b_nd),
        "rebuild": row("rebuild", b_rebuild),
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
