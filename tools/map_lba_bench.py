#!/usr/bin/env python3
"""LocalBundleAdjustment on the Map, timed on a KITTI-like window beside tools/ba_bench.py: K
keyframes of N features on a line looking along +z (keyframe s observes the landmarks [step * s,
step * s + N), step = N / 31), the current keyframe last: about 32 local keyframes, the few
keyframes before them as fixed cameras, every landmark a local point, about 17 observations per
point.  Keypoints are the projections with half a pixel of noise, one in a hundred moved by tens
of pixels; the stored poses and positions are slightly off.

Every figure is a wall time from a drained stream to a drained stream with the profiler off, the
median over --runs fresh maps (the call edits the map), after one warm-up map:

  window     orbg_map_lba_window_device (seven launches behind a current observation index)
  apply      orbg_map_lba_apply_device with the optimiser's flags and estimates: the erasures,
             the poses and points, the index rebuild and UpdateNormalAndDepth
  optimize   orbg_local_ba_optimize alone on the same window from host arrays
  call       orbg_map_local_ba: window, download of the edge records, the same optimisation on
             the device arrays, upload of the flags, apply

The LM is shared, so call - optimize is what the Map's own stages and copies cost.

Prints one JSON line and appends it to --out.

    python tools/map_lba_bench.py [--keyframes 36] [--features 2000] [--runs 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448     # synthetic.KITTI_*


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=36)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_lba_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    K, N = args.keyframes, args.features
    Kmax = 1 << (K - 1).bit_length()
    step = max(N // 31, 1)
    P = step * (K - 1) + N
    cur = K - 1
    ctx = _ctx(0)
    rng = np.random.default_rng(17)

    def cuda(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.fields else a).to("cuda")

    span = 0.3
    land = np.stack([span * (np.arange(P) / step), rng.uniform(-2, 2, P), rng.uniform(8, 14, P)], 1)
    centres = np.stack([span * (np.arange(K) + 15.6), np.zeros(K), np.zeros(K)], 1)
    rows = (np.arange(K)[:, None] * step + np.arange(N)[None]).astype(np.int32)
    octs = rng.integers(0, 6, (K, N)).astype(np.uint8)
    kps = np.zeros((Kmax, N), L.KP_DTYPE)
    ur = np.full((Kmax, N), -1.0, np.float32)
    feat = np.zeros((K, N), np.uint8)
    for s in range(K):
        X = land[rows[s]] - centres[s]
        u = FX * X[:, 0] / X[:, 2] + CX + rng.normal(0, 0.5, N)
        v = FY * X[:, 1] / X[:, 2] + CY + rng.normal(0, 0.5, N)
        out = rng.random(N) < 0.01
        u = u + out * rng.choice([-1.0, 1.0], N) * rng.uniform(30, 60, N)
        kps["x"][s], kps["y"][s], kps["octave"][s] = u, v, octs[s]
        st = rng.random(N) < 0.5
        ur[s] = np.where(st, u - BF / X[:, 2], -1.0)
        feat[s] = np.where(st, L.MAP_FEAT_STEREO, 0)
    cams = np.zeros(Kmax, L.FRUSTUM_DTYPE)
    cams["fx"], cams["fy"], cams["cx"], cams["cy"], cams["bf"] = FX, FY, CX, CY, BF
    T = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (K, 1, 1))
    T[:, :, 3] = -(centres + rng.normal(0, 5e-3, (K, 3)))
    T = T.astype(np.float32)
    cams["Tcw"][:K] = T.reshape(K, 12)
    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    pos = land + rng.normal(0, 2e-2, (P, 3))
    rec["x"], rec["y"], rec["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    rec["flags"] = L.MP_VALID
    ref = np.minimum(np.arange(P) // step, K - 1).astype(np.int32)
    slots, counts = np.arange(K, dtype=np.int32), np.full(K, N, np.int32)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    acounts = np.zeros(Kmax, np.int32)
    acounts[:K] = N
    d = dict(slots=cuda(slots), rows=cuda(rows), octs=cuda(octs), counts=cuda(counts),
             centres=cuda(centres.astype(np.float32)), flags=cuda(flags), rec=cuda(rec),
             desc=cuda(rng.integers(0, 256, (P, 32), dtype=np.uint8)), ref=cuda(ref),
             T=cuda(T.reshape(K, 12)), kdesc=torch.zeros(Kmax * N * 32, dtype=torch.uint8, device="cuda"),
             kps=cuda(kps), ur=cuda(ur), acounts=cuda(acounts), feat=cuda(feat))
    torch.cuda.synchronize()

    def fresh_map():
        m = Map(Kmax, N, P)
        t_cams = cuda(cams)
        torch.cuda.synchronize()
        m.set_points_device(None, 0, P, d["rec"].data_ptr(), d["desc"].data_ptr(), d["ref"].data_ptr())
        m.set_keyframes_device(d["slots"].data_ptr(), K, d["rows"].data_ptr(), d["octs"].data_ptr(), N,
                               d["counts"].data_ptr(), d["centres"].data_ptr(), d["flags"].data_ptr())
        L.check(L.lib().orbg_map_set_keyframe_features_device(
            ctx.handle, m.handle, d["slots"].data_ptr(), K, d["feat"].data_ptr(), N,
            d["counts"].data_ptr()), "orbg_map_set_keyframe_features_device")
        m.set_poses_device(d["slots"].data_ptr(), K, d["T"].data_ptr(), None)
        m.AttachKeyFrames(d["kdesc"].data_ptr(), d["kps"].data_ptr(), d["ur"].data_ptr(),
                          d["acounts"].data_ptr(), N, t_cams.data_ptr())
        m.update_connections_batch_device(d["slots"].data_ptr(), K)
        m.update_normal_and_depth_batch_device(None, P)
        ctx.sync()
        return m, t_cams

    pc, qc, ec = Kmax, P, K * N
    u8 = dict(dtype=torch.uint8, device="cuda")
    t_ks, t_po = torch.zeros(pc * 4, **u8), torch.zeros(pc * L.POSE_DTYPE.itemsize, **u8)
    t_id, t_pt = torch.zeros(qc * 4, **u8), torch.zeros(qc * 24, **u8)
    t_ed, t_ef = torch.zeros(ec * L.EDGE_DTYPE.itemsize, **u8), torch.zeros(ec * 4, **u8)
    t_cn, t_st, t_er, t_o2 = (torch.zeros(16, **u8), torch.zeros(16, **u8), torch.zeros(ec, **u8),
                              torch.zeros(16, **u8))
    times = {k: [] for k in ("window", "apply", "optimize", "call")}
    sizes, reports = [], []

    def timed(name, fn, keep=True):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        if keep:
            times[name].append((time.perf_counter() - t0) * 1e3)
        return r

    def window(m):
        m.lba_window_device(cur, t_ks.data_ptr(), t_po.data_ptr(), pc, t_id.data_ptr(),
                            t_pt.data_ptr(), qc, t_ed.data_ptr(), t_ef.data_ptr(), ec,
                            t_cn.data_ptr(), t_st.data_ptr())

    def optimize(poses, points, edges):
        erase, rep = np.zeros(len(edges), np.uint8), L.LbaReport()
        L.check(L.lib().orbg_local_ba_optimize(ctx.handle, L.ptr(poses), len(poses), L.ptr(points),
                                               len(points), L.ptr(edges), len(edges), None, None,
                                               None, L.ptr(erase), C.byref(rep)),
                "orbg_local_ba_optimize")
        return poses, points, erase

    for run in range(args.runs + 1):
        keep = run > 0                                   # the first map warms every shape up
        m, t_cams = fresh_map()
        window(m)                                        # the index is current from here on
        for _ in range(3):
            timed("window", lambda: window(m), keep)
        assert np.frombuffer(t_st.cpu().numpy().tobytes(), np.int32)[0] == 0
        w = m.LbaWindow(cur, pc, qc, ec)
        copies = (np.array(w["poses"]), np.array(w["points"]), np.array(w["edges"]))
        poses, points, erase = timed("optimize", lambda: optimize(*copies), keep)
        m2, t_cams2 = fresh_map()                        # the same map for the whole call
        rep = timed("call", lambda: m2.LocalBundleAdjustment(cur, d_cams_out=t_cams2.data_ptr()), keep)
        t_po[:poses.nbytes] = cuda(poses)
        t_pt[:points.nbytes] = cuda(points.view(np.uint8).reshape(-1))
        t_er[:len(erase)] = cuda(erase)
        torch.cuda.synchronize()
        timed("apply", lambda: m.lba_apply_device(
            t_ks.data_ptr(), pc, t_id.data_ptr(), qc, t_ed.data_ptr(), t_ef.data_ptr(), ec,
            t_cn.data_ptr(), t_po.data_ptr(), t_pt.data_ptr(), t_er.data_ptr(), t_cams.data_ptr(),
            t_o2.data_ptr()), keep)
        o2 = np.frombuffer(t_o2.cpu().numpy().tobytes(), np.int32)[:2].tolist()
        assert o2 == [rep["nerased"], rep["npoints_bad"]] and int(erase.sum()) == rep["n_erase"]
        if keep:
            sizes.append((rep["nlocal"], rep["nfixed"], rep["npoints"], rep["nedges"]))
            reports.append((rep["lm"][0]["iterations"], rep["lm"][1]["iterations"], rep["n_erase"],
                            rep["nerased"], rep["npoints_bad"]))

    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    own = round(med["window"] + med["apply"], 3)
    out = {"metric": "LocalBundleAdjustment on the Map, %d local keyframes x %d features" % (sizes[0][0], N),
           "value": med["call"], "unit": "ms", "higher_is_better": False, "data": "synthetic",
           "config": {"keyframes": K, "max_keyframes": Kmax, "features": N, "points": P,
                      "nlocal": sizes[0][0], "nfixed": sizes[0][1], "npoints": sizes[0][2],
                      "nedges": sizes[0][3], "runs": args.runs,
                      "lm_iterations_erased_bad": reports[0]},
           "stages_ms": med, "window_plus_apply_ms": own,
           "window_plus_apply_over_optimize": round(own / med["optimize"], 4),
           "call_minus_optimize_ms": round(med["call"] - med["optimize"], 3),
           "runs_ms": {k: [round(x, 3) for x in v] for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
