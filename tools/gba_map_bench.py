#!/usr/bin/env python3
"""Global BA's stages on the Map, timed on tools/gba_bench.py's 1500-keyframe trajectory put into
a Map (keyframe s = pose s, its features the edges of pose s, parent s - 1): about 30 000 points
and 210 000 edges.

Every figure is a wall time from a drained stream to a drained stream with the profiler off, the
median over --runs repeats after one warm-up:

  window   orbg_map_gba_window_device (four launches behind a current observation index)
  upload   the host-to-device copy of the poses, points and edge records of the same window from
           pageable host arrays: what orbg_global_ba_optimize's caller pays today and the window
           replaces (building those arrays on the host is not counted)
  store    orbg_map_gba_store_device with loop_kf != 0 (mTcwGBA / mPosGBA and the marks)
  store0   the same with loop_kf == 0 (SetPose, SetWorldPos, UpdateNormalAndDepth)
  update   orbg_map_gba_update_device: the last --tail keyframes and their points are outside the
           BA (their marks are cleared before every repeat), so the propagation runs a chain of
           that length

Beside the times, the bytes each stage writes and the larger arrays it reads.  Prints one JSON
line and appends it to --out.

    python tools/gba_map_bench.py [--keyframes 1500] [--tail 30] [--runs 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=1500)
    ap.add_argument("--tail", type=int, default=30)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_map_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import gba_bench
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    ctx = _ctx(0)
    poses, points, edges = gba_bench.trajectory(args.keyframes)
    K, P, LOOP = len(poses), len(points), 7
    Kmax = 1 << (K - 1).bit_length()
    order = np.lexsort((edges["point"], edges["pose"]))          # by keyframe, then point
    e = edges[order]
    per = np.bincount(e["pose"], minlength=K)
    N = int(per.max())
    idx = np.arange(len(e)) - np.repeat(np.cumsum(per) - per, per)
    rows = np.full((K, N), -1, np.int32)
    rows[e["pose"], idx] = e["point"]
    isg = np.array([1.0 / float(np.float32(np.float32(1.2) ** (2 * l))) for l in range(8)])
    octs = np.zeros((K, N), np.uint8)
    octs[e["pose"], idx] = np.argmin(np.abs(isg[None] - e["inv_sigma2"][:, None]), 1)
    kps = np.zeros((Kmax, N), L.KP_DTYPE)
    ur = np.full((Kmax, N), -1.0, np.float32)
    kps["x"][e["pose"], idx], kps["y"][e["pose"], idx] = e["obs"][:, 0], e["obs"][:, 1]
    kps["octave"][:K] = octs
    ur[e["pose"], idx] = np.where(e["stereo"] != 0, e["obs"][:, 2], -1.0)
    cams = np.zeros(Kmax, L.FRUSTUM_DTYPE)
    cams["fx"], cams["fy"], cams["cx"], cams["cy"], cams["bf"] = gba_bench.CAM
    q = poses["q"]
    x, y, z, w = q.T
    Rm = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                   np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                   np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    T = np.concatenate([Rm, poses["t"][:, :, None]], 2).astype(np.float32)
    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["flags"] = L.MP_VALID
    first = np.full(P, K, np.int64)
    np.minimum.at(first, e["point"], e["pose"])
    ref = first.astype(np.int32)

    def cuda(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.fields else a).to("cuda")

    slots, counts = np.arange(K, dtype=np.int32), per.astype(np.int32)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    acounts = np.zeros(Kmax, np.int32)
    acounts[:K] = per
    centres = -np.einsum("nji,nj->ni", T[:, :, :3].astype(np.float64), T[:, :, 3].astype(np.float64))
    d = dict(slots=cuda(slots), rows=cuda(rows), octs=cuda(octs), counts=cuda(counts),
             centres=cuda(centres.astype(np.float32)), flags=cuda(flags), rec=cuda(rec),
             desc=torch.zeros(P * 32, dtype=torch.uint8, device="cuda"), ref=cuda(ref),
             T=cuda(T.reshape(K, 12)), kdesc=torch.zeros(Kmax * N * 32, dtype=torch.uint8, device="cuda"),
             kps=cuda(kps), ur=cuda(ur), acounts=cuda(acounts), cams=cuda(cams),
             origin=cuda(np.zeros(1, np.int32)))
    torch.cuda.synchronize()
    m = Map(Kmax, N, P)
    m.set_points_device(None, 0, P, d["rec"].data_ptr(), d["desc"].data_ptr(), d["ref"].data_ptr())
    m.set_keyframes_device(d["slots"].data_ptr(), K, d["rows"].data_ptr(), d["octs"].data_ptr(), N,
                           d["counts"].data_ptr(), d["centres"].data_ptr(), d["flags"].data_ptr())
    m.set_poses_device(d["slots"].data_ptr(), K, d["T"].data_ptr(), None)
    m.AttachKeyFrames(d["kdesc"].data_ptr(), d["kps"].data_ptr(), d["ur"].data_ptr(),
                      d["acounts"].data_ptr(), N, d["cams"].data_ptr())
    for s in range(1, K):
        m.ChangeParent(s, s - 1)
    m.rebuild()
    ctx.sync()

    pc, qc, ec = Kmax, P, len(e)
    u8 = dict(dtype=torch.uint8, device="cuda")
    t_ks, t_po = torch.zeros(pc * 4, **u8), torch.zeros(pc * L.POSE_DTYPE.itemsize, **u8)
    t_id, t_pt = torch.zeros(qc * 4, **u8), torch.zeros(qc * 24, **u8)
    t_ed, t_ef = torch.zeros(ec * L.EDGE_DTYPE.itemsize, **u8), torch.zeros(ec * 4, **u8)
    t_h = torch.zeros(96, **u8)
    h = t_h.data_ptr()
    times = {k: [] for k in ("window", "upload", "store", "store0", "update")}

    def timed(name, fn, keep):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        if keep:
            times[name].append((time.perf_counter() - t0) * 1e3)

    def window():
        m.gba_window_device(0, t_ks.data_ptr(), t_po.data_ptr(), pc, t_id.data_ptr(), t_pt.data_ptr(),
                            qc, t_ed.data_ptr(), t_ef.data_ptr(), ec, h, h + 16)

    def store(loop_kf):
        m.gba_store_device(t_ks.data_ptr(), pc, t_id.data_ptr(), qc, h, t_po.data_ptr(),
                           t_pt.data_ptr(), loop_kf, d["cams"].data_ptr(), h + 32)

    window()
    ctx.sync()
    cnt = np.frombuffer(t_h.cpu().numpy().tobytes(), np.int32)[:8].tolist()
    assert cnt[:3] == [K, P, len(e)] and cnt[4] == 0, cnt
    hp = np.frombuffer(t_po.cpu().numpy().tobytes(), L.POSE_DTYPE)[:K].copy()
    hx = np.frombuffer(t_pt.cpu().numpy().tobytes(), np.float64)[:3 * P].copy()
    he = np.frombuffer(t_ed.cpu().numpy().tobytes(), L.EDGE_DTYPE)[:len(e)].copy()
    up = [(torch.from_numpy(hp.view(np.uint8)), t_po[:hp.nbytes]), (torch.from_numpy(hx.view(np.uint8)), t_pt[:hx.nbytes]),
          (torch.from_numpy(he.view(np.uint8)), torch.zeros(he.nbytes, **u8))]
    tail = np.arange(K - args.tail, K)
    tail_pts = np.flatnonzero(ref >= K - args.tail)
    zeros_kf = np.zeros(len(tail), np.int32)
    out6 = None
    for run in range(args.runs + 1):
        keep = run > 0
        timed("window", window, keep)
        timed("upload", lambda: [dst.copy_(src) for src, dst in up], keep)
        timed("store", lambda: store(LOOP), keep)
        # the tail is outside the BA: its marks go back to 0 (contiguous ranges)
        m.SetGbaState(int(tail[0]), kf_ba_global=zeros_kf)
        if len(tail_pts):
            lo, hi = int(tail_pts.min()), int(tail_pts.max()) + 1
            mk = np.full(hi - lo, LOOP, np.int32)
            mk[tail_pts - lo] = 0
            m.SetGbaState(first_point=lo, mp_ba_global=mk)
        timed("update", lambda: m.gba_update_device(d["origin"].data_ptr(), 1, LOOP, d["cams"].data_ptr(),
                                                    h + 48, h + 80), keep)
        o = np.frombuffer(t_h.cpu().numpy().tobytes(), np.int32)
        assert o[20] == 0 and o[12:14].tolist() == [K, args.tail], o[12:24].tolist()
        out6 = o[12:18].tolist()
        m.set_poses_device(d["slots"].data_ptr(), K, d["T"].data_ptr(), None)     # the poses as before
        m.set_points_device(None, 0, P, d["rec"].data_ptr(), d["desc"].data_ptr(), d["ref"].data_ptr())
        timed("store0", lambda: store(0), keep)
        m.set_poses_device(d["slots"].data_ptr(), K, d["T"].data_ptr(), None)
        m.set_points_device(None, 0, P, d["rec"].data_ptr(), d["desc"].data_ptr(), d["ref"].data_ptr())
        ctx.sync()

    ne = len(e)
    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    nbytes = {
        "window_written": K * (4 + 64) + P * (4 + 24) + ne * (112 + 4),
        "window_read": ne * 4 * 2 + ne * (28 + 4) + P * 36 + K * (48 + 12),   # index twice, keypoints, records, poses
        "upload": hp.nbytes + hx.nbytes + he.nbytes,
        "store_written": K * 52 + P * 16, "store_read": K * 68 + P * 28,
        "update_written": K * (48 * 2 + 12 + 4) + args.tail * 52 + P * 12,
        "update_read": K * (48 + 12 + 8) + P * (36 + 4 + 12 + 4)}
    out = {"metric": "GlobalBundleAdjustment on the Map, window of %d keyframes" % K, "value": med["window"],
           "unit": "ms", "higher_is_better": False, "data": "synthetic",
           "config": {"keyframes": K, "max_keyframes": Kmax, "kf_cap": N, "points": P, "edges": ne,
                      "tail": args.tail, "runs": args.runs, "update_out": out6},
           "stages_ms": med, "bytes": nbytes,
           "window_over_upload": round(med["window"] / med["upload"], 3),
           "runs_ms": {k: [round(x, 3) for x in v] for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
