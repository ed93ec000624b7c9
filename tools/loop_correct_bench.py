#!/usr/bin/env python3
"""The Map's CorrectLoop stages, timed at DESIGN.md's map size beside tools/map_edit_bench.py: K
keyframes of N features on a trajectory (keyframe s observes the landmarks [step * s,
step * s + N), step = N / 40: about 40 observations per landmark, about 78 connected keyframes
per keyframe), cameras on a line looking along +z, every keyframe with a pose.

Every call edits the map, so each figure is the median of single runs with `cur` on slots far
apart: the wall time of the device form from a drained stream to a drained stream, the profiler
off (the launches are part of the cost: LoopConnections issues four launches per entry of
set_cap, not per member it finds).

  propagate          orbg_map_propagate_device: UpdateConnections(cur), the set, the Sim3 tables,
                     the map-point loop, SetPose and UpdateConnections per member
  loop_connections   orbg_map_loop_connections_device over that set
  essential_graph    orbg_map_essential_graph_device: vertices, Scw / Snc, the edge list
  apply              orbg_map_apply_correction_device with Siw = Scw (every point is moved
                     through the two maps and lands where it was) and UpdateNormalAndDepth of
                     all points

Prints one JSON line and appends it to --out.

    python tools/loop_correct_bench.py [--keyframes 2000] [--features 1000] [--set-cap 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--set-cap", type=int, default=128)
    ap.add_argument("--slots", type=int, nargs="*", default=[300, 700, 1100, 1500, 1850])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_correct_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    K, N, cap = args.keyframes, args.features, args.set_cap
    Kmax = 1 << (K - 1).bit_length()
    step = max(N // 40, 1)
    P = step * (K - 1) + N
    ctx = _ctx(0)
    m = Map(Kmax, N, P)
    rng = np.random.default_rng(11)

    def cuda(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to("cuda")

    span = 12.0 / 40.0
    land = np.stack([span * (np.arange(P) / step) - 6.0, rng.uniform(-4, 4, P),
                     rng.uniform(8, 12, P)], 1)
    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    rec["x"], rec["y"], rec["z"] = land[:, 0], land[:, 1], land[:, 2]
    rec["flags"] = L.MP_VALID
    rows = (np.arange(K)[:, None] * step + np.arange(N)[None]).astype(np.int32)
    ref = np.minimum(np.arange(P) // step, K - 1).astype(np.int32)
    centres = np.stack([span * np.arange(K), np.zeros(K), np.zeros(K)], 1).astype(np.float32)
    T = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32), (K, 1, 1))
    T[:, :, 3] = -centres
    slots = np.arange(K, dtype=np.int32)
    counts = np.full(K, N, np.int32)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    d = [cuda(a) for a in (slots, rows, rng.integers(0, 6, (K, N)).astype(np.uint8), counts,
                           centres, flags, rec, rng.integers(0, 256, (P, 32), dtype=np.uint8), ref,
                           T.reshape(K, 12))]
    torch.cuda.synchronize()
    m.set_points_device(None, 0, P, d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr())
    m.set_keyframes_device(d[0].data_ptr(), K, d[1].data_ptr(), d[2].data_ptr(), N,
                           d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr())
    m.set_poses_device(d[0].data_ptr(), K, d[9].data_ptr(), None)
    for lo in range(0, K, 256):
        m.update_connections_batch_device(d[0][lo:].data_ptr(), min(256, K - lo))
    m.update_normal_and_depth_batch_device(None, P)
    ctx.sync()

    i32 = dict(dtype=torch.int32, device="cuda")
    t_set, t_n, t_st = torch.zeros(cap, **i32), torch.zeros(4, **i32), torch.zeros(8, **i32)
    t_co = torch.zeros(Kmax * 64, dtype=torch.uint8, device="cuda")
    t_nc = torch.zeros(Kmax * 64, dtype=torch.uint8, device="cuda")
    pcap, ecap = cap * 256, 64 * K
    t_pr, t_vs = torch.zeros(2 * pcap, **i32), torch.zeros(Kmax, **i32)
    t_sc = torch.zeros(2 * Kmax * 64, dtype=torch.uint8, device="cuda")
    t_ed = torch.zeros(3 * ecap, **i32)
    t_T = torch.zeros(Kmax * 12, dtype=torch.float32, device="cuda")
    times = {k: [] for k in ("propagate", "loop_connections", "essential_graph", "apply")}
    sizes = []

    def timed(name, fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        times[name].append((time.perf_counter() - t0) * 1e3)

    for cur in args.slots:
        S = np.zeros(1, L.SIM3D_DTYPE)
        S["q"][0], S["t"][0], S["s"][0] = (0, 0, 0, 1), -1.01 * centres[cur].astype(np.float64), 1.01
        t_S = cuda(S)
        loop = cur - 200
        torch.cuda.synchronize()
        timed("propagate", lambda: m.propagate_device(cur, t_S.data_ptr(), t_set.data_ptr(), cap,
                                                      t_n.data_ptr(), t_co.data_ptr(),
                                                      t_nc.data_ptr(), t_st.data_ptr()))
        timed("loop_connections", lambda: m.loop_connections_device(
            t_set.data_ptr(), cap, t_n.data_ptr(), t_pr.data_ptr(), pcap, t_n[1:].data_ptr()))
        timed("essential_graph", lambda: m.essential_graph_device(
            cur, loop, t_co.data_ptr(), t_nc.data_ptr(), t_set.data_ptr(), cap, t_n.data_ptr(),
            t_pr.data_ptr(), pcap, t_n[1:].data_ptr(), t_vs.data_ptr(), t_n[2:].data_ptr(),
            t_n[3:].data_ptr(), t_sc.data_ptr(), t_sc[Kmax * 64:].data_ptr(), t_ed.data_ptr(), ecap,
            t_st[4:].data_ptr(), t_st[5:].data_ptr()))
        assert t_st[0].item() == 0 and t_st[5].item() == 0, t_st.tolist()
        nv = t_n[2].item()
        Tcw = m.poses()[0]
        t_T[:nv * 12] = torch.from_numpy(Tcw[t_vs[:nv].cpu().numpy()].reshape(-1)).cuda()
        torch.cuda.synchronize()
        timed("apply", lambda: m.apply_correction_device(cur, t_vs.data_ptr(), t_n[2:].data_ptr(),
                                                         t_sc.data_ptr(), t_sc.data_ptr(),
                                                         t_T.data_ptr()))
        sizes.append((t_n[0].item(), t_n[1].item(), nv, t_st[4].item()))

    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    out = {"metric": "CorrectLoop stages on the Map, K=%d keyframes" % K,
           "value": round(sum(med.values()), 3), "unit": "ms", "higher_is_better": False,
           "data": "synthetic",
           "config": {"keyframes": K, "max_keyframes": Kmax, "features": N, "points": P,
                      "set_cap": cap, "cur_slots": args.slots,
                      "set_members": [s[0] for s in sizes], "pairs": [s[1] for s in sizes],
                      "vertices": sizes[0][2], "edges": [s[3] for s in sizes]},
           "stages_ms": med, "runs_ms": {k: [round(x, 3) for x in v] for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
