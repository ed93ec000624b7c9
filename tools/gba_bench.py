#!/usr/bin/env python3
"""Device time of GlobalBundleAdjustment's optimisation: optimize(10), not robust
(LoopClosing::RunGlobalBundleAdjustment's call), on synthetic trajectories with loop closures
at 200, 500 and 1500 keyframes, through the sparse Schur plan (csrc/bsolve_kernels.hip) and,
as the baseline, through the dense plan on the same graph -- the path a global BA had before
the sparse plan existed.  The two run interleaved in one process (sparse, dense, sparse, ...),
each from the same initial estimates; wall time per call as median and min, HIP-event kernel
time per phase from one further profiled call each, the sparse plan's figures and the host
time of both plans.  One JSON line per size.

The dense plan factorises a (6 n)^2 matrix in one workgroup, so it is only run up to
--dense-max keyframes (default 500: at 1500 one factorisation alone is 27 times that).

    python tools/gba_bench.py [--sizes 200,500,1500] [--dense-max 500] [--steps 3] [--warmup 1]
        [--out profiles/gba_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAM = (718.856, 718.856, 607.1928, 185.2157, 386.1448)


def trajectory(n_kf, per_kf=20, band=3, n_loops=None, loop_points=10, seed=5):
    """n_kf keyframes 1.5 m apart with small rotations; per_kf points anchored at each keyframe
    and seen by the keyframes within `band` of it; n_loops (default n_kf // 50) loop closures:
    keyframe pairs half a trajectory apart sharing loop_points points.  Stereo fraction 0.6,
    0.5 px noise, float-exact observations; the start is 2 mm / 5 cm off the truth.  Built with
    array operations (tests/ref_gba.py's gba_scene, which the tests use, loops over edges)."""
    from orb_slam2_test_amd import _lib as L
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=(n_kf, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.1, n_kf)
    q = np.concatenate([ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], 1)
    x, y, z, w = q.T
    Rm = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                   np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                   np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    center = np.stack([rng.normal(0, 0.5, n_kf), rng.normal(0, 0.1, n_kf), 1.5 * np.arange(n_kf)], 1)
    t = -np.einsum("nij,nj->ni", Rm, center)
    n_loops = n_kf // 50 if n_loops is None else n_loops
    la = (np.arange(n_loops) * (n_kf // 2) // max(n_loops, 1)).astype(np.int64)
    lb = la + n_kf // 2 - 1
    anchor = np.concatenate([np.repeat(np.arange(n_kf), per_kf), np.repeat(lb, loop_points)])
    npt = len(anchor)
    nband = n_kf * per_kf
    e_pt, e_kf = [], []
    for d in range(-band, band + 1):
        k = anchor[:nband] + d
        ok = (k >= 0) & (k < n_kf)
        e_pt.append(np.flatnonzero(ok))
        e_kf.append(k[ok])
    e_pt += [np.arange(nband, npt), np.arange(nband, npt)]
    e_kf += [np.repeat(la, loop_points), np.repeat(lb, loop_points)]
    e_pt, e_kf = np.concatenate(e_pt), np.concatenate(e_kf)
    order = np.lexsort((e_kf, e_pt))
    e_pt, e_kf = e_pt[order], e_kf[order]
    depth = rng.uniform(8, 40, npt) + 1.5 * band
    xc = np.stack([rng.uniform(-0.4, 0.4, npt) * depth, rng.uniform(-0.15, 0.15, npt) * depth, depth], 1)
    X = np.einsum("nji,nj->ni", Rm[anchor], xc - t[anchor])
    c = np.einsum("eij,ej->ei", Rm[e_kf], X[e_pt]) + t[e_kf]
    assert (c[:, 2] > 1).all()
    ne = len(e_pt)
    E = np.zeros(ne, L.EDGE_DTYPE)
    E["point"], E["pose"] = e_pt, e_kf
    lv = rng.integers(0, 8, ne)
    E["inv_sigma2"] = (1.0 / (np.float32(1.2) ** (2 * lv)).astype(np.float32)).astype(np.float32)
    E["fx"], E["fy"], E["cx"], E["cy"], E["bf"] = CAM
    u = CAM[0] * c[:, 0] / c[:, 2] + CAM[2]
    v = CAM[1] * c[:, 1] / c[:, 2] + CAM[3]
    nz = rng.normal(0, 0.5, (ne, 3))
    st = rng.random(ne) < 0.6
    E["obs"][:, 0] = (u + nz[:, 0]).astype(np.float32)
    E["obs"][:, 1] = (v + nz[:, 1]).astype(np.float32)
    E["obs"][:, 2] = np.where(st, (u - CAM[4] / c[:, 2] + nz[:, 2]).astype(np.float32), 0.0)
    E["stereo"] = st
    E["huber_delta"] = np.where(st, np.float32(np.sqrt(7.815)), np.float32(np.sqrt(5.99)))
    E["robust"], E["active"] = 0, 1
    P = np.zeros(n_kf, L.POSE_DTYPE)
    P["q"], P["t"] = q, t
    P["fixed"][0] = 1
    P["t"][1:] += rng.normal(0, 2e-3, (n_kf - 1, 3))
    return P, X + rng.normal(0, 5e-2, X.shape), E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,500,1500")
    ap.add_argument("--dense-max", type=int, default=500)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from orb_slam2_test_amd.optimizer import DeviceLBA
    lines = []
    for n_kf in [int(s) for s in args.sizes.split(",")]:
        poses, pts, edges = trajectory(n_kf)
        paths = {}
        for kind in ("sparse", "dense"):
            if kind == "dense" and n_kf > args.dense_max:
                continue
            g = DeviceLBA(poses, pts, edges, graph=True)
            t0 = time.perf_counter()
            info = g.schur_plan(poses["fixed"], sparse=kind == "sparse")
            g.ctx.sync()
            paths[kind] = dict(g=g, plan_ms=(time.perf_counter() - t0) * 1e3, info=info, wall=[],
                               p0=g.d_poses.clone(), q0=g.d_points.clone())

        def run(p):
            p["g"].d_poses.copy_(p["p0"])
            p["g"].d_points.copy_(p["q0"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = p["g"].optimize(10)
            return (time.perf_counter() - t0) * 1e3, rep

        for i in range(args.warmup + args.steps):      # interleaved: sparse, dense, sparse, ...
            for kind, p in paths.items():
                ms, p["rep"] = run(p)
                if i >= args.warmup:
                    p["wall"].append(ms)
                print("# %d keyframes %s call %d: %.2f ms" % (n_kf, kind, i, ms), flush=True)
        for kind, p in paths.items():                  # one profiled call each (HIP events)
            ctx = p["g"].ctx
            ctx.profile(True)
            ctx.profile_reset()
            run(p)
            kern = ctx.profile_read()
            ctx.profile(False)
            ctx.profile_reset()
            p["kernel_ms"] = {k: round(v[0], 4) for k, v in sorted(kern.items())}
            p["launches"] = {k: int(v[1]) for k, v in sorted(kern.items())}
        r = {"metric": "GlobalBundleAdjustment optimize(10) time per call, sparse Schur plan",
             "value": round(float(np.median(paths["sparse"]["wall"])), 3), "unit": "ms",
             "higher_is_better": False, "data": "synthetic", "dtype": "f64",
             "config": {"workload": "%d keyframes, %d points, %d edges, band 3, %d loop closures, "
                                    "optimize(10) not robust" % (n_kf, len(pts), len(edges), n_kf // 50),
                        "steps": args.steps, "warmup": args.warmup, "interleaved": True}}
        for kind, p in paths.items():
            rep = p["rep"]
            r[kind] = {"wall_ms_median": round(float(np.median(p["wall"])), 3),
                       "wall_ms_min": round(float(np.min(p["wall"])), 3),
                       "wall_ms_max": round(float(np.max(p["wall"])), 3),
                       "plan_ms_host": round(p["plan_ms"], 3), "iterations": rep["iterations"],
                       "trials": rep["trials"], "final_chi2": rep["final_chi2"],
                       "kernel_ms_per_call": p["kernel_ms"], "launches_per_call": p["launches"]}
            if p["info"]:
                r[kind]["plan"] = p["info"]
        if "dense" in paths:
            r["dense_over_sparse_median"] = round(r["dense"]["wall_ms_median"] /
                                                  r["sparse"]["wall_ms_median"], 3)
        else:
            r["dense"] = "not run above --dense-max %d keyframes" % args.dense_max
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        paths.clear()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
