#!/usr/bin/env python3
"""Throughput of the device Sim3Solver (csrc/sim3_kernels.hip,
orbg_sim3_solve_batch_device), one JSON line with HIP-event kernel times:

  256 candidate pairs x 300 RANSAC iterations x n correspondences per launch
  (LoopClosing::ComputeSim3's SetRansacParameters(0.99, 20, 300); 32 distinct synthetic
  scenes of synthetic.sim3_scene, each used 8 times with its own draws): pairs/s.

Work per launch: pairs x iterations Horn solves and pairs x iterations x n inlier tests
(two projections each).  The NumPy reference of tests/ref_sim3.py (float64, one core)
evaluates the same iterations of a bounded sample of pairs for scale.

    python tools/sim3_bench.py [--steps 20] [--warmup 3] [--n 300] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=300, help="correspondences per pair")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from orb_slam2_test_amd import _lib as L, synthetic
    from orb_slam2_test_amd import sim3solver as S
    from orb_slam2_test_amd.orbmatcher import _ctx
    ctx = _ctx()
    NQ, REP, ITS, MIN_INL = 32, 8, 300, 20
    P, n = NQ * REP, args.n
    cap = (n + 63) // 64 * 64
    scenes = [synthetic.sim3_scene(seed=700 + q, n=n) for q in range(NQ)]
    its = S.ransac_iterations(0.99, MIN_INL, ITS, n)
    probs = np.zeros(P, L.SIM3_PROBLEM_DTYPE)
    corrs = np.zeros((P, cap), L.SIM3_CORR_DTYPE)
    samples = np.zeros((P, ITS, 3), np.int32)
    for p in range(P):
        sc = scenes[p % NQ]
        probs[p] = S.make_problem(sc["T1w"], sc["T2w"], sc["K"], sc["K"], n, False, MIN_INL, its)[0]
        corrs[p, :n] = S.make_corrs(sc["Xw1"], sc["Xw2"], sc["sigma2_1"], sc["sigma2_2"], sc["index1"])
        rng = np.random.default_rng(9000 + p)
        samples[p, :its] = S.draw_samples(n, its, rng.integers(0, 2147483648, 3 * its).tolist())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = [up(probs), up(corrs), up(samples)]
    torch.cuda.synchronize()
    out = S.Sim3Solver.solve_batch(t[0], t[1], t[2], P, cap, ITS, n, ctx=ctx)

    def run():
        S.Sim3Solver.solve_batch(t[0], t[1], t[2], P, cap, ITS, n, out=out, ctx=ctx)
    for _ in range(args.warmup):
        run()
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    ctx.sync()
    dt = (time.perf_counter() - t0) / args.steps
    kern = ctx.profile_read()
    ctx.profile(False)
    kt = {k: v[0] / max(v[1], 1) for k, v in kern.items() if k.startswith("sim3_")}
    res = out["results"].cpu().numpy().reshape(-1).view(L.SIM3_RESULT_DTYPE)
    r = {"metric": "Sim3Solver (Horn RANSAC, LoopClosing::ComputeSim3) candidate pairs/s",
         "value": round(P / dt, 1), "unit": "pairs/s", "higher_is_better": True,
         "data": "synthetic", "dtype": "f32",
         "config": {"workload": "%d pairs x %d iterations x %d correspondences (30%% outliers, "
                                "0.02 noise), min_inliers %d" % (P, its, n, MIN_INL),
                    "pairs_with_a_hit": int((res["hit_iter"] >= 0).sum()),
                    "mean_inliers": round(float(res["ninliers"].mean()), 1)},
         "ms_per_step": round(dt * 1e3, 4),
         "kernels": {k: round(v, 5) for k, v in kt.items()},
         "kernel_ms": round(sum(kt.values()), 5),
         "hypotheses_per_s": round(P * its / (sum(kt.values()) * 1e-3), 1) if kt else None,
         "inlier_tests_per_s": round(P * its * n / (sum(kt.values()) * 1e-3), 1) if kt else None}
    if not args.no_cpu:
        import ref_sim3 as R
        t0 = time.perf_counter()
        calls = 0
        while time.perf_counter() - t0 < 3.0:
            sc = scenes[calls % NQ]
            R.evaluate(sc, samples[calls % P, :its])
            calls += 1
        cdt = time.perf_counter() - t0
        r["cpu_baseline"] = {"value": round(calls / cdt, 1), "unit": "pairs/s", "cores": 1,
                             "kind": "numpy float64 reference (tests/ref_sim3.py)",
                             "sample": "%d pairs, %.2f s" % (calls, cdt)}
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
