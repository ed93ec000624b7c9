#!/usr/bin/env python3
"""Throughput of the device PnPsolver (csrc/pnp_kernels.hip, orbg_pnp_solve_batch_device), one
JSON line with HIP-event kernel times:

  256 relocalization candidates x 300 RANSAC iterations x n correspondences per launch,
  min_set 4 (Tracking::Relocalization's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
  32 distinct synthetic scenes of synthetic.pnp_scene, each used 8 times with its own draws):
  candidates/s.  --iterations 0 runs SetRansacParameters' own count instead of 300.

Work per launch: candidates x iterations EPnP solves on 4 points (fp64) and candidates x
iterations x n inlier tests, then one EPnP on all inliers per record iteration.  The NumPy
reference of tests/ref_pnp.py (float64, one core) evaluates the same iterations of a bounded
sample of candidates for scale.  ORBG_LIB_VARIANT selects a variant build of the library
(e.g. one made with EXTRA=-DORBG_PNP_HYP_LANES=64: a wave per hypothesis).

    python tools/pnp_bench.py [--steps 20] [--warmup 3] [--n 300] [--no-cpu]
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
    ap.add_argument("--n", type=int, default=300, help="correspondences per candidate")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from orb_slam2_test_amd import _lib as L, synthetic
    from orb_slam2_test_amd import pnpsolver as S
    from orb_slam2_test_amd.orbmatcher import _ctx
    ctx = _ctx()
    NQ, REP, ITS, MIN_SET = 32, 8, 300, 4
    P, n = NQ * REP, args.n
    cap = (n + 63) // 64 * 64
    scenes = [synthetic.pnp_scene(seed=700 + q, n=n, inliers=int(0.6 * n), noise=0.7) for q in range(NQ)]
    mi, its = S.ransac_parameters(0.99, 10, ITS, MIN_SET, 0.5, n)
    if args.iterations:
        its = min(args.iterations, ITS)
    probs = np.zeros(P, L.PNP_PROBLEM_DTYPE)
    corrs = np.zeros((P, cap), L.PNP_CORR_DTYPE)
    samples = np.zeros((P, ITS, L.PNP_MAX_SET), np.int32)
    for p in range(P):
        sc = scenes[p % NQ]
        probs[p] = S.make_problem(sc["K"], n, MIN_SET, mi, its)[0]
        corrs[p, :n] = S.make_corrs(sc["Xw"], sc["uv"], sc["sigma2"], sc["index"])
        rng = np.random.default_rng(9000 + p)
        samples[p, :its, :MIN_SET] = S.draw_samples(n, its, MIN_SET,
                                                    rng.integers(0, 2147483648, MIN_SET * its).tolist())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = [up(probs), up(corrs), up(samples)]
    torch.cuda.synchronize()
    out = S.solve_batch(t[0], t[1], t[2], P, cap, ITS, n, ctx=ctx)

    def run():
        S.solve_batch(t[0], t[1], t[2], P, cap, ITS, n, out=out, ctx=ctx)
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
    kt = {k: v[0] / max(v[1], 1) for k, v in kern.items() if k.startswith("pnp_")}
    res = out["results"].cpu().numpy().reshape(-1).view(L.PNP_RESULT_DTYPE)
    rf = out["refines"].cpu().numpy().reshape(P, ITS, -1).view(L.PNP_REFINE_DTYPE)[..., 0]
    r = {"metric": "PnPsolver (EPnP RANSAC, Tracking::Relocalization) candidates/s",
         "value": round(P / dt, 1), "unit": "candidates/s", "higher_is_better": True,
         "data": "synthetic", "dtype": "f64",
         "config": {"workload": "%d candidates x %d iterations x %d correspondences (40%% outliers, "
                                "0.7 px noise), min_set %d, min_inliers %d" % (P, its, n, MIN_SET, mi),
                    "library": os.environ.get("ORBG_LIB_VARIANT", "product"),
                    "candidates_with_a_hit": int((res["hit_iter"] >= 0).sum()),
                    "record_iterations": int(rf["valid"].sum()),
                    "mean_inliers": round(float(res["ninliers"].mean()), 1)},
         "ms_per_step": round(dt * 1e3, 4),
         "kernels": {k: round(v, 5) for k, v in kt.items()},
         "kernel_ms": round(sum(kt.values()), 5),
         "hypotheses_per_s": round(P * its / (sum(kt.values()) * 1e-3), 1) if kt else None}
    if not args.no_cpu:
        import ref_pnp as R
        t0 = time.perf_counter()
        calls = 0
        while time.perf_counter() - t0 < 3.0:
            sc = scenes[calls % NQ]
            R.evaluate(sc, samples[calls % P, :its, :MIN_SET])
            calls += 1
        cdt = time.perf_counter() - t0
        r["cpu_baseline"] = {"value": round(calls / cdt, 2), "unit": "candidates/s", "cores": 1,
                             "kind": "numpy float64 reference (tests/ref_pnp.py)",
                             "sample": "%d candidates, %.2f s" % (calls, cdt)}
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
