#!/usr/bin/env python3
"""Device time of Optimizer::OptimizeSim3 (csrc/sim3opt_kernels.hip,
orbg_optimize_sim3_batch_device), one JSON line per configuration with HIP-event kernel times:

  256 loop candidates x 150 correspondences with 20 % gross outliers per launch, th2 = 10, once
  with a free scale (monocular) and once with the scale fixed (32 distinct scenes of
  tests/ref_sim3opt.py, each used 8 times).

This is a latency figure: one workgroup per candidate, a handful of candidates per loop
closure in real use.  For scale, lib/sim3opt_host runs the same batch on one host core through
the very __host__ __device__ statements the kernel runs (csrc/sim3opt_args.h), in the kernel's
summation order; the records of the two are compared byte for byte.  Neither number has a
pass / fail threshold.

    python tools/sim3opt_bench.py [--steps 20] [--warmup 3] [--n 150] [--no-cpu]
        [--out profiles/sim3opt_bench.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_run(L, probs, corrs, init, n1cap, repeat):
    exe = os.path.join(os.path.dirname(L.LIB_PATH), "sim3opt_host")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(np.array([len(probs), corrs.shape[1], n1cap, 0], np.int32).tobytes())
            f.write(probs.tobytes())
            f.write(corrs.tobytes())
            f.write(init.tobytes())
        sec = float(subprocess.check_output([exe, os.path.join(d, "in"), os.path.join(d, "out"),
                                             str(repeat)]))
        raw = open(os.path.join(d, "out"), "rb").read()
    nb = len(probs) * L.SIM3OPT_RESULT_DTYPE.itemsize
    return sec, raw[:nb], raw[nb:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=150, help="correspondences per candidate")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import ref_sim3opt as R
    from orb_slam2_test_amd import _lib as L, optimizer as O
    from orb_slam2_test_amd.orbmatcher import _ctx
    ctx = _ctx()
    NQ, REP = 32, 8
    P, n = NQ * REP, args.n
    cap = (n + 63) // 64 * 64
    lines = []
    for fix_scale in (False, True):
        scenes = [R.scene(n=n, seed=900 + q, n_out=n // 5, fix_scale=fix_scale) for q in range(NQ)]
        n1cap = max(sc["n1"] for sc in scenes)
        probs = np.zeros(P, L.SIM3OPT_PROBLEM_DTYPE)
        corrs = np.zeros((P, cap), L.SIM3OPT_CORR_DTYPE)
        init = np.zeros(P, L.SIM3_HYP_DTYPE)
        for p in range(P):
            sc = scenes[p % NQ]
            pr, c, h = O.sim3opt_records(sc["T1w"], sc["T2w"], sc["K1"], sc["K2"], sc["Xw1"],
                                         sc["Xw2"], sc["obs1"], sc["obs2"], sc["inv_sigma2_1"],
                                         sc["inv_sigma2_2"], sc["index1"], sc["R12"], sc["t12"],
                                         sc["s12"], sc["th2"], fix_scale)
            probs[p], corrs[p, :n], init[p] = pr[0], c, h[0]

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        d_p, d_c, d_h = up(probs), up(corrs), up(init)
        d_r = torch.zeros(P * L.SIM3OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_k = torch.zeros(P * n1cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def run():
            L.check(L.lib().orbg_optimize_sim3_batch_device(
                ctx.handle, d_p.data_ptr(), d_c.data_ptr(), d_h.data_ptr(), P, cap,
                d_r.data_ptr(), d_k.data_ptr(), n1cap), "orbg_optimize_sim3_batch_device")
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
        kt = {k: v[0] / max(v[1], 1) for k, v in kern.items() if k == "sim3_opt"}
        raw_r, raw_k = d_r.cpu().numpy(), d_k.cpu().numpy()
        res = raw_r.view(L.SIM3OPT_RESULT_DTYPE)
        r = {"metric": "OptimizeSim3 (LoopClosing::ComputeSim3) device time per batch",
             "value": round(sum(kt.values()), 5) if kt else round(dt * 1e3, 5), "unit": "ms",
             "higher_is_better": False, "data": "synthetic", "dtype": "f64",
             "config": {"workload": "%d candidates x %d correspondences (20%% outliers), th2 10, "
                                    "fix_scale %d" % (P, n, int(fix_scale)),
                        "mean_inliers": round(float(res["ninliers"].mean()), 1),
                        "mean_lm_iterations": round(float(res["iterations"].sum(1).mean()), 2)},
             "ms_per_step_wall": round(dt * 1e3, 4),
             "kernel_ms": {k: round(v, 5) for k, v in kt.items()},
             "us_per_candidate": round(sum(kt.values()) * 1e3 / P, 3) if kt else None}
        if not args.no_cpu:
            sec, hr, hk = host_run(L, probs, corrs, init, n1cap, 3)
            r["host_one_core"] = {"value": round(sec * 1e3, 4), "unit": "ms per batch", "cores": 1,
                                  "kind": "lib/sim3opt_host (the kernel's __host__ __device__ "
                                          "statements)",
                                  "us_per_candidate": round(sec * 1e6 / P, 3),
                                  "records_equal_device": bool(hr == raw_r.tobytes()),
                                  "keep_equal_device": bool(hk == raw_k.tobytes())}
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
