#!/usr/bin/env python3
"""Device time of Optimizer::OptimizeEssentialGraph (csrc/essential_kernels.hip behind the
orbg_eg_graph entry points): a ring of 1500 keyframes (tests/ref_essential.py's scene: spanning
tree, two covisibility edges per keyframe, LoopConnections at the closure), optimize(20) with
the scale free and with the scale fixed.  One JSON line per configuration: the host plan's
time, ms per orbg_eg_graph_optimize call (wall, upload excluded), HIP-event kernel times per
phase and call, iterations and trials.

This is a latency figure: one call per loop closure.  Nothing comparable ran before it, so no
number has a pass / fail threshold.

    python tools/essential_bench.py [--n 1500] [--steps 5] [--warmup 1]
        [--out profiles/essential_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ("eg_perturb", "eg_linearize", "eg_assemble", "eg_solve", "eg_update", "eg_errors")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1500, help="keyframes")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import ref_essential as E
    from orb_slam2_test_amd import _lib as L, optimizer as O
    from orb_slam2_test_amd.orbmatcher import _ctx
    ctx = _ctx()
    lines = []
    for fix_scale in (False, True):
        sc = E.scene(n=args.n, seed=77, ncorr=10, fix_scale=fix_scale, rot_drift=1e-4,
                     scale_drift=1e-4)
        Scw, Snc = O.sim3d_records(list(zip(*sc["Scw"]))), O.sim3d_records(list(zip(*sc["Snc"])))
        t0 = time.perf_counter()
        g = O.EssentialGraph(sc["edges"], sc["n"], sc["fixed"])
        plan_ms = (time.perf_counter() - t0) * 1e3
        nfree, hb, lb = g.info()

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        d_c, d_n = up(Scw), up(Snc)
        d_o = torch.zeros(sc["n"] * 64, dtype=torch.uint8, device="cuda")
        d_t = torch.zeros(sc["n"] * 12, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rep = L.LmReport()

        def run():
            L.check(L.lib().orbg_eg_graph_optimize(ctx.handle, g.handle, d_c.data_ptr(), d_n.data_ptr(),
                                                   int(fix_scale), 20, d_o.data_ptr(), d_t.data_ptr(),
                                                   ctypes.byref(rep)), "orbg_eg_graph_optimize")
        for _ in range(args.warmup):
            run()
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run()
        dt = (time.perf_counter() - t0) / args.steps
        kern = ctx.profile_read()
        ctx.profile(False)
        ctx.profile_reset()
        kt = {k: kern[k][0] / args.steps for k in PHASES if k in kern}
        calls = {k: kern[k][1] // args.steps for k in PHASES if k in kern}
        r = {"metric": "OptimizeEssentialGraph (LoopClosing::CorrectLoop) time per call",
             "value": round(dt * 1e3, 4), "unit": "ms", "higher_is_better": False,
             "data": "synthetic", "dtype": "f64",
             "config": {"workload": "ring of %d keyframes, %d edges, fix_scale %d, optimize(20)"
                                    % (sc["n"], len(sc["edges"]), int(fix_scale)),
                        "free_vertices": nfree, "h_blocks": hb, "l_blocks": lb,
                        "iterations": rep.iterations, "trials": rep.trials,
                        "terminated": rep.terminated, "initial_chi2": rep.initial_chi2,
                        "final_chi2": rep.final_chi2},
             "plan_ms_host": round(plan_ms, 3),
             "kernel_ms_per_call": {k: round(v, 4) for k, v in kt.items()},
             "launches_per_call": calls,
             "kernel_ms_per_launch": {k: round(kt[k] / max(calls[k], 1), 4) for k in kt}}
        g.close()
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
