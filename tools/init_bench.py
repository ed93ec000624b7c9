#!/usr/bin/env python3
"""Throughput of the device Initializer (csrc/init_kernels.hip, orbg_initialize_batch_device),
one JSON line with HIP-event kernel times, printed and appended to profiles/init_bench.jsonl:

  512 frame pairs x 200 RANSAC iterations x 300 .. 1500 matches per launch (Tracking's
  Initializer(frame, 1.0, 200); 32 distinct synthetic two-view scenes of
  tests/ref_initializer.make_scene -- half of them planar -- with 20 % wrong matches and a
  quarter more keypoints than matches, each used 16 times with its own draws): pairs/s.

Work per launch: pairs x iterations x 2 eight-point models (two 9x9 eigen solves in fp64),
pairs x iterations x 2 x N chi-square tests, then 4 or 8 triangulate-and-check passes over the
inliers of each pair.  lib/init_host (csrc/init_host.hip), the same statements on one host
core, runs a bounded sample of the pairs for scale.  ORBG_LIB_VARIANT selects a variant build
of the library.

    python tools/init_bench.py [--steps 10] [--warmup 2] [--pairs 512] [--no-cpu] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import ref_initializer as R
    import init_checks as K
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd import initializer as I
    from orb_slam2_test_amd.orbmatcher import _ctx
    ctx = _ctx()
    NQ, P, ITS, CAP = 32, args.pairs, args.iterations, 2048
    scenes = []
    for q in range(NQ):
        nm = 300 + (1200 * q) // (NQ - 1)
        kw = dict(seed=500 + q, nmatch=nm, nkeys=nm + nm // 4, depth=(3.0, 8.0))
        if q % 2:
            kw.update(depth=None, plane=(5.0, 0.8, 0.3))
        scenes.append(R.make_scene(**kw))
    cases = []
    for p in range(P):
        sc = scenes[p % NQ]
        n = I.count_matches(sc["matches12"], len(sc["keys2"]))
        rng = np.random.default_rng(9000 + p)
        cases.append((sc, I.draw_sets(n, ITS, rng.integers(0, 2147483648, 8 * ITS).tolist()), ITS))
    arrays = K.batch_arrays(I, L, cases, CAP)
    probs, kps, counts, f1, f2, m12, sets = arrays
    nmatch = [I.count_matches(c[0]["matches12"], len(c[0]["keys2"])) for c in cases]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = [up(a) for a in arrays]
    torch.cuda.synchronize()
    call = dict(frame_stride=kps.shape[1], nframes=len(counts), npairs=P, cap=CAP, max_its=ITS)

    def run(out=None):
        return I.initialize_batch(t[0], t[1], call["frame_stride"], t[2], call["nframes"], t[3], t[4],
                                  t[5], t[6], P, CAP, ITS, out=out, ctx=ctx)
    out = run()
    for _ in range(args.warmup):
        run(out)
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run(out)
    ctx.sync()
    dt = (time.perf_counter() - t0) / args.steps
    kern = ctx.profile_read()
    ctx.profile(False)
    kt = {k: v[0] / max(v[1], 1) for k, v in kern.items() if k.startswith("init_")}
    res = out["results"].cpu().numpy().reshape(-1).view(L.INIT_RESULT_DTYPE)
    tests = 2.0 * ITS * float(np.sum(nmatch))
    r = {"metric": "Initializer (H/F RANSAC + two-view reconstruction, MonocularInitialization) pairs/s",
         "value": round(P / dt, 1), "unit": "pairs/s", "higher_is_better": True,
         "data": "synthetic", "dtype": "f64 linear algebra, f32 tests",
         "config": {"workload": "%d pairs x %d iterations x %d .. %d matches (mean %.0f; 20%% wrong, "
                                "0.5 px noise), cap %d" % (P, ITS, min(nmatch), max(nmatch),
                                                           np.mean(nmatch), CAP),
                    "library": os.environ.get("ORBG_LIB_VARIANT", "product"),
                    "pairs_initialised": int(res["success"].sum()),
                    "model_h": int((res["model"] == 1).sum()), "model_f": int((res["model"] == 2).sum())},
         "ms_per_step": round(dt * 1e3, 4),
         "kernels": {k: round(v, 5) for k, v in kt.items()},
         "kernel_ms": round(sum(kt.values()), 5),
         "chi2_tests_per_s": round(tests / (kt["init_score"] * 1e-3), 1) if "init_score" in kt else None}
    if not args.no_cpu:
        sample = cases[:NQ]
        host, secs = K.run_host(I, L, sample, CAP)
        same = all(host["results"][p].tobytes() == res[p].tobytes() for p in range(len(sample)))
        r["cpu_baseline"] = {"value": round(len(sample) / secs, 2), "unit": "pairs/s", "cores": 1,
                             "kind": "lib/init_host: the kernels' statements on one host core",
                             "sample": "%d pairs, %.2f s" % (len(sample), secs),
                             "records_equal_the_device": bool(same)}
    line = json.dumps(r)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
