#!/usr/bin/env python3
"""LocalMapping::KeyFrameCulling / MapPointCulling on the device Map, timed at DESIGN.md's map
size beside tools/map_bench.py: K keyframes of N features on a trajectory (keyframe s observes the
points [step * s, step * s + N), step = N / 40: about 40 observations per point, 78 connected
keyframes per slot, all above the threshold of 15).  A feature's octave is its point's base
octave plus a jitter from {-1, 0, 0, 0, 1, 2}.

Timed (HIP events around the launches, the context's profiler):
  cull_score           the scoring launch alone (one workgroup per list entry), beside its
                       algorithmic bytes: per list entry the row (4 B / feature), the feature's
                       flags and octave (2 B), per point its flags and two index offsets (12 B),
                       per observation the index entry, the observer's slot flags, row entry,
                       feature flags and octave (14 B)
  keyframe_culling     the whole call (score + the sequential pass + the deferred re-sorts)
    no_erasure         every list entry marked not-erase: each scores redundant or not, none is
                       erased, nothing is scored twice; `--steps` calls after `--warmup`
    erasures           the erasures the scene produces, on `--slots` culling slots far apart (an
                       erasure changes the map, so each is ONE run: HIP-event time of one call)
  point_culling        MapPointCulling of `--recent` distinct recent points (one run per culling
                       slot: it sets points bad)
  rebuild              the observation-index rebuild that follows a culling call

Appends nothing itself; prints one JSON line (profiles/culling_bench.jsonl keeps them).

    python tools/culling_bench.py [--keyframes 2000] [--features 2000] [--recent 4000]
                                  [--steps 5] [--warmup 2]
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
    ap.add_argument("--recent", type=int, default=4000)
    ap.add_argument("--slots", type=int, nargs="*", default=[300, 700, 1100, 1500, 1900])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from orb_slam2_test_amd import Map
    from orb_slam2_test_amd import _lib as L
    from orb_slam2_test_amd.orbmatcher import _ctx

    K, N = args.keyframes, args.features
    Kmax = 1 << (K - 1).bit_length()
    step = max(N // 40, 1)
    P = step * (K - 1) + N
    ctx = _ctx(0)
    m = Map(Kmax, N, P)
    rng = np.random.default_rng(6)

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    rec = np.zeros(P, L.MAPPOINT_DTYPE)
    rec["x"], rec["y"], rec["z"] = np.arange(P) * (40.0 / P), rng.uniform(-2, 2, P), rng.uniform(6, 12, P)
    rec["flags"] = L.MP_VALID
    ref = np.minimum(np.arange(P) // step, K - 1).astype(np.int32)
    rows = (np.arange(K, dtype=np.int32)[:, None] * step + np.arange(N, dtype=np.int32)[None])
    base = rng.integers(0, 8, P)
    octs = np.clip(base[rows] + rng.choice([-1, 0, 0, 0, 1, 2], (K, N)), 0, 7).astype(np.uint8)
    flags = np.zeros(K, np.int32)
    flags[0] = 1
    centres = np.stack([np.arange(K) * (40.0 / K), np.zeros(K), np.zeros(K)], 1).astype(np.float32)
    t = [cuda(a) for a in (rec.view(np.uint8).reshape(-1), ref, np.arange(K, dtype=np.int32), rows,
                           octs, np.full(K, N, np.int32), centres, flags)]
    t_desc = torch.randint(0, 256, (P, 32), dtype=torch.uint8, device="cuda")
    t_stats = [cuda(a.astype(np.int32)) for a in (rng.integers(K - 4, K + 1, P),
                                                  rng.integers(0, 20, P), rng.integers(0, 12, P))]
    torch.cuda.synchronize()
    m.set_points_device(None, 0, P, t[0].data_ptr(), t_desc.data_ptr(), t[1].data_ptr(), ctx)
    m.set_point_stats_device(None, 0, P, *[x.data_ptr() for x in t_stats], ctx)
    m.set_keyframes_device(t[2].data_ptr(), K, t[3].data_ptr(), t[4].data_ptr(), N,
                           t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), ctx)
    m.update_connections_batch_device(t[2].data_ptr(), K, ctx)
    ctx.sync()

    t_rec = torch.zeros((Kmax, 4), dtype=torch.int32, device="cuda")
    t_n = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def read_prof():
        ctx.sync()
        kern = ctx.profile_read()
        ctx.profile_reset()
        return {k[4:]: v[0] / v[1] for k, v in kern.items() if k.startswith("map_") and v[1]}

    def cull(slot):
        m.keyframe_culling_device(slot, True, t_rec.data_ptr(), Kmax, t_n.data_ptr(), ctx)

    # no erasure: the list entries of one slot marked not-erase
    s0 = K // 2
    lst = m.GetVectorCovisibleKeyFrames(s0)
    for s in lst:
        m.SetNotErase(s)
    for _ in range(args.warmup):
        cull(s0)
        m.rebuild(ctx)
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(args.steps):
        cull(s0)
        m.rebuild(ctx)
    ms = read_prof()
    r0 = t_rec[:len(lst)].cpu().numpy()
    assert t_n[0].item() == len(lst) and not (r0[:, 1] == 1).any()
    nobs = np.zeros(P, np.int64)
    for s in range(K):
        nobs[s * step:s * step + N] += 1
    b_score = int(sum(N * (4 + 2 + 12) + nobs[s * step:s * step + N].sum() * 14 for s in lst))
    for s in lst:
        m.SetErase(s)                    # erases the entries the calls marked; leaves s0's area
    ctx.profile_reset()

    # the erasures the scene produces: one run per culling slot
    runs = []
    for slot in args.slots:
        n_list = len(m.GetVectorCovisibleKeyFrames(slot))
        ctx.profile_reset()
        cull(slot)
        m.rebuild(ctx)
        p = read_prof()
        r = t_rec[:n_list].cpu().numpy()
        lo = max(slot * step - N, 0)
        recent = (lo + rng.permutation(min(3 * N, P - lo))[:args.recent]).astype(np.int32)
        t_recent = cuda(recent)
        torch.cuda.synchronize()
        m.point_culling_device(t_recent.data_ptr(), len(recent), K, True, t_n[1:].data_ptr(), None, ctx)
        m.rebuild(ctx)
        q = read_prof()
        runs.append({"slot": slot, "list": n_list, "erased": int((r[:, 1] == 1).sum()),
                     "score_ms": round(p["cull_score"], 4),
                     "call_ms": round(p["cull_score"] + p["cull_sequence"], 4),
                     "rebuild_ms": round(p["rebuild"], 4),
                     "point_culling_ms": round(q["point_culling"], 4),
                     "recent": len(recent), "recent_kept": int(t_n[1].item())})
    ctx.profile(False)

    frac = b_score / (ms["cull_score"] * 1e-3) / HBM_BPS
    res = {
        "metric": "KeyFrameCulling call with the scene's erasures, K=%d keyframes (median of %d single runs)"
                  % (K, len(runs)),
        "value": float(np.median([r["call_ms"] for r in runs])) if runs else None,
        "unit": "ms", "higher_is_better": False, "dtype": "i32/u16/u8", "data": "synthetic",
        "config": {"keyframes": K, "max_keyframes": Kmax, "features": N, "points": int(P),
                   "observations_per_point": round(float(nobs.mean()), 1), "list_entries": len(lst),
                   "steps": args.steps, "warmup": args.warmup},
        "cull_score": {"ms": round(ms["cull_score"], 4), "bytes": b_score,
                       "gbs": round(b_score / (ms["cull_score"] * 1e-3) / 1e9, 1),
                       "hbm_frac": round(frac, 4), "bound": "bytes" if frac > 0.3 else "latency"},
        "keyframe_culling_no_erasure": {"ms": round(ms["cull_score"] + ms["cull_sequence"], 4),
                                        "redundant_entries": int((r0[:, 1] == 2).sum())},
        "rebuild_after": {"ms": round(ms["rebuild"], 4)},
        "erasure_runs": runs,
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
