"""GPU: the device PnPsolver (csrc/pnp_kernels.hip behind orbg_pnp_solve and
orbg_pnp_solve_batch_device, and the Python class on top) against the float64 reference of
tests/ref_pnp.py.

What the device derives from its own per-iteration outputs (the record flags, the result, Tcw,
ninliers, the inlier bytes) is checked exactly, on every scene and every min_set.  Masks are
checked against NumPy's CheckInliers on the device's own double hypotheses.  Hypotheses are
compared with the reference iteration by iteration where EPnP is well posed (min_set 6 and 8)
and at every Refine(); at min_set = 4, where the null-space basis of M^T M is arbitrary and
no two implementations agree iteration by iteration, the comparison is statistical.

tests/test_pnp_ref.py holds the CPU side of the premises: the reference's own sensitivity (the
1e-6 tolerance here is 10 x the bound asserted there), the share of decisions inside the
threshold band, the remixed basis passing the same statistical test, and that the hit is
determined on the scenes where hit_iter is compared.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_pnp as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    from orb_slam2_test_amd import pnpsolver
    return pnpsolver


@pytest.fixture(scope="module")
def L():
    from orb_slam2_test_amd import _lib
    return _lib


def records(P, scene, min_set, min_inliers, iterations):
    p = P.make_problem(scene["K"], scene["n"], min_set, min_inliers, iterations, R.TH2)
    c = P.make_corrs(scene["Xw"], scene["uv"], scene["sigma2"], scene["index"])
    return p, c


_solved = {}


def device_solve(P, scene, samples, min_inliers, iterations, key=None):
    if key is not None and key in _solved:
        return _solved[key]
    min_set = samples.shape[1]
    p, c = records(P, scene, min_set, min_inliers, iterations)
    if len(samples) < iterations:   # iterations that never run read no sample
        samples = np.concatenate([samples, np.zeros((iterations - len(samples), min_set), np.int32)])
    d = P.solve(p, c, samples, scene["n1"])
    n = scene["n"]
    d["bits"] = R.unpack_masks(d["masks"], n) if n else np.zeros((len(d["counts"]), 0), bool)
    d["refined_bits"] = R.unpack_masks(d["refined_masks"], n) if n else d["bits"].copy()
    d["R"] = d["hyps"]["R"].reshape(-1, 3, 3)
    d["t"] = d["hyps"]["t"]
    if key is not None:
        _solved[key] = d
    return d


def solve_case(P, name):
    scene, samples, mi, its = R.case(name)
    return scene, samples, mi, its, device_solve(P, scene, samples, mi, its, key=name)


def check_own_outputs(L, scene, min_inliers, d):
    """The record flags are the strict prefix maximum of the device's counts; result, Tcw,
    ninliers and the inlier bytes are exactly what the acceptance rule makes of the device's
    own counts, hypotheses, refine records and masks; every hypothesis is a rotation."""
    n, counts, rf = scene["n"], d["counts"], d["refines"]
    recs = R.records(counts.tolist(), min_inliers) if n >= min_inliers else []
    assert np.flatnonzero(rf["valid"]).tolist() == recs
    rest = np.ones(len(counts), bool)
    rest[recs] = False
    assert rf[rest].tobytes() == bytes(int(rest.sum()) * L.PNP_REFINE_DTYPE.itemsize)
    assert not d["refined_masks"][rest].any()
    assert np.array_equal(d["bits"].sum(1), counts)
    for i in recs:
        assert int(rf["count"][i]) == int(d["refined_bits"][i].sum())
        assert int(rf["ok"][i]) == int(rf["count"][i] > min_inliers)
    want, inl = R.select(counts, d["R"], d["t"], d["bits"], rf["valid"], rf["count"], rf["ok"],
                         rf["hyp"]["R"].reshape(-1, 3, 3), rf["hyp"]["t"], d["refined_bits"],
                         scene["index"], scene["n1"], min_inliers, n)
    res = d["result"]
    for k in ("hit_iter", "best_iter", "ninliers", "nomore", "refined"):
        assert int(res[k]) == int(want[k]), k
    assert res["Tcw"].tobytes() == want["Tcw"].tobytes()
    assert np.array_equal(d["inliers"], inl)
    for Rs in (d["R"], rf["hyp"]["R"].reshape(-1, 3, 3)):
        assert np.isfinite(Rs).all()
        live = np.abs(Rs).sum((1, 2)) > 0
        if live.any():
            assert np.abs(np.einsum("kji,kjl->kil", Rs[live], Rs[live]) - np.eye(3)).max() <= 1e-9
            assert np.abs(np.linalg.det(Rs[live]) - 1.0).max() <= 1e-9
    assert np.isfinite(d["t"]).all() and np.isfinite(rf["hyp"]["t"]).all()


def masks_agree(bits, R_, t_, scene, band):
    """bits [n] against NumPy's CheckInliers of pose (R_, t_), outside the band"""
    th = R.max_error(scene["sigma2"])
    want, e2 = R.check_inliers(R_, t_, scene["Xw"], scene["uv"], th, scene["K"])
    skip = R.in_band(e2, th, band)
    assert np.array_equal(bits[~skip], want[~skip])
    return int(skip.sum())


# ---- 1. own outputs, exact ----
@pytest.mark.parametrize("name", list(R.CASES))
def test_own_outputs_are_exact(P, L, name):
    scene, samples, mi, its, d = solve_case(P, name)
    check_own_outputs(L, scene, mi, d)
    print(name, "counts max", int(d["counts"].max()), "records", np.flatnonzero(d["refines"]["valid"]).tolist(),
          "hit", int(d["result"]["hit_iter"]))


# ---- 2. masks from the device's own hypotheses ----
@pytest.mark.parametrize("name", R.MIN_SET_4)
def test_masks_follow_the_devices_own_hypotheses(P, name):
    scene, samples, mi, its, d = solve_case(P, name)
    skipped = 0
    for i in range(its):
        if np.abs(d["R"][i]).sum() == 0:
            assert d["counts"][i] == 0 and not d["bits"][i].any()
            continue
        skipped += masks_agree(d["bits"][i], d["R"][i], d["t"][i], scene, R.BAND_OWN)
        assert d["counts"][i] == d["bits"][i].sum()
    print(name, "decisions in the band", skipped)
    assert skipped <= R.MAX_BAND * its * scene["n"]


# ---- 3. well-posed hypotheses against the reference ----
@pytest.mark.parametrize("name", R.WELL_POSED)
def test_well_posed_hypotheses_against_the_reference(P, name):
    scene, samples, mi, its, d = solve_case(P, name)
    ref, again = R.reference(name)
    ill = R.ill_conditioned(ref, again)
    assert ill.mean() <= R.MAX_ILL
    worst = (0.0, 0.0)
    th = ref["ev"]["th"]
    for i in np.flatnonzero(~ill):
        dR, dt = R.pose_delta(d["R"][i], d["t"][i], ref["ev"]["R"][i], ref["ev"]["t"][i])
        worst = (max(worst[0], dR), max(worst[1], dt))
        skip = R.in_band(ref["ev"]["err2"][i], th, R.BAND_REF)
        assert np.array_equal(d["bits"][i][~skip], ref["ev"]["masks"][i][~skip]), i
    print(name, "max|dR| %.3g |dt| %.3g over %d iterations" % (worst + (int((~ill).sum()),)))
    assert worst[0] <= R.POSE_TOL and worst[1] <= R.POSE_TOL
    assert R.hit_is_determined(ref, again, mi)   # test_pnp_ref.py asserts this premise too
    assert int(d["result"]["hit_iter"]) == ref["result"]["hit_iter"]
    assert int(d["result"]["ninliers"]) == ref["result"]["ninliers"]


# ---- 4. Refine ----
@pytest.mark.parametrize("name", list(R.CASES))
def test_refine_against_the_reference_on_the_devices_best_set(P, name):
    scene, samples, mi, its, d = solve_case(P, name)
    rf = d["refines"]
    worst = (0.0, 0.0)
    for i in np.flatnonzero(rf["valid"]):
        assert d["bits"][i].sum() >= 10       # EPnP on that many points is well posed
        Rr, tr, mr, e2 = R.refine(scene, d["bits"][i])
        Rd, td = rf["hyp"]["R"][i].reshape(3, 3), rf["hyp"]["t"][i]
        dR, dt = R.pose_delta(Rd, td, Rr, tr)
        worst = (max(worst[0], dR), max(worst[1], dt))
        masks_agree(d["refined_bits"][i], Rd, td, scene, R.BAND_OWN)
        skip = R.in_band(e2, R.max_error(scene["sigma2"]), R.BAND_REF)
        assert np.array_equal(d["refined_bits"][i][~skip], mr[~skip])
        if not skip.any():
            assert int(rf["count"][i]) == int(mr.sum()) and bool(rf["ok"][i]) == bool(mr.sum() > mi)
    print(name, "refines", int(rf["valid"].sum()), "max|dR| %.3g |dt| %.3g" % worst)
    assert worst[0] <= R.POSE_TOL and worst[1] <= R.POSE_TOL


# ---- 5. statistical, min_set = 4 ----
def test_min_set_4_succeeds_as_often_as_the_reference(P):
    n_ref, share_ref = R.stat_reference_share()
    tot, good = 0, 0.0
    for scene, samples, mi in R.stat_scenes():
        d = device_solve(P, scene, samples, mi, R.STAT_ITERATIONS)
        k, share = R.success_share(scene, samples, mi, counts=d["counts"])
        tot, good = tot + k, good + share * k
        want, _ = R.solve_until_hit(scene, samples, mi)
        assert want is not None and int(d["result"]["hit_iter"]) >= 0
        err_dev, err_ref = R.pose_error(d["result"]["Tcw"], scene), R.pose_error(want, scene)
        print("pose error device %.3g reference %.3g" % (err_dev, err_ref))
        assert err_dev <= max(3.0 * err_ref, 1e-5)
    print("all-inlier samples", tot, "device share %.3f reference share %.3f" % (good / tot, share_ref))
    assert tot == n_ref and good / tot >= share_ref - R.STAT_MARGIN


# ---- 6. rule edges ----
def test_fewer_correspondences_than_min_inliers(P, L):
    from orb_slam2_test_amd import synthetic
    scene = synthetic.pnp_scene(seed=31, n=9, inliers=9)
    mi, its = R.ransac_parameters(0.99, 10, 300, 4, 0.5, 9)
    assert mi == 10
    d = device_solve(P, scene, np.zeros((0, 4), np.int32), mi, 7)
    res = d["result"]
    assert (int(res["hit_iter"]), int(res["best_iter"]), int(res["ninliers"]), int(res["nomore"])) == \
        (-1, -1, 0, 1)
    assert not d["counts"].any() and not d["hyps"]["R"].any() and not d["inliers"].any()
    assert res["Tcw"].tobytes() == bytes(48)


def test_n_equal_to_min_inliers_runs_one_iteration(P, L):
    from orb_slam2_test_amd import synthetic
    scene = synthetic.pnp_scene(seed=32, n=10, inliers=10)
    mi, its = P.ransac_parameters(0.99, 10, 300, 4, 0.5, 10)
    assert (mi, its) == (10, 1)
    samples = R.draw_samples_literal(10, 1, 6, R.rand_stream(33, 6))
    d = device_solve(P, scene, samples, mi, its)
    check_own_outputs(L, scene, mi, d)
    assert len(d["counts"]) == 1 and d["counts"][0] == 10
    # a record, but Refine's 10 is not > 10: the unrefined best comes back
    res = d["result"]
    assert (int(res["hit_iter"]), int(res["best_iter"]), int(res["refined"]), int(res["nomore"])) == \
        (-1, 0, 0, 1)


def test_all_outliers_give_no_record(P, L):
    from orb_slam2_test_amd import synthetic
    scene = synthetic.pnp_scene(seed=34, n=40, inliers=0)
    mi, _ = R.ransac_parameters(0.99, 10, 300, 4, 0.5, 40)
    samples = R.draw_samples_literal(40, 64, 4, R.rand_stream(35, 256))
    d = device_solve(P, scene, samples, mi, 64)
    check_own_outputs(L, scene, mi, d)
    res = d["result"]
    assert d["counts"].max() < mi and not d["refines"]["valid"].any()
    assert (int(res["hit_iter"]), int(res["best_iter"]), int(res["ninliers"]), int(res["nomore"])) == \
        (-1, -1, 0, 1)
    assert res["Tcw"].tobytes() == bytes(48) and not d["inliers"].any()


def test_exactly_min_inliers_true_inliers_return_the_unrefined_best(P, L):
    from orb_slam2_test_amd import synthetic
    scene = synthetic.pnp_scene(seed=36, n=40, inliers=20)
    mi, _ = R.ransac_parameters(0.99, 10, 300, 4, 0.5, 40)
    assert mi == 20
    # half of the samples come from the true inliers alone (6 points: well posed), so a
    # hypothesis with all 20 exists whatever the implementation
    samples = R.draw_samples_literal(40, 64, 6, R.rand_stream(37, 64 * 6))
    good = np.flatnonzero(~scene["outlier"])
    samples[1::2] = good[R.draw_samples_literal(20, 32, 6, R.rand_stream(38, 32 * 6))]
    d = device_solve(P, scene, samples, mi, 64)
    check_own_outputs(L, scene, mi, d)
    rf, res = d["refines"], d["result"]
    assert d["counts"].max() == 20 and rf["valid"].any()
    assert not rf["ok"].any() and (rf["count"][rf["valid"] != 0] <= mi).all()
    assert (int(res["hit_iter"]), int(res["refined"]), int(res["nomore"]), int(res["ninliers"])) == \
        (-1, 0, 1, 20)
    assert int(res["best_iter"]) == int(np.argmax(d["counts"]))
    assert np.array_equal(d["inliers"].astype(bool)[scene["index"]], ~scene["outlier"])


def test_host_call_rejects_bad_input(P, L):
    scene, samples, mi, its = R.case("n40_s4")
    p, c = records(P, scene, 4, mi, 8)

    def rc(prob=p, corrs=c, smp=samples[:8], n1=scene["n1"]):
        with pytest.raises(L.OrbgError) as e:
            P.solve(prob, corrs, smp, n1)
        return e.value.code

    s = samples[:8].copy()
    s[3, 1] = 40
    assert rc(smp=s) == L.ORBG_EINVAL            # outside [0, n)
    s = samples[:8].copy()
    s[5, 2] = s[5, 0]
    assert rc(smp=s) == L.ORBG_EINVAL            # repeated within the sample
    for m in (3, 9):
        q = p.copy()
        q["min_set"] = m
        assert rc(prob=q, smp=np.zeros((8, m), np.int32)) == L.ORBG_EINVAL
    assert rc(n1=39) == L.ORBG_EINVAL            # an index outside [0, n1)
    big = P.make_problem(scene["K"], 8193, 4, mi, 1, R.TH2)
    assert rc(prob=big, corrs=np.zeros(8193, L.PNP_CORR_DTYPE), smp=np.zeros((1, 4), np.int32),
              n1=1) == L.ORBG_ENOTSUP


# ---- 7. batch ----
def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _batch(P, L, cands, cap, max_its, n1cap):
    """cands: [(scene, samples, min_inliers, iterations)] -> two runs of the batch call as numpy"""
    import torch
    from orb_slam2_test_amd.orbmatcher import _ctx
    N = len(cands)
    probs = np.zeros(N, L.PNP_PROBLEM_DTYPE)
    corrs = np.zeros((N, cap), L.PNP_CORR_DTYPE)
    smp = np.zeros((N, max_its, L.PNP_MAX_SET), np.int32)
    for k, (scene, samples, mi, its) in enumerate(cands):
        p, c = records(P, scene, samples.shape[1], mi, its)
        probs[k], corrs[k, :scene["n"]] = p[0], c
        m = min(its, len(samples))
        smp[k, :m, :samples.shape[1]] = samples[:m]
    t = [_upload(probs), _upload(corrs), _upload(smp)]
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        out = P.solve_batch(t[0], t[1], t[2], N, cap, max_its, n1cap)
        _ctx(0).sync()
        runs.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    return runs


def test_batch_equals_single_candidate_calls_bit_for_bit(P, L):
    from orb_slam2_test_amd import synthetic
    names = ("n40_s4", "n65_s8_noise", "n100_s4", "n64_s6_noise", "n100_s6_sparse", "n40_s6_noise",
             "n65_s4")
    iters = (64, 40, 64, 17, 64, 1, 33)
    cands = []
    for name, its in zip(names, iters):
        scene, samples, mi, full = R.case(name)
        cands.append((scene, samples, mi, its))
    few = synthetic.pnp_scene(seed=31, n=9, inliers=9)           # n < min_inliers: nothing runs
    cands.append((few, np.zeros((0, 4), np.int32), 10, 7))
    cap, max_its, n1cap = 128, 64, 160
    first, second = _batch(P, L, cands, cap, max_its, n1cap)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k + " differs between two runs"
    words = first["masks"].view(np.uint64)
    rwords = first["refined_masks"].view(np.uint64)
    results = first["results"].reshape(-1).view(L.PNP_RESULT_DTYPE)
    refines = first["refines"].reshape(len(cands), max_its, -1).view(L.PNP_REFINE_DTYPE)[..., 0]
    hyps = first["hyps"]
    for k, (scene, samples, mi, its) in enumerate(cands):
        d = device_solve(P, scene, samples, mi, its)
        n, nw = scene["n"], (scene["n"] + 63) // 64
        assert np.array_equal(first["counts"][k, :its], d["counts"])
        assert hyps[k, :its].tobytes() == d["hyps"].tobytes()
        assert np.array_equal(words[k, :its, :nw], d["masks"])
        assert refines[k, :its].tobytes() == d["refines"].tobytes()
        assert np.array_equal(rwords[k, :its, :nw], d["refined_masks"])
        assert results[k].tobytes() == d["result"].tobytes()
        assert np.array_equal(first["inliers"][k, :scene["n1"]], d["inliers"])
        # iterations past the candidate's own and mask words past its n are zero
        assert not first["counts"][k, its:].any() and not hyps[k, its:].any()
        assert not words[k, its:].any() and not words[k, :, nw:].any()
        assert not rwords[k, its:].any() and not rwords[k, :, nw:].any()
        assert refines[k, its:].tobytes() == bytes((max_its - its) * L.PNP_REFINE_DTYPE.itemsize)
        assert not first["inliers"][k, scene["n1"]:].any()
        if n % 64:
            assert not (words[k, :, nw - 1] >> np.uint64(n % 64)).any()
            assert not (rwords[k, :, nw - 1] >> np.uint64(n % 64)).any()


def test_device_form_counts_a_bad_sample_as_degenerate(P, L):
    scene, samples, mi, its = R.case("n64_s6_noise")
    clean = device_solve(P, scene, samples, mi, 16)
    s = samples[:16].copy()
    s[2, 3], s[3, 5], s[9, 0] = s[2, 0], 64, -1
    got = _batch(P, L, [(scene, s, mi, 16)], 64, 16, 64)[0]
    bad = np.zeros(16, bool)
    bad[[2, 3, 9]] = True
    assert not got["counts"][0, bad].any() and not got["masks"][0, bad].any()
    assert not got["hyps"][0, bad].any()
    assert np.array_equal(got["counts"][0, ~bad], clean["counts"][~bad])
    assert got["hyps"][0, ~bad].tobytes() == clean["hyps"][~bad].tobytes()
    assert np.array_equal(got["masks"].view(np.uint64)[0, ~bad], clean["masks"][~bad])


# ---- the class ----
def test_iterate_in_windows_follows_the_rule(P):
    """PnPsolver.iterate(5) as Tracking calls it: the OR in the reference's loop condition makes
    the first call run to mRansacMaxIts unless it hits; after a hit the next call hits again at
    the next iteration with count >= min_inliers, on the unchanged best set."""
    scene, samples, mi, its = R.case("n40_s6_noise")
    solver = P.PnPsolver(scene["K"], scene["Xw"], scene["uv"], scene["sigma2"], scene["index"],
                         scene["n1"], stream=R.rand_stream(18 + 1000, 6 * 300))
    solver.SetRansacParameters(0.99, 10, 300, 6, 0.5, R.TH2)
    assert solver.mRansacMinInliers == mi
    n_its = solver.mRansacMaxIts
    T, nomore, inl, ninl = solver.iterate(5)
    d = solver._eval
    assert np.array_equal(solver.samples[:min(n_its, its)], samples[:min(n_its, its)])
    res = solver.result
    hit = int(res["hit_iter"])
    assert hit >= 0 and not nomore and solver.mnIterations == hit + 1
    assert T[:3].astype(np.float32).tobytes() == res["Tcw"].tobytes() and ninl == int(res["ninliers"])
    assert np.array_equal(inl, solver.inliers.astype(bool))
    nxt, best = -1, int(res["best_iter"])
    for i in range(hit + 1, n_its):
        if d["counts"][i] >= mi:
            if d["refines"]["valid"][i]:
                best = i
            if d["refines"]["ok"][best]:
                nxt = i
                break
    T2, nomore2, inl2, ninl2 = solver.iterate(5)
    if nxt >= 0:
        assert solver.mnIterations == nxt + 1 and not nomore2 and T2 is not None
        assert ninl2 == int(d["refines"]["count"][best])
    else:
        assert nomore2 and solver.mnIterations == n_its
