"""GPU: the device Initializer (csrc/init_kernels.hip behind orbg_initialize and
orbg_initialize_batch_device, and the Python class on top) against the float64 reference of
tests/ref_initializer.py.  The rules themselves are in tests/init_checks.py, which
tests/test_initializer_ref.py also applies to the one-core host program.

What the device derives from its own per-iteration outputs (the best iterations, SH, SF, RH,
the model, the decision from its counts and parallaxes, R21, t21, the zeroed outputs) is
checked exactly, on every case.  Masks and scores are checked against NumPy's CheckHomography /
CheckFundamental on the device's own float matrices.  Hypotheses are compared with the
reference iteration by iteration within ref_initializer.DEVICE_TOL, results on the cases
tests/test_initializer_ref.py shows to be determined.

Hypothesis indices are not compared with the reference: which index holds which motion follows
the sign of the null vector (and, for DecomposeE, the pairing of two nearly equal singular
values), which no two SVD routines share.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_initializer as R  # noqa: E402
import init_checks as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I():
    from orb_slam2_test_amd import initializer
    return initializer


@pytest.fixture(scope="module")
def L():
    from orb_slam2_test_amd import _lib
    return _lib


_runs = {}


def device_run(I, name):
    if name not in _runs:
        sc, sets, its = R.case(name)
        _runs[name] = I.initialize(K.problem_of(I, sc, its), sc["keys1"], sc["keys2"],
                                   sc["matches12"], sets)
    return _runs[name]


@pytest.mark.parametrize("name", K.ALL_CASES)
def test_own_outputs_masks_and_scores(I, name):
    sc, sets, its = R.case(name)
    d = device_run(I, name)
    K.check_own_outputs(I, sc, its, d)
    share, skipped = K.check_masks_and_scores(I, sc, its, d)
    print(name, "share of decisions in the band", share, "H iterations skipped", skipped)
    assert share <= R.MAX_BAND and skipped <= K.MAX_SKIP_H12


@pytest.mark.parametrize("name", list(K.HYP_CASES))
def test_hypotheses_against_the_reference(I, name):
    worst, ill = K.check_hypotheses(name, device_run(I, name), K.HYP_CASES[name])
    print(name, "worst distance", worst, "tolerance", R.DEVICE_TOL, "skipped", ill)
    assert ill <= R.MAX_ILL


@pytest.mark.parametrize("name", K.RESULT_CASES)
def test_results_against_the_reference(I, name):
    print(name, K.check_results(name, device_run(I, name)))


@pytest.mark.parametrize("name", K.PARALLAX_CASES)
def test_parallax_against_the_reference(I, name):
    print(name, "worst share of the tolerance", K.check_parallax(name, device_run(I, name)))


def test_device_records_equal_the_host_program(I, L):
    """lib/init_host runs the kernels' statements on one core in the kernels' summation orders:
    every output of every case is the same, byte for byte.  That holds the kernel-only code (the
    compaction, the reductions, the ballots, the selection of the order statistic by bisection)
    to what tests/test_initializer_ref.py checks of the host program."""
    for name in K.ALL_CASES:
        sc, sets, its = R.case(name)
        dev, host = device_run(I, name), K.host_single(I, L, sc, sets, its)
        for k in dev:
            assert dev[k].tobytes() == host[k].tobytes(), (name, k)


def test_far_points_are_counted_but_not_triangulated(I):
    d = device_run(I, "far")
    r = d["result"]
    assert r["success"] == 1 and r["ngood"][r["hyp"]] - r["ntriangulated"] == 8
    assert int(d["p3d"].any(1).sum()) - int(d["triangulated"].sum()) == 8


def test_edge_cases(I):
    for name in ("n7", "n0"):    # N < 8 runs nothing
        d = device_run(I, name)
        r = d["result"]
        assert r["n"] == int(name[1:]) and r["model"] == 0 and r["success"] == 0
        assert r["best_h"] == -1 and r["best_f"] == -1
        for k in ("scores_h", "scores_f", "H21", "F21", "p3d", "triangulated"):
            assert not d[k].any(), (name, k)
    d = device_run(I, "rotation")   # a pure rotation is refused, with zeroed outputs
    assert d["result"]["success"] == 0 and d["result"]["model"] in (1, 2)
    assert not d["p3d"].any() and not d["triangulated"].any() and not d["result"]["R21"].any()
    few, some = device_run(I, "few")["result"], device_run(I, "some")["result"]
    assert 0 < few["ngood"].max() <= 50       # the order statistic takes size - 1
    assert some["ngood"].max() >= 52          # ... and index 50
    # a set with a repeated index or one out of range scores nothing; the others are untouched
    sc, sets, its = R.bad_sets_case()
    bad = I.initialize(K.problem_of(I, sc, its), sc["keys1"], sc["keys2"], sc["matches12"], sets)
    K.check_own_outputs(I, sc, its, bad)
    good = device_run(I, "n64")
    for it in (3, 5, 6):
        assert not bad["H21"][it].any() and not bad["F21"][it].any()
        assert bad["scores_h"][it] == 0 and bad["scores_f"][it] == 0
        assert not bad["masks_h"][it].any() and not bad["masks_f"][it].any()
        assert good["F21"][it].any()
    keep = [i for i in range(its) if i not in (3, 5, 6)]
    for k in ("H21", "F21", "scores_h", "scores_f", "masks_h", "masks_f"):
        assert np.array_equal(bad[k][keep], good[k][keep]), k


def test_matches_past_n2_are_no_matches(I):
    sc, sets, its = R.case("n65")
    m = sc["matches12"].copy()
    drop = np.flatnonzero(m >= 0)[:3]
    far = m.copy()
    far[drop] = len(sc["keys2"]) + np.arange(3)
    m[drop] = -1
    n = int((m >= 0).sum())
    s = I.draw_sets(n, its, R.rand_stream(77, its * 8))
    a = I.initialize(K.problem_of(I, sc, its), sc["keys1"], sc["keys2"], m, s)
    b = I.initialize(K.problem_of(I, sc, its), sc["keys1"], sc["keys2"], far, s)
    assert a["result"]["n"] == n == 62
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _batch(I, L, names, order, cap):
    import torch
    cases = [R.case(names[i]) for i in order]
    probs, kps, counts, f1, f2, m12, sets = K.batch_arrays(I, L, cases, cap)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (probs, kps, counts, f1, f2, m12, sets)]
    torch.cuda.synchronize()   # the uploads (torch's stream) before the kernels (context stream)
    from orb_slam2_test_amd.orbmatcher import _ctx
    out = I.initialize_batch(dev[0], dev[1], kps.shape[1], dev[2], len(counts), dev[3], dev[4],
                             dev[5], dev[6], len(cases), cap, sets.shape[1])
    _ctx(0).sync()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["results"] = host["results"].view(L.INIT_RESULT_DTYPE).reshape(-1)
    return cases, host


def test_batch_equals_single_in_any_position(I, L):
    names = ("n64", "n7", "some")     # three pairs of different N, one below 8, cap = 128
    first = None
    for order in ((0, 1, 2), (2, 0, 1), (0, 1, 2)):
        cases, out = _batch(I, L, names, order, 128)
        for p, i in enumerate(order):
            sc, sets, its = cases[p]
            one, got = device_run(I, names[i]), K.single_of(out, p, sc, its)
            for k in one:
                assert one[k].tobytes() == got[k].tobytes(), (names[i], order, k)
            n1 = len(sc["keys1"])
            assert not out["p3d"][p, n1:].any() and not out["triangulated"][p, n1:].any()
            assert not out["scores_h"][p, its:].any() and not out["H21"][p, its:].any()
            N = int(out["results"][p]["n"])
            assert not out["masks_f"][p, :, (N + 63) // 64:].any()
        if order == (0, 1, 2):     # two runs give identical bytes
            if first is None:
                first = out
            else:
                for k in out:
                    assert first[k].tobytes() == out[k].tobytes(), k


def test_optional_outputs_may_be_left_out(I, L):
    import torch
    from orb_slam2_test_amd.orbmatcher import _ctx
    cases = [R.case("some")]
    probs, kps, counts, f1, f2, m12, sets = K.batch_arrays(I, L, cases, 128)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (probs, kps, counts, f1, f2, m12, sets)]
    torch.cuda.synchronize()
    out = I.initialize_batch(dev[0], dev[1], kps.shape[1], dev[2], 2, dev[3], dev[4], dev[5], dev[6],
                             1, 128, sets.shape[1], details=False)
    _ctx(0).sync()
    one = device_run(I, "some")
    assert out["results"].cpu().numpy().view(L.INIT_RESULT_DTYPE)[0].tobytes() == one["result"].tobytes()
    n1 = len(cases[0][0]["keys1"])
    assert np.array_equal(out["p3d"].cpu().numpy()[0, :n1], one["p3d"])


def test_device_resident_chain(I, L):
    """extract -> SearchForInitialization -> Initialize with nothing going through the host:
    the batched entry straight on the extractor's and the matcher's device arrays equals the
    host-array call on the downloaded arrays, byte for byte."""
    import torch
    from orb_slam2_test_amd import ORBextractor, synthetic
    h, w, its = 480, 640, 64
    frames = synthetic.sequence(2, h, w, seed=synthetic.DEFAULT_SEED + 31)
    d = torch.from_numpy(frames).cuda()
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=2)
    ext.extract_batch_device(d.data_ptr(), 2, w, h)
    ext.match_batch_device([0], [1], 100, 0.9, True)
    ext.ctx.sync()   # the match stream's writes before the context stream's reads
    d_kps, _, d_counts, frame_cap = ext.batch_outputs()
    _, d_m12, _, mcap = ext.match_outputs()
    assert mcap == frame_cap
    ka, _ = ext.download_frame(0)
    kb, _ = ext.download_frame(1)
    _, m12, nm = ext.download_matches(0, len(ka))
    assert nm >= 8 and len(ka) <= L.INIT_MAX_N
    cap = min((frame_cap + 63) // 64 * 64, L.INIT_MAX_N)
    sets = I.draw_sets(nm, its, R.rand_stream(5, its * 8))
    prob = I.make_problem((517.3, 516.5, 318.6, 255.3), 1.0, its)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (prob, np.zeros(1, np.int32), np.ones(1, np.int32), sets)]
    torch.cuda.synchronize()
    out = I.initialize_batch(dev[0], d_kps, frame_cap, d_counts, 2, dev[1], dev[2], d_m12, dev[3],
                             1, cap, its, match_stride=frame_cap, ctx=ext.ctx)
    ext.ctx.sync()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["results"] = host["results"].view(L.INIT_RESULT_DTYPE).reshape(-1)
    sc = {"keys1": ka, "keys2": kb}
    got = K.single_of(host, 0, sc, its)
    one = I.initialize(prob, ka, kb, m12, sets, ctx=ext.ctx)
    assert one["result"]["n"] == nm
    for k in one:
        assert one[k].tobytes() == got[k].tobytes(), k
    assert not host["p3d"][0, len(ka):].any() and not host["triangulated"][0, len(ka):].any()
    ext.close()


def test_class_interface(I):
    sc, sets, its = R.case("general")
    init = I.Initializer(sc["keys1"], sc["K"], sigma=1.0, iterations=its, stream=R.rand_stream(2, its * 8))
    ok, R21, t21, p3d, tri = init.Initialize(sc["keys2"], sc["matches12"])
    assert np.array_equal(init.mvSets, sets)
    d = device_run(I, "general")
    assert ok and np.array_equal(R21.reshape(9), d["result"]["R21"]) and np.array_equal(t21, d["result"]["t21"])
    assert np.array_equal(p3d, d["p3d"]) and np.array_equal(tri, d["triangulated"].astype(bool))
    assert R.rotation_angle(R21, sc["R"]) < 1e-2 and R.direction_angle(t21, sc["t"]) < 0.125


def test_compat_init_selftest():
    exe = os.path.join(K.ROOT, "orb_slam2_test_amd", "lib", "compat_init_selftest")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
