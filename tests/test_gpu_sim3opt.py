"""GPU: the device Optimizer::OptimizeSim3 (csrc/sim3opt_kernels.hip behind
orbg_optimize_sim3 and orbg_optimize_sim3_batch_device, and the Python functions on top)
against the float64 reference of tests/ref_sim3opt.py with g2o's numeric Jacobian, by the
comparison rule stated there (ref_sim3opt.compare): keep flags equal except on pairs within
CLOSE of th2, counts equal up to those, the estimate within SIM3_TOL and its robust cost on the
kept pairs no more than SIM3_TOL above the reference's.  What is exact is checked exactly: the
float record is the double one rounded once, a fixed scale is untouched, the return-0 path
gives back the input, two runs and the two entry points agree bit for bit.

tests/test_sim3opt_ref.py holds the CPU side of the premises.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_sim3opt as R  # noqa: E402
from test_sim3opt_ref import RETURN0, as_got, records  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(R.CASES)


@pytest.fixture(scope="module")
def O():
    from orb_slam2_test_amd import optimizer
    return optimizer


@pytest.fixture(scope="module")
def L():
    from orb_slam2_test_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def single(O):
    """name -> (result record, keep uint8 [n1]) of the single-entry call, run once."""
    out = {}
    for k in NAMES:
        sc = R.case(k)[0]
        out[k] = O.optimize_sim3(*records(sc), sc["n1"])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_case_against_the_numeric_reference(single, name):
    sc, ref = R.case(name)
    r, keep = single[name]
    assert set(np.unique(keep)) <= {0, 1}
    fig = R.compare(sc, ref, as_got(r, keep))
    print(name, fig, "iterations", r["iterations"].tolist(), [len(t) for t in ref["trace"]])
    # the float record: toRotationMatrix of q, t and s, each rounded once
    assert np.array_equal(r["R"].reshape(3, 3), R.rot_of_quat(r["q"]).astype(np.float32))
    assert np.array_equal(r["tf"], r["t"].astype(np.float32))
    assert r["sf"] == np.float32(r["s"])
    if sc["fix_scale"]:
        assert float(r["s"]) == float(sc["s12"])     # bit for bit: the float input widened
    assert 0 <= r["iterations"][0] <= 5 and 0 <= r["iterations"][1] <= 10
    assert (r["iterations"][0] > 0) == (sc["n"] > 0)


@pytest.mark.parametrize("name", RETURN0)
def test_return_zero_path_gives_back_the_input(O, single, name):
    sc, ref = R.case(name)
    r, _ = single[name]
    r0, keep0 = O.optimize_sim3(*records(sc, n=0), sc["n1"])
    assert r["ninliers"] == 0 and r["nbad"] == ref["nBad"] and r["iterations"][1] == 0
    for f in ("q", "t", "s", "R", "tf", "sf"):
        assert r[f].tobytes() == r0[f].tobytes(), f
    assert not keep0.any() and r0["ncorr"] == 0 and r0["nbad"] == 0
    q, t, s = R.sim3_from_float(sc["R12"], sc["t12"], sc["s12"])
    assert np.abs(r0["q"] - q).max() <= R.INIT_Q_BOUND
    assert np.array_equal(r0["t"], t) and float(r0["s"]) == s


def test_two_identical_calls_return_identical_bytes(O, single):
    for name in ("n300", "far_init"):
        sc = R.case(name)[0]
        r, keep = O.optimize_sim3(*records(sc), sc["n1"])
        assert r.tobytes() == single[name][0].tobytes()
        assert keep.tobytes() == single[name][1].tobytes()


def test_batch_equals_the_single_entry_bit_for_bit(O, L, single):
    import torch
    from orb_slam2_test_amd.orbmatcher import _ctx
    recs = [records(R.case(k)[0]) for k in NAMES]
    nmax = max(len(c) for _, c, _ in recs)
    cap = (nmax + 63) // 64 * 64 + 64            # a multiple of 64 above the largest n
    n1cap = max(R.case(k)[0]["n1"] for k in NAMES) + 5
    P = len(NAMES)
    corrs = np.zeros((P, cap), L.SIM3OPT_CORR_DTYPE)
    corrs["index1"] = -1                          # slots past a candidate's n are never read
    for i, (_, c, _) in enumerate(recs):
        corrs[i, :len(c)] = c

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_p = up(np.concatenate([p for p, _, _ in recs]))
    d_c = up(corrs)
    d_h = up(np.concatenate([h for _, _, h in recs]))
    tail = 64
    d_r = torch.zeros(P * L.SIM3OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_k = torch.full((P * n1cap + tail,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx = _ctx(0)
    L.check(L.lib().orbg_optimize_sim3_batch_device(ctx.handle, d_p.data_ptr(), d_c.data_ptr(),
                                                    d_h.data_ptr(), P, cap, d_r.data_ptr(),
                                                    d_k.data_ptr(), n1cap), "batch")
    ctx.sync()
    res = d_r.cpu().numpy().view(L.SIM3OPT_RESULT_DTYPE)
    kraw = d_k.cpu().numpy()
    assert (kraw[P * n1cap:] == 0xAB).all()       # nothing past the array
    keep = kraw[:P * n1cap].reshape(P, n1cap)
    assert set(np.unique(keep)) <= {0, 1}
    for i, k in enumerate(NAMES):
        n1 = R.case(k)[0]["n1"]
        assert res[i].tobytes() == single[k][0].tobytes(), k
        assert keep[i, :n1].tobytes() == single[k][1].tobytes(), k
        assert not keep[i, n1:].any()             # slots no correspondence names are 0
    # a count outside [0, cap] runs nothing: the record of n = 0
    bad = np.concatenate([p for p, _, _ in recs])
    bad["n"][NAMES.index("n300")] = cap + 1
    d_k.fill_(0xAB)
    L.check(L.lib().orbg_optimize_sim3_batch_device(ctx.handle, up(bad).data_ptr(), d_c.data_ptr(),
                                                    d_h.data_ptr(), P, cap, d_r.data_ptr(),
                                                    d_k.data_ptr(), n1cap), "batch")
    ctx.sync()
    r = d_r.cpu().numpy().view(L.SIM3OPT_RESULT_DTYPE)[NAMES.index("n300")]
    assert r["ncorr"] == 0 and r["ninliers"] == 0 and r["iterations"].tolist() == [0, 0]
    assert not d_k.cpu().numpy()[:P * n1cap].reshape(P, n1cap)[NAMES.index("n300")].any()


def test_host_keep_past_n1_keeps_its_sentinel(L):
    from orb_slam2_test_amd.orbmatcher import _ctx
    sc = R.case("n40_out8")[0]
    p, c, h = records(sc)
    r = np.zeros(1, L.SIM3OPT_RESULT_DTYPE)
    keep = np.full(sc["n1"] + 16, 0xAB, np.uint8)
    L.check(L.lib().orbg_optimize_sim3(_ctx(0).handle, L.ptr(p), L.ptr(c), L.ptr(h), sc["n1"],
                                       L.ptr(r), L.ptr(keep)), "orbg_optimize_sim3")
    assert (keep[sc["n1"]:] == 0xAB).all() and set(np.unique(keep[:sc["n1"]])) <= {0, 1}


def test_public_functions(single):
    import orb_slam2_test_amd as pkg
    names = ["n40_out8", "n0", "n9", "two_cameras"]
    args = []
    for k in names:
        sc = R.case(k)[0]
        args.append({f: sc[f] for f in ("T1w", "T2w", "K1", "K2", "Xw1", "Xw2", "obs1", "obs2",
                                        "inv_sigma2_1", "inv_sigma2_2", "index1", "n1", "R12",
                                        "t12", "s12", "th2")})
        args[-1]["bFixScale"] = sc["fix_scale"]
    sc = R.case(names[0])[0]
    a = args[0]
    nIn, (q, t, s), keep = pkg.OptimizeSim3(a["T1w"], a["T2w"], a["K1"], a["K2"], a["Xw1"], a["Xw2"],
                                            a["obs1"], a["obs2"], a["inv_sigma2_1"],
                                            a["inv_sigma2_2"], a["index1"], a["n1"], a["R12"],
                                            a["t12"], a["s12"], a["th2"], a["bFixScale"])
    r, k1 = single[names[0]]
    assert nIn == r["ninliers"] and np.array_equal(q, r["q"]) and np.array_equal(t, r["t"])
    assert s == float(r["s"]) and keep.dtype == bool and np.array_equal(keep, k1.astype(bool))
    out = pkg.OptimizeSim3Batch(args)
    for (nIn, (q, t, s), keep), k in zip(out, names):
        r, k1 = single[k]
        assert nIn == r["ninliers"] and np.array_equal(q, r["q"]) and s == float(r["s"])
        assert np.array_equal(keep, k1.astype(bool))


def test_errors_are_reported_without_a_launch(L):
    from orb_slam2_test_amd.orbmatcher import _ctx
    h = _ctx(0).handle
    sc = R.case("n40")[0]
    p, c, hyp = records(sc)

    def call(p, c, n1):
        r = np.full(1, 0, L.SIM3OPT_RESULT_DTYPE)
        r.view(np.uint8)[:] = 0xCD
        keep = np.full(max(n1, 1), 0xAB, np.uint8)
        rc = L.lib().orbg_optimize_sim3(h, L.ptr(p), L.ptr(c), L.ptr(hyp), n1, L.ptr(r), L.ptr(keep))
        assert (r.view(np.uint8) == 0xCD).all() and (keep == 0xAB).all()   # nothing came back
        return rc
    c2 = c.copy()
    c2["index1"][3] = sc["n1"]
    assert call(p, c2, sc["n1"]) == L.ORBG_EINVAL
    c2["index1"][3] = -1
    assert call(p, c2, sc["n1"]) == L.ORBG_EINVAL
    for th2 in (0.0, -1.0, np.inf, np.nan):
        p2 = p.copy()
        p2["th2"] = th2
        assert call(p2, c, sc["n1"]) == L.ORBG_EINVAL
    big = np.zeros(8193, L.SIM3OPT_CORR_DTYPE)
    p3 = p.copy()
    p3["n"] = 8193
    assert call(p3, big, 8193) == L.ORBG_ENOTSUP
    assert L.lib().orbg_optimize_sim3_batch_device(h, 1, 1, 1, 1, 8192 + 64, 1, 1, 1) == L.ORBG_ENOTSUP
    assert L.lib().orbg_optimize_sim3_batch_device(h, 1, 1, 1, 1, 100, 1, 1, 1) == L.ORBG_EINVAL
