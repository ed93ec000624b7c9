"""CPU: the independent statement of Optimizer::OptimizeSim3 (tests/ref_sim3opt.py) against
figures worked out by hand and against the definitions it rests on, the boundary of the library
without a GPU (the symbols include/orbg.h declares are exported and bound, the record sizes,
NULL arguments), and the premises of tests/test_gpu_sim3opt.py that need no GPU: on every case
the numeric- and analytic-Jacobian runs agree under the comparison rule, SIM3_TOL is what the
reference alone measures, and no decision the GPU test compares hinges on an ambiguous pair.

The kernel's arithmetic is a set of __host__ __device__ functions (csrc/sim3opt_args.h); the
one-core host program built from them (lib/sim3opt_host) is held to the same rule here.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_sim3opt as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["orbg_optimize_sim3", "orbg_optimize_sim3_batch_device"]
NO_OUTLIER = [k for k, v in R.CASES.items() if v.get("n_out", 0) == 0 and v["n"] > 0]
RETURN0 = ["n9", "n9_fs", "n10_out1", "n10_out1_fs", "mostly_outliers"]


@pytest.fixture(scope="module")
def lib():
    from orb_slam2_test_amd import _lib
    return _lib


def records(sc, n=None):
    from orb_slam2_test_amd import optimizer as O
    p, c, h = O.sim3opt_records(sc["T1w"], sc["T2w"], sc["K1"], sc["K2"], sc["Xw1"], sc["Xw2"],
                                sc["obs1"], sc["obs2"], sc["inv_sigma2_1"], sc["inv_sigma2_2"],
                                sc["index1"], sc["R12"], sc["t12"], sc["s12"], sc["th2"],
                                sc["fix_scale"])
    if n is not None:
        p["n"] = n
    return p, c, h


def as_got(r, keep):
    return dict(q=r["q"].copy(), t=r["t"].copy(), s=float(r["s"]), keep=np.asarray(keep, bool),
                nIn=int(r["ninliers"]), nBad=int(r["nbad"]), ncorr=int(r["ncorr"]))


# ---- the boundary ----
def test_symbols_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbg.h")).read(), flags=re.S)
    L = lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert hasattr(L, name), name + " is not exported"
        assert getattr(L, name).argtypes is not None, name + " is not bound"
    for struct in ("orbg_sim3opt_problem", "orbg_sim3opt_corr", "orbg_sim3opt_result"):
        assert re.search(r"\}\s*%s\s*;" % struct, text), struct
    assert L.orbg_abi_version() == 1


def test_record_sizes_match_the_header(lib):
    assert lib.SIM3OPT_PROBLEM_DTYPE.itemsize == (12 + 12 + 8) * 4 + 4 * 4
    assert lib.SIM3OPT_CORR_DTYPE.itemsize == (3 + 3 + 2 + 2 + 2) * 4 + 4
    assert lib.SIM3OPT_RESULT_DTYPE.itemsize == 8 * 8 + 13 * 4 + 5 * 4
    assert lib.SIM3OPT_RESULT_DTYPE.fields["R"][1] == 64      # no padding after the doubles


def test_optimize_sim3_is_exported_from_the_package():
    import orb_slam2_test_amd as pkg
    assert "OptimizeSim3" in pkg.__all__ and "OptimizeSim3Batch" in pkg.__all__
    assert pkg.OptimizeSim3.__module__ == "orb_slam2_test_amd.optimizer"
    assert callable(pkg.OptimizeSim3Batch)


def test_null_arguments_are_einval(lib):
    L = lib.lib()
    p = np.zeros(1, lib.SIM3OPT_PROBLEM_DTYPE)
    p["th2"] = 10
    h = np.zeros(1, lib.SIM3_HYP_DTYPE)
    r = np.zeros(1, lib.SIM3OPT_RESULT_DTYPE)
    assert L.orbg_optimize_sim3(None, lib.ptr(p), None, lib.ptr(h), 0, lib.ptr(r),
                                None) == lib.ORBG_EINVAL
    assert L.orbg_optimize_sim3(None, None, None, None, 0, None, None) == lib.ORBG_EINVAL
    assert L.orbg_optimize_sim3_batch_device(None, None, None, None, 1, 64, None, None,
                                             1) == lib.ORBG_EINVAL


# ---- the reference's premises ----
def _hand_scene():
    """Identity Sim3, f = 100, c = 0, one correspondence at (0.04, -0.08, 4) in both cameras:
    it projects to (1, -2); obs1 = (9, -14) so e12 = (8, -12), obs2 = (5, 1) so e21 = (4, 3);
    information 0.01: chi2 = 2.08 and 0.25, both below th2 = 10, so rho' = 1."""
    f = np.float32
    I34 = np.eye(4, dtype=f)
    X = np.array([[0.04, -0.08, 4.0]], f)
    return {"T1w": I34, "T2w": I34, "K1": (100, 100, 0, 0), "K2": (100, 100, 0, 0), "Xw1": X,
            "Xw2": X, "obs1": np.array([[9, -14]], f), "obs2": np.array([[5, 1]], f),
            "inv_sigma2_1": np.array([0.01], f), "inv_sigma2_2": np.array([0.01], f),
            "index1": np.array([0], np.int32), "n1": 1, "n": 1, "R12": np.eye(3, dtype=f),
            "t12": np.zeros(3, f), "s12": f(1), "th2": 10.0, "fix_scale": False}


def test_hand_worked_linearisation():
    sc = _hand_scene()
    pb = R.Problem(sc)
    S = R.sim3_from_float(sc["R12"], sc["t12"], sc["s12"])
    x, y, z = [float(v) for v in pb.P2c[0]]        # the float32 values of 0.04, -0.08, 4
    e12, e21 = R.errors(pb, S)
    assert np.allclose(e12, [[9 - 100 * x / z, -14 - 100 * y / z]], rtol=0, atol=1e-13)
    assert np.allclose(e21, [[5 - 100 * x / z, 1 - 100 * y / z]], rtol=0, atol=1e-13)
    # d pi = [[f / z, 0, -f x / z^2], [0, f / z, -f y / z^2]] = [[25, 0, -.25], [0, 25, .5]];
    # G(y) = [-[y]x, I, y]; d pi G: rows (0.02, 100.01, 2 | 25, 0, -.25 | 0) and
    # (-100.04, -0.02, 1 | 0, 25, .5 | 0); J12 = -d pi G, and at the identity J21 = +d pi G
    dpiG = np.array([[0.02, 100.01, 2, 25, 0, -0.25, 0], [-100.04, -0.02, 1, 0, 25, 0.5, 0]])
    J12, J21 = R.jacobians_analytic(pb, S)
    assert np.allclose(J12[0], -dpiG, rtol=0, atol=1e-5)    # 0.04 and 0.08 are float32 values
    assert np.allclose(J21[0], dpiG, rtol=0, atol=1e-5)
    # H = 0.01 (J12^T J12 + J21^T J21) = 0.02 (d pi G)^T (d pi G);
    # b = -0.01 (J12^T e12 + J21^T e21) = 0.01 (d pi G)^T (e12 - e21), e12 - e21 = (4, -15)
    H, b, F = R.linearize(pb, S, np.ones(1, bool), "analytic")
    assert np.allclose(H, 0.02 * dpiG.T @ dpiG, rtol=1e-5, atol=1e-6)
    assert np.allclose(b, 0.01 * dpiG.T @ np.array([4.0, -15.0]), rtol=1e-5, atol=1e-6)
    assert abs(F - 0.01 * (64 + 144 + 16 + 9)) < 1e-4
    # g2o's difference quotients: within |e| eps64 / delta of the derivative
    N12, N21 = R.jacobians_numeric(pb, S)
    for N, J, e in ((N12, J12, e12), (N21, J21, e21)):
        bound = float(np.linalg.norm(e)) * R.EPS64 / R.DELTA
        print("numeric - analytic %.3g (bound %.3g)" % (np.abs(N - J).max(), bound))
        assert np.abs(N - J).max() <= bound
    # under fix_scale the scale column is exactly zero
    sc["fix_scale"] = True
    N12, N21 = R.jacobians_numeric(R.Problem(sc), S)
    assert not N12[:, :, 6].any() and not N21[:, :, 6].any()


@pytest.mark.parametrize("theta,sigma", [(1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.4, -0.3)])
def test_exp_branches_against_the_series(theta, sigma):
    """Each of Sim3(Vector7d)'s four branches against the power series of the 4x4 generator.
    The two small-argument branches are truncations: below 1e-5 rad R = I + Omega + Omega^2
    errs by theta^2 / 2 and A, B are the limits (error ~ theta |upsilon|); below |sigma| = 1e-5
    C = 1 errs by sigma / 2 |upsilon|."""
    w = np.array([0.6, -0.48, 0.64]) * theta
    ups = np.array([0.3, -1.1, 0.7])
    q, t, s = R.sim3_exp(np.concatenate([w, ups, [sigma]]))
    Rs, ts, ss = R.sim3_exp_series(np.concatenate([w, ups, [sigma]]))
    small_t, small_s = theta < 1e-5, abs(sigma) < 1e-5
    tol_R = 1e-15 * 8 + (theta ** 2 if small_t else 0)
    tol_t = 1e-15 * 8 + ((theta if small_t else 0) + (abs(sigma) if small_s else 0)) * np.linalg.norm(ups)
    assert np.abs(R.rot_of_quat(q / np.linalg.norm(q)) - Rs).max() <= tol_R
    assert np.abs(t - ts).max() <= tol_t
    assert s == ss


def test_compose_and_inverse_round_trips():
    rng = np.random.default_rng(3)
    for _ in range(20):
        A = R.sim3_exp(np.concatenate([rng.normal(size=3) * 0.4, rng.normal(size=3), [rng.uniform(-0.5, 0.5)]]))
        B = R.sim3_exp(np.concatenate([rng.normal(size=3) * 0.4, rng.normal(size=3), [rng.uniform(-0.5, 0.5)]]))
        x = rng.normal(size=(5, 3)) * 3
        assert np.abs(R.sim3_map(R.sim3_inv(A), R.sim3_map(A, x)) - x).max() < 1e-13
        assert np.abs(R.sim3_map(R.sim3_mul(A, B), x) - R.sim3_map(A, R.sim3_map(B, x))).max() < 1e-13
        q, t, s = R.sim3_mul(A, R.sim3_inv(A))
        assert np.abs(q - [0, 0, 0, 1]).max() < 1e-14 and np.abs(t).max() < 1e-14 and abs(s - 1) < 1e-15


def test_initial_quaternion_is_eigens():
    sc, _ = R.case("n40")
    q, t, s = R.sim3_from_float(sc["R12"], sc["t12"], sc["s12"])
    R64 = sc["R12"].astype(np.float64)
    assert np.abs(R.rot_of_quat(q / np.linalg.norm(q)) - R64).max() < 1e-6   # a float32 rotation
    assert q[3] > 0 and np.array_equal(t, sc["t12"].astype(np.float64)) and s == float(sc["s12"])


# ---- the premises of the GPU test ----
@pytest.fixture(scope="module")
def variants():
    """Per case: the analytic-Jacobian run and the longdouble-error run."""
    return {k: (R.optimize_sim3(R.case(k)[0], "analytic"),
                R.optimize_sim3(R.case(k)[0], "numeric", np.longdouble)) for k in R.CASES}


def _as_got(o):
    return dict(q=o["q"], t=o["t"], s=o["s"], keep=o["keep"], nIn=o["nIn"], nBad=o["nBad"],
                ncorr=o["ncorr"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_numeric_and_analytic_agree_under_the_rule(variants, name):
    sc, ref = R.case(name)
    for o in variants[name]:
        print(name, R.compare(sc, ref, _as_got(o)))


def test_tolerance_is_measured(variants):
    worst = np.zeros((2, 3))
    for k in R.CASES:
        ref = R.case(k)[1]
        if ref["chi2"][1] is None:
            continue
        for i, o in enumerate(variants[k]):
            worst[i] = np.maximum(worst[i], R.distance(o, ref))
    print("numeric vs analytic   R %.3e t %.3e s %.3e" % tuple(worst[0]))
    print("float64 vs longdouble R %.3e t %.3e s %.3e" % tuple(worst[1]))
    assert 4 * worst.max() <= R.SIM3_TOL <= 4 * worst.max() * 1.05    # covers, and is not wider


def test_no_decision_hinges_on_an_ambiguous_pair():
    for k in R.CASES:
        sc, ref = R.case(k)
        a = int(R.ambiguous(ref).sum())
        n, nbad, nin = ref["ncorr"], ref["nBad"], ref["nIn"]
        assert a <= R.MAX_SKIPPED
        assert nbad == 0 and a == 0 or nbad > a, k                  # nBad == 0 versus > 0
        assert n - nbad - a >= 10 or n - nbad + a < 10, k           # the < 10 gate
        assert nin - a >= 20 or nin + a < 20, k                     # nIn against 20


def test_cases_exercise_what_they_are_for():
    for k in NO_OUTLIER:
        ref = R.case(k)[1]
        assert ref["nBad"] == 0, k
        if ref["ncorr"] >= 10:
            assert len(ref["trace"][1]) <= 5 and ref["nIn"] == ref["ncorr"], k
    for k in RETURN0:
        ref = R.case(k)[1]
        assert ref["nIn"] == 0 and ref["chi2"][1] is None and ref["chi2"][0] is not None, k
        assert 0 < ref["alive"].sum() < 10
    assert R.case("n10")[1]["nIn"] == 10 and R.case("n11_out1")[1]["nIn"] == 10
    assert R.case("n40_out8")[1]["nBad"] >= 8
    assert R.case("mostly_outliers")[1]["nBad"] >= 21
    assert sum(r["rejected"] for t in R.case("far_init")[1]["trace"] for r in t) >= 1
    assert R.CASES["two_cameras"]["K2"] != R.K_A
    for k in ("n257", "n300"):
        assert R.case(k)[1]["nIn"] >= 20


# ---- the shared statements on the host ----
def host_run(lib, names):
    """lib/sim3opt_host (csrc/sim3opt_host.hip: OptimizeSim3 through sim3opt_args.h's
    statements, in the kernel's summation order) on the named cases as one batch."""
    exe = os.path.join(os.path.dirname(lib.LIB_PATH), "sim3opt_host")
    recs = [records(R.case(k)[0]) for k in names]
    n1cap = max(R.case(k)[0]["n1"] for k in names)
    cap = max(64, (max(len(c) for _, c, _ in recs) + 63) // 64 * 64)
    corrs = np.zeros((len(names), cap), lib.SIM3OPT_CORR_DTYPE)
    for i, (_, c, _) in enumerate(recs):
        corrs[i, :len(c)] = c
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(np.array([len(names), cap, n1cap, 0], np.int32).tobytes())
            f.write(np.concatenate([p for p, _, _ in recs]).tobytes())
            f.write(corrs.tobytes())
            f.write(np.concatenate([h for _, _, h in recs]).tobytes())
        subprocess.check_output([exe, os.path.join(d, "in"), os.path.join(d, "out")])
        raw = open(os.path.join(d, "out"), "rb").read()
    nb = len(names) * lib.SIM3OPT_RESULT_DTYPE.itemsize
    return (np.frombuffer(raw[:nb], lib.SIM3OPT_RESULT_DTYPE),
            np.frombuffer(raw[nb:], np.uint8).reshape(len(names), n1cap))


def test_host_program_meets_the_rule(lib):
    names = list(R.CASES)
    res, keep = host_run(lib, names)
    for i, k in enumerate(names):
        sc, ref = R.case(k)
        assert set(np.unique(keep[i])) <= {0, 1} and not keep[i, sc["n1"]:].any()
        print(k, R.compare(sc, ref, as_got(res[i], keep[i, :sc["n1"]])))
        if sc["fix_scale"]:
            assert res[i]["s"] == float(sc["s12"])
