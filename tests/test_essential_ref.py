"""CPU: the premises of tests/test_gpu_essential.py, from tests/ref_essential.py alone.

  - sim3_log inverts sim3_exp in all four branches, and sim3_exp is the group exponential
    (ref_sim3opt.sim3_exp_series, the power series of the 4x4 generator);
  - in every case the reference LM stops by its own rule before iteration 20;
  - EG_TOL is measured: 4 x the largest difference between the delta 1e-9 run and the runs with
    reversed edge summation and with delta 1e-6.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_essential as E  # noqa: E402
import ref_sim3opt as R  # noqa: E402

RUN = [k for k in E.CASES if k not in ("n1", "e0")]


def vertex_distance(a, b):
    """The largest component of ref_sim3opt.distance over the vertices of two results."""
    return max(max(R.distance(dict(q=a["q"][v], t=a["t"][v], s=a["s"][v]),
                              dict(q=b["q"][v], t=b["t"][v], s=b["s"][v])))
               for v in range(len(b["s"])))


# (omega scale, sigma): theta and |sigma| on either side of 1e-5
BRANCHES = {"small_small": (1e-7, 3e-6), "small_sigma": (1e-7, 0.3),
            "theta_small": (0.7, -4e-6), "theta_sigma": (1.1, -0.4)}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_log_inverts_exp(name):
    th, sigma = BRANCHES[name]
    rng = np.random.default_rng(11)
    w = rng.normal(size=(64, 3))
    w *= th * rng.uniform(0.5, 1.0, (64, 1)) / np.linalg.norm(w, axis=1, keepdims=True)
    u = np.concatenate([w, rng.normal(size=(64, 3)), sigma * rng.uniform(0.5, 1.0, (64, 1))], 1)
    S = E.sim3_exp(u)
    d = 0.5 * (np.trace(E.rot_of_quat(S[0]), axis1=1, axis2=2) - 1)
    assert ((d > 1 - E.EPS) == (th < 1e-3)).all() and ((np.abs(u[:, 6]) < E.EPS) == (abs(sigma) < 1e-5)).all()
    back = E.sim3_log(S)
    print(name, float(np.abs(back - u).max()))
    assert np.abs(back - u).max() <= 1e-12


@pytest.mark.parametrize("name", list(BRANCHES))
def test_exp_is_the_group_exponential(name):
    th, sigma = BRANCHES[name]
    rng = np.random.default_rng(12)
    for _ in range(8):
        w = rng.normal(size=3)
        u = np.concatenate([w / np.linalg.norm(w) * th, rng.normal(size=3), [sigma]])
        q, t, s = E.sim3_exp(u[None])
        Rs, ts, ss = R.sim3_exp_series(u)
        q1, t1, s1 = R.sim3_exp(u)
        assert np.abs(E.rot_of_quat(q[0]) - Rs).max() <= 1e-10   # I + Om + Om^2 below 1e-5 rad
        # below 1e-5 g2o takes C = 1 for (e^sigma - 1) / sigma = 1 + sigma / 2 + ..., and A, B of
        # theta = 0: W is off by at most 1e-5 / 2 + 1e-5 / 6 relative
        tol = 1e-12 if (th > 1e-5 and abs(sigma) > 1e-5) else 1e-5 * np.linalg.norm(u[3:6])
        assert np.abs(t[0] - ts).max() <= tol and abs(s[0] - ss) <= 1e-15 * ss
        assert np.abs(q[0] - q1).max() <= 1e-14 and np.abs(t[0] - t1).max() <= 1e-14 and s[0] == s1


def test_big_angle_takes_the_acos_branch():
    sc, _ = E.case("big_angle")
    e = sc["edges"]
    err = E.edge_errors(E.measurements(sc), E.take(sc["Scw"], e[:, 0]), E.take(sc["Scw"], e[:, 1]))
    th = np.linalg.norm(err[:, :3], axis=1)
    assert th.max() > 0.8 and (th < 1e-8).sum() > len(e) // 2   # and most edges start at zero


@pytest.mark.parametrize("name", RUN)
def test_reference_stops_by_its_own_rule(name):
    sc, ref = E.case(name)
    print(name, ref["iterations"], ref["trials"], ref["stop"], ref["chi2"])
    assert 1 <= ref["iterations"] < E.ITERATIONS and ref["stop"] in ("rho", "gain")
    assert ref["chi2"][1] < ref["chi2"][0]
    f = sc["fixed"]
    for k, a in zip(("q", "t", "s"), sc["Scw"]):
        assert np.array_equal(ref[k][f], a[f])
    if sc["fix_scale"]:
        assert np.array_equal(ref["s"], sc["Scw"][2])


@pytest.mark.parametrize("name", ["n1", "e0"])
def test_nothing_to_optimise(name):
    sc, ref = E.case(name)
    assert ref["iterations"] == 0
    for k, a in zip(("q", "t", "s"), sc["Scw"]):
        assert np.array_equal(ref[k], a)


def test_scene_shapes():
    sc = E.case("ring24_mid")[0]
    e = sc["edges"]
    pairs = [tuple(sorted(p)) for p in e[:, :2].tolist()]
    assert len(set(pairs)) < len(pairs)                      # duplicate vertex pairs
    assert sc["fixed"] == 6 and [15, 3, 1] in e.tolist()     # an older loop edge
    assert 700 <= len(E.case("ring256")[0]["edges"]) <= 1100


def test_tolerance_is_measured():
    worst = 0.0
    for name in RUN:
        sc, ref = E.case(name)
        for kw in (dict(reverse=True), dict(delta=1e-6)):
            o = E.optimize(sc, **kw)
            d = vertex_distance(o, ref)
            c = abs(o["chi2"][1] - ref["chi2"][1]) / ref["chi2"][1]
            print(name, kw, o["iterations"], o["stop"], "distance %.3g chi2 %.3g" % (d, c))
            worst = max(worst, d, c)
    print("worst", worst, "EG_TOL", E.EG_TOL)
    assert 4 * worst <= E.EG_TOL <= 1.05 * 4 * worst
