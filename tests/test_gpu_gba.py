"""GPU: GlobalBundleAdjustment -- the sparse Schur plan (orbg_ba_graph_schur_plan_sparse), its
block-sparse LDL^T (bsolve_kernels.hip), the LM over it, orbg_global_ba_optimize and the
map-point correction -- against tests/ref_optim.py (the numeric reference, with its bounds) on
tests/ref_gba.py's scenes.  tests/test_gba_ref.py shows on the CPU that the reference's LM
decisions on these cases are clear and do not depend on the order of its sums, so the device
is held to the same path.  Every check prints its figures before asserting."""
import numpy as np
import pytest

import ref_gba as G
import ref_optim as R
from orb_slam2_test_amd import CorrectPointsGBA, GlobalBundleAdjustment
from orb_slam2_test_amd.optimizer import DeviceLBA
from test_gpu_optim_ref import GraphBA

pytestmark = pytest.mark.gpu

SOLVE_SCENES = ("ring12", "clique14", "two_islands", "band40")


class SparseBA(GraphBA):
    """GraphBA on the sparse plan (sparse=False: the dense plan, the parent path)."""

    def __init__(self, sparse=True):
        super().__init__()
        self.sparse = sparse
        self.info = None

    def _graph(self, poses, pts, edges):
        g = DeviceLBA(poses, pts, edges, graph=True)
        self.info = g.schur_plan(poses["fixed"], sparse=self.sparse)
        return g


@pytest.fixture(scope="module")
def scenes():
    return {k: f() for k, f in G.SCENES.items()}


@pytest.mark.parametrize("lam_scale", [1e-5, 1e-3, 10.0])
@pytest.mark.parametrize("name", SOLVE_SCENES)
def test_sparse_solve(scenes, name, lam_scale):
    """The sparse plan's increments within schur_tolerance of one dense solve of the whole
    system; the dense device plan on the same blocks differs by at most twice that bound (each
    is within it of the reference); a second solve gives the same bytes."""
    poses, pts, edges = scenes[name]
    impl = SparseBA()
    sy = R.check_schur(impl, poses, pts, edges, lam_scale, name=name + " sparse")
    assert impl.info["nfree"] == len(poses) - 1 and impl.info["l_blocks"] >= impl.info["s_blocks"]
    diag = np.abs(sy["hpose"].reshape(len(poses), 36)[:, ::7]).max()
    lam = lam_scale * float(diag)
    ok, dp, dq = impl.schur(poses, len(pts), edges, sy, lam)
    ok2, dp2, dq2 = impl.schur(poses, len(pts), edges, sy, lam)
    assert ok and ok2 and dp.tobytes() == dp2.tobytes() and dq.tobytes() == dq2.tobytes()
    okd, ddp, ddq = SparseBA(sparse=False).schur(poses, len(pts), edges, sy, lam)
    tol = R.schur_tolerance(sy, lam)
    scale = max(np.abs(ddp).max(), np.abs(ddq).max())
    fp, fq = np.abs(dp - ddp).max() / scale, np.abs(dq - ddq).max() / scale
    print("sparse vs dense plan %s lam %.3g: pose %.3g point %.3g (bound %.3g)"
          % (name, lam, fp, fq, 2 * tol))
    assert okd and fp <= 2 * tol and fq <= 2 * tol


@pytest.mark.parametrize("variant", ["+lone_point", "+fixed_last", "+two_fixed", "+third_inactive"])
def test_sparse_solve_variants(variant):
    """A point without an edge, a fixed pose that is not index 0, a second fixed pose, a third
    of the edges inactive."""
    label, poses, pts, edges = [v for v in G.variants("ring12") if v[0].endswith(variant)][0]
    impl = SparseBA()
    R.check_schur(impl, poses, pts, edges, 1e-3, name=label)
    _, dp, dq = impl.schur(poses, len(pts), edges, R.ba_system(poses, pts, edges), 1.0)
    assert not dp[poses["fixed"] != 0].any()
    if variant == "+lone_point":
        assert not dq[-1].any()


def test_sparse_solve_all_poses_fixed(scenes):
    poses, pts, edges = scenes["ring12"]
    poses = poses.copy()
    poses["fixed"] = 1
    impl = SparseBA()
    sy = R.check_schur(impl, poses, pts, edges, 1e-3, name="all fixed")
    assert len(sy["pose_index"]) == 0 and impl.info["nfree"] == 0
    ok, dp, dq = impl.schur(poses, len(pts), edges, sy, 1.0)
    assert ok and not dp.any() and dq.any()


def test_sparse_solve_pose_without_edge_at_lambda_zero(scenes):
    """Its diagonal block of S is zero: a zero pivot, ok = 0, every increment zero."""
    poses, pts, edges = G.with_lone_pose(scenes["ring12"])
    impl = SparseBA()
    sy = R.ba_system(poses, pts, edges)
    ok, dp, dq = impl.schur(poses, len(pts), edges, sy, 0.0)
    assert ok == 0 and not dp.any() and not dq.any()
    ok, dp, dq = impl.schur(poses, len(pts), edges, sy, 1.0)     # damped: solvable again
    assert ok == 1 and dp[:-1].any() and not dp[-1].any()


@pytest.mark.parametrize("label", sorted(G.LM_CASES))
def test_sparse_optimize(label):
    """optimize(iterations) on the sparse plan takes the reference LM's path and arrives at
    its estimates (check_optimize: TOL_LM_*; fixed poses byte-identical)."""
    make, iters = G.LM_CASES[label]
    poses, pts, edges = make()
    (gp, gq, rep), (_, _, rrep) = R.check_optimize(SparseBA(), poses, pts, edges, iters, name=label)
    assert rep["final_chi2"] < rep["initial_chi2"]
    if label.endswith("/far"):
        assert rep["trials"] > rep["iterations"]


def test_sparse_optimize_after_set_active(scenes):
    """A third of the edges switched off through set_active: the plan is rebuilt as a sparse
    one, with fewer blocks of S (a covisibility pair is gone)."""
    sc = scenes["ring12"]
    poses, pts, edges = sc
    active = G.third_inactive(sc)
    impl = SparseBA()
    R.check_optimize(impl, poses, pts, edges, 10, active=active, name="ring12 third inactive")
    full = impl.info["s_blocks"]
    g = impl._graph(poses, pts, edges)
    g.set_active(active)
    e2 = edges.copy()
    e2["active"] = active
    g.build_system()
    g.schur_solve(1.0)
    g.ctx.sync()
    cold = SparseBA()          # the same active set given at creation: the same plan, the same bytes
    h = cold._graph(poses, pts, e2)
    h.build_system()
    h.schur_solve(1.0)
    h.ctx.sync()
    assert cold.info["s_blocks"] < full
    assert g.d_dx_pose.cpu().numpy().tobytes() == h.d_dx_pose.cpu().numpy().tobytes()


@pytest.mark.parametrize("stop_it,stop_trial", [(-2, -1), (2, -1), (0, 0), (1, 0)])
def test_sparse_optimize_force_stop_flag(oracle, stop_it, stop_trial):
    """The force-stop flag raised by a post-iteration / post-trial action of orbg_lm_control at
    (stop_it, stop_trial) (-2: before the call) stops the sparse-plan LM where the restated LM
    with the same flag (oracle ba_optimize_ctl, as tests/test_gpu_ba.py's LBA test) stops: the
    same iterations, trials and terminated = 3.  Estimates: both are within TOL_LM_EST of
    ref_optim's LM on a clear case, so within twice that of each other."""
    poses, pts, edges = G.clique14(robust=True, s_pose=0.1, s_point=2.0)
    g = SparseBA()._graph(poses, pts, edges)
    flag = np.zeros(1, np.uint8)
    flag[0] = 1 if stop_it == -2 else 0

    def post_iteration(it):
        if it == stop_it and stop_trial == -1:
            flag[0] = 1

    def post_trial(it, tr):
        if it == stop_it and tr == stop_trial:
            flag[0] = 1

    rep = g.optimize_ctl(10, stop_flag=flag, post_iteration=post_iteration, post_trial=post_trial)
    gp, gq = g.estimates()
    rp, rq, rrep = oracle.ba_optimize_ctl(poses, pts, edges, 10, stop_it=stop_it,
                                          stop_trial=stop_trial)
    print("stop (%d, %d):" % (stop_it, stop_trial), rep, rrep)
    for k in ("iterations", "trials", "terminated"):
        assert rep[k] == rrep[k], (k, rep, rrep)
    assert rep["terminated"] == 3
    if stop_it == -2:
        assert rep["iterations"] == 0 and gp.tobytes() == np.asarray(poses).tobytes()
        return
    assert rep["iterations"] == stop_it + 1
    sgn = np.where(np.sum(gp["q"] * rp["q"], 1) < 0, -1.0, 1.0)[:, None]
    fe = max(R.rel(gq, rq), R.rel(gp["t"], rp["t"]), float(np.abs(sgn * gp["q"] - rp["q"]).max()))
    print("stop (%d, %d): estimates %.3g (bound %.3g)" % (stop_it, stop_trial, fe, 2 * R.TOL_LM_EST))
    assert fe <= 2 * R.TOL_LM_EST


def test_global_ba_optimize_equals_graph_path(scenes):
    """orbg_global_ba_optimize from host arrays = graph + sparse plan + optimize, byte for
    byte; a point and a pose without edges and the fixed pose come back untouched; the report
    carries the LM's and the plan's figures."""
    poses, pts, edges = G.with_lone_point(G.with_lone_pose(scenes["ring12"]))
    impl = SparseBA()
    gp, gq, grep = impl.optimize(poses, pts, edges, 10)
    hp, hq, rep = GlobalBundleAdjustment(poses, pts, edges, 10)
    assert hp.tobytes() == gp.tobytes() and hq.tobytes() == gq.tobytes()
    assert hq[-1].tobytes() == pts[-1].tobytes() and hp[0].tobytes() == poses[0].tobytes()
    assert hp[-1].tobytes() == poses[-1].tobytes()
    assert (hq[:-1] != pts[:-1]).any() and (hp["t"][1:-1] != poses["t"][1:-1]).any()
    for k in ("iterations", "trials", "terminated", "initial_chi2", "final_chi2", "lambda"):
        assert rep[k] == grep[k], k
    assert rep["iterations"] >= 1 and rep["final_chi2"] < rep["initial_chi2"]
    assert rep["plan"] == impl.info and rep["plan"]["nfree"] == len(poses) - 1
    flag = np.ones(1, np.uint8)
    sp, sq, srep = GlobalBundleAdjustment(poses, pts, edges, 10, stop_flag=flag)
    assert srep["iterations"] == 0 and srep["terminated"] == 3
    assert sp.tobytes() == poses.tobytes() and sq.tobytes() == pts.tobytes()


def test_gba_point_correction():
    """Bit-equal to the NumPy restatement on 1000 points over 8 keyframes, ref < 0 among them."""
    rng = np.random.default_rng(9)
    poses, pts, _ = G.gba_scene(8, 1000, 2, seed=21)
    Tb = np.stack([R.pose_matrix(p["q"], p["t"]) for p in poses]).astype(np.float32)
    moved = poses.copy()
    moved["t"] += rng.normal(0, 0.3, moved["t"].shape)
    Ta = np.linalg.inv(np.stack([R.pose_matrix(p["q"], p["t"]) for p in moved])).astype(np.float32)
    x = pts.astype(np.float32)
    ref = rng.integers(-1, 8, len(x)).astype(np.int32)
    assert (ref < 0).any() and len(x) == 1000
    got = CorrectPointsGBA(Tb, Ta, ref, x)
    want = G.correct_points(Tb, Ta, ref, x)
    assert got.tobytes() == want.tobytes()
    assert got[ref < 0].tobytes() == x[ref < 0].tobytes() and (got[ref >= 0] != x[ref >= 0]).any()
