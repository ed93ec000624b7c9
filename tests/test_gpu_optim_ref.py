"""GPU: PoseOptimization (k_pose_opt), the LocalBundleAdjustment linearisation, Schur solve,
update and device LM against tests/ref_optim.py, an independent NumPy float64 statement of the
same operations -- no oracle here.  tests/test_optim_ref.py holds the oracle to the same
reference on the same cases, and checks the reference's own premises, on the CPU.

Bounds are ref_optim.py's: derived ones for the per-edge records, blocks, solve and update;
measured ones (4 x the larger of CPU-oracle-vs-reference and GPU-vs-reference) after LM
iterations.  Every check prints its figures before asserting (run with -s to measure)."""
import numpy as np
import pytest

import ref_optim as R
from orb_slam2_test_amd import PoseOptimization, linearize_local_ba
from orb_slam2_test_amd import _lib as L
from orb_slam2_test_amd import synthetic as S
from orb_slam2_test_amd.optimizer import DeviceLBA, ba_errors, ba_schur_solve

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ PoseOptimization
class DevicePose:
    def pose(self, edges, cam, T0):
        n, To, q, t, out = PoseOptimization(edges, T0, *cam)
        # SetPose's float matrix is the double pose rounded once
        T = R.pose_matrix(q, t)[:3]
        assert np.abs(To - T).max() <= R.EPS32 * max(1.0, np.abs(T).max())
        return q, t, out, n


@pytest.fixture(scope="module")
def pose_refs():
    refs = {}
    for case in R.POSE_CASES + R.POSE_BATCH_CASES:
        e, _, T0 = R.pose_scene(*case)
        refs[case] = (e, T0, R.pose_optimization(e, R.CAM, T0))
    return refs


@pytest.mark.parametrize("case", R.POSE_CASES)
def test_pose_optimization(pose_refs, case):
    e, T0, ref = pose_refs[case]
    rmin = R.pose_minimiser(e, R.CAM, T0) if case in R.POSE_MIN_CASES else None
    R.check_pose(DevicePose(), e, T0, ref, rmin, name=str(case))


class BatchPose:
    """orbg_pose_optimization_batch_device on POSE_BATCH_CASES at once; pose() hands out
    frame i's slice."""
    SENTINEL = 0xA5

    def __init__(self, frames):
        import torch
        from orb_slam2_test_amd.orbmatcher import _ctx
        B = len(frames)
        self.cap = cap = max(len(e) for e, _ in frames) + 37
        ed = np.zeros((B, cap), L.PEDGE_DTYPE)
        cnt = np.zeros(B, np.int32)
        tin = np.zeros((B, 12), np.float32)
        cams = (L.PoseCamera * B)()
        for i, (e, T0) in enumerate(frames):
            ed[i, :len(e)] = e
            cnt[i] = len(e)
            tin[i] = np.asarray(T0, np.float32).reshape(12)
            cams[i] = L.PoseCamera(*[float(np.float32(v)) for v in R.CAM], 0.0)
        dev = "cuda"
        d_e = torch.from_numpy(ed.view(np.uint8).reshape(-1)).to(dev)
        d_cnt = torch.from_numpy(cnt).to(dev)
        d_cam = torch.from_numpy(np.frombuffer(bytes(cams), np.uint8).copy()).to(dev)
        d_tin = torch.from_numpy(tin).to(dev)
        d_q = torch.zeros(B * 4, dtype=torch.float64, device=dev)
        d_t = torch.zeros(B * 3, dtype=torch.float64, device=dev)
        d_to = torch.zeros(B * 12, dtype=torch.float32, device=dev)
        d_out = torch.full((B * cap,), self.SENTINEL, dtype=torch.uint8, device=dev)
        d_ni = torch.zeros(B, dtype=torch.int32, device=dev)
        ctx = _ctx(0)
        torch.cuda.synchronize()
        L.check(L.lib().orbg_pose_optimization_batch_device(
            ctx.handle, d_e.data_ptr(), d_cnt.data_ptr(), cap, d_cam.data_ptr(), d_tin.data_ptr(),
            d_q.data_ptr(), d_t.data_ptr(), d_to.data_ptr(), d_out.data_ptr(), d_ni.data_ptr(), B),
            "pose batch")
        ctx.sync()
        self.q = d_q.cpu().numpy().reshape(B, 4)
        self.t = d_t.cpu().numpy().reshape(B, 3)
        self.out = d_out.cpu().numpy().reshape(B, cap)
        self.ni = d_ni.cpu().numpy()
        self.cnt = cnt
        self.i = 0

    def pose(self, edges, cam, T0):
        i = self.i
        return self.q[i], self.t[i], self.out[i, :len(edges)] != 0, int(self.ni[i])


def test_pose_optimization_batch(pose_refs):
    """The batched device entry with counts mixed below the capacity (0 and 2 among them):
    every frame within the bounds of its reference and equal to its single-frame result,
    the outlier bytes past counts[f] untouched."""
    frames = [pose_refs[c][:2] for c in R.POSE_BATCH_CASES]
    b = BatchPose(frames)
    for i, case in enumerate(R.POSE_BATCH_CASES):
        e, T0, ref = pose_refs[case]
        b.i = i
        R.check_pose(b, e, T0, ref, name="batch %s" % (case,))
        assert np.all(b.out[i, len(e):] == b.SENTINEL)
        assert set(np.unique(b.out[i, :len(e)])) <= {0, 1}
        n, To, q, t, out = PoseOptimization(e, T0, *R.CAM)
        assert n == b.ni[i] and np.array_equal(out, b.out[i, :len(e)] != 0)
        assert np.array_equal(q, b.q[i]) and np.array_equal(t, b.t[i])


# ------------------------------------------------------------------ local BA
def _sync_torch():
    import torch
    torch.cuda.synchronize()        # torch's copies before liborbg's stream reads them


class RecordBA:
    """The host entry points (orbg_ba_linearize, orbg_ba_errors, orbg_ba_schur_solve)."""

    def linearize(self, poses, pts, edges):
        eo, hp, bp, hq, bq = linearize_local_ba(poses, pts, edges)
        out = {k: eo[k] for k in ("err", "chi2", "rho1", "jp", "jt", "hpl")}
        out.update(hpose=hp, bpose=bp, hpoint=hq, bpoint=bq)
        return out

    def errors(self, poses, pts, edges):
        return ba_errors(poses, pts, edges)

    def schur(self, poses, npoint, edges, sy, lam):
        eo = np.zeros(len(edges), L.EDGE_OUT_DTYPE)
        eo["hpl"] = sy["hpl"]
        return ba_schur_solve(poses, npoint, edges, eo, sy["hpose"], sy["bpose"], sy["hpoint"],
                              sy["bpoint"], lam)


class ResidentBA:
    """DeviceLBA with every array in HBM (orbg_ba_linearize_device)."""

    def linearize(self, poses, pts, edges):
        lba = DeviceLBA(poses, pts, edges)
        lba.linearize()
        eo, hp, bp, hq, bq = lba.download()
        out = {k: eo[k] for k in ("err", "chi2", "rho1", "jp", "jt", "hpl")}
        out.update(hpose=hp, bpose=bp, hpoint=hq, bpoint=bq)
        return out


class GraphBA:
    """DeviceLBA(graph=True): the packed graph's build / error pass / Schur solve / update /
    LM (orbg_ba_graph_*).  `edges`: the graph update() runs on."""

    def __init__(self, edges=None):
        self.edges = edges

    def _graph(self, poses, pts, edges):
        g = DeviceLBA(poses, pts, edges, graph=True)
        g.schur_plan(poses["fixed"])
        return g

    def linearize(self, poses, pts, edges):
        import torch
        g = DeviceLBA(poses, pts, edges, graph=True)
        g.build_system()
        for t in (g.d_hpose, g.d_bpose, g.d_hpoint, g.d_bpoint):    # the build writes every block
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        g.build_system()
        g.ctx.sync()
        ne, npo, npt = len(edges), len(poses), len(pts)
        return dict(hpl=g.d_hpl.cpu().numpy()[:ne], hpose=g.d_hpose.cpu().numpy()[:npo],
                    bpose=g.d_bpose.cpu().numpy()[:npo], hpoint=g.d_hpoint.cpu().numpy()[:npt],
                    bpoint=g.d_bpoint.cpu().numpy()[:npt])

    def errors(self, poses, pts, edges):
        g = DeviceLBA(poses, pts, edges, graph=True)
        g.errors()
        g.ctx.sync()
        ne = len(edges)
        return None, g.d_chi2.cpu().numpy()[:ne], g.d_rho0.cpu().numpy()[:ne], None, None

    def schur(self, poses, npoint, edges, sy, lam):
        import torch
        g = self._graph(poses, np.zeros((npoint, 3)), edges)
        g.build_system()            # allocates d_hpl; the blocks are then the reference's
        g.ctx.sync()
        ne = len(edges)
        g.d_hpl[:ne].copy_(torch.from_numpy(sy["hpl"]))
        for t, k in ((g.d_hpose, "hpose"), (g.d_bpose, "bpose"), (g.d_hpoint, "hpoint"),
                     (g.d_bpoint, "bpoint")):
            t.copy_(torch.from_numpy(sy[k]))
        _sync_torch()
        g.schur_solve(lam)
        g.ctx.sync()
        return (int(g.d_ok.cpu().numpy()[0]), g.d_dx_pose.cpu().numpy(),
                g.d_dx_point.cpu().numpy())

    def update(self, poses, pts, dxp, dxq):
        import torch
        g = self._graph(poses, pts, self.edges)
        g.d_dx_pose.copy_(torch.from_numpy(dxp))
        g.d_dx_point.copy_(torch.from_numpy(dxq))
        _sync_torch()
        g.update()
        return g.estimates()

    def optimize(self, poses, pts, edges, iters, active=None, robust=None):
        g = self._graph(poses, pts, edges)
        if active is not None:
            g.set_active(active)
        if robust is not None:
            g.set_robust(robust)
        rep = g.optimize(iters)
        gp, gq = g.estimates()
        return gp, gq, rep


@pytest.fixture(scope="module")
def ba_scenes():
    return {k: f() for k, f in R.BA_SCENES.items()}


@pytest.mark.parametrize("path", ["record", "resident", "graph"])
@pytest.mark.parametrize("name", sorted(R.BA_SCENES))
def test_linearize(ba_scenes, name, path):
    """err, chi2, rho', Jp, Jt, H_pl and the four block arrays of the three paths (the graph
    path has no per-edge record: its H_pl and blocks, and chi2 / rho from its error pass)."""
    poses, pts, edges = ba_scenes[name]
    impl = dict(record=RecordBA, resident=ResidentBA, graph=GraphBA)[path]()
    sy, got = R.check_linearize(impl, poses, pts, edges, name="%s/%s" % (name, path))
    fixed = poses["fixed"] != 0
    assert not np.asarray(got["hpose"])[fixed].any() and not np.asarray(got["bpose"])[fixed].any()
    assert not np.asarray(got["hpl"])[fixed[edges["pose"]]].any()
    if path != "resident":
        R.check_errors(impl, poses, pts, edges, name="%s/%s" % (name, path))


@pytest.mark.parametrize("path", ["record", "graph"])
@pytest.mark.parametrize("lam_scale", [1e-5, 1e-3, 10.0])
def test_schur_solve(lam_scale, path):
    poses, pts, edges = R.ba_perturbed(70, 150)
    impl = dict(record=RecordBA, graph=GraphBA)[path]()
    R.check_schur(impl, poses, pts, edges, lam_scale, name=path)


@pytest.mark.parametrize("path", ["record", "graph"])
def test_schur_solve_all_poses_fixed(path):
    poses, pts, edges = R.ba_perturbed(70, 150)
    poses["fixed"] = 1
    impl = dict(record=RecordBA, graph=GraphBA)[path]()
    sy = R.check_schur(impl, poses, pts, edges, 1e-3, name=path + " all fixed")
    assert len(sy["pose_index"]) == 0


def test_update():
    """k_ba_update against oplus: |omega| from 1e-7 across the 1e-5 branch switch up to 3.1
    rad, translations up to 100 m, fixed poses untouched, unit quaternions."""
    poses, pts, edges = S.ba_window(n_local=13, n_fixed=3, n_points=20, seed=31)
    dxp = R.update_twists(len(poses))
    dxq = np.random.default_rng(6).normal(0, 1e-2, pts.shape)
    R.check_update(GraphBA(edges), poses, pts, dxp, dxq)


@pytest.mark.parametrize("case", R.LM_CASES)
def test_optimize(case):
    seed, npt, iters, sp, sq = case
    poses, pts, edges = R.ba_perturbed(seed, npt, sp, sq)
    (gp, gq, rep), _ = R.check_optimize(GraphBA(), poses, pts, edges, iters, name=str(case))
    assert rep["final_chi2"] < rep["initial_chi2"]


def test_lba_sequence():
    """LocalBundleAdjustment's optimize(5) -> deactivate by chi2 / depth, drop the robust
    kernels -> optimize(10) (Optimizer.cc:857-905) on two windows in one graph."""
    R.check_lba_sequence(GraphBA())
