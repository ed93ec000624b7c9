"""Optimizer -- the per-edge arithmetic of Optimizer::LocalBundleAdjustment on the GPU.

Reference: src/Optimizer.cc:633-979 builds a g2o graph with EdgeSE3ProjectXYZ /
EdgeStereoSE3ProjectXYZ edges (Huber delta sqrt(5.991) / sqrt(7.815), information
invSigma2 * I) and runs Levenberg-Marquardt.  The LM driver, Schur solve and map
write-back stay on the host (they are sequential); this module replaces the
arithmetic g2o performs per edge in computeActiveErrors + BlockSolver::buildSystem:
residual, analytic Jacobians, chi2, Huber weight and the J^T W J / J^T W r blocks.

Arrays use the dtypes of ``_lib`` (POSE_DTYPE, EDGE_DTYPE, EDGE_OUT_DTYPE).

PoseOptimization (Optimizer.cc:356-631) and OptimizeSim3 (:1366-1578, the Sim3 refinement of
LoopClosing::ComputeSim3) run whole on the device, LM driver included: one workgroup per frame
or per loop candidate.  OptimizeEssentialGraph (:1021-1324, the pose graph of
LoopClosing::CorrectLoop) keeps its state on the device and its LM loop on the host.
"""
import ctypes
import math

import numpy as np

from . import _lib as L
from .orbmatcher import _ctx

TH_HUBER_MONO = float(np.float32(math.sqrt(5.991)))     # const float thHuberMono (Optimizer.cc:758)
TH_HUBER_STEREO = float(np.float32(math.sqrt(7.815)))   # const float thHuberStereo (:759)
CHI2_MONO = 5.991                                       # outlier cut (:879)
CHI2_STEREO = 7.815                                     # (:895)


def linearize_local_ba(poses, points, edges, device=0, with_edges=True):
    """Returns (edge_out | None, H_pose[np,6,6], b_pose[np,6], H_point[nq,3,3], b_point[nq,3])."""
    poses = np.ascontiguousarray(poses, L.POSE_DTYPE)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, L.EDGE_DTYPE)
    npose, npoint, nedge = len(poses), len(points), len(edges)
    eout = np.zeros(nedge, L.EDGE_OUT_DTYPE) if with_edges else None
    hpose = np.zeros((npose, 6, 6))
    bpose = np.zeros((npose, 6))
    hpoint = np.zeros((npoint, 3, 3))
    bpoint = np.zeros((npoint, 3))
    L.check(L.lib().orbg_ba_linearize(_ctx(device).handle, L.ptr(poses), npose, L.ptr(points),
                                      npoint, L.ptr(edges), nedge, L.ptr(eout), L.ptr(hpose),
                                      L.ptr(bpose), L.ptr(hpoint), L.ptr(bpoint)),
            "orbg_ba_linearize")
    return eout, hpose, bpose, hpoint, bpoint


def ba_errors(poses, points, edges, device=0):
    """g2o's per-trial error pass (computeActiveErrors + activeRobustChi2 terms +
    isDepthPositive, sparse_optimizer.cpp:61-114, orbg_ba_errors) for the LBA edges.
    Returns (err (n, 3), chi2 (n,), rho0 (n,), depth_ok (n,) bool, active robust chi2 sum in
    edge order)."""
    poses = np.ascontiguousarray(poses, L.POSE_DTYPE)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, L.EDGE_DTYPE)
    n = len(edges)
    err = np.zeros((max(n, 1), 3))
    chi2 = np.zeros(max(n, 1))
    rho0 = np.zeros(max(n, 1))
    dok = np.zeros(max(n, 1), np.uint8)
    tot = ctypes.c_double()
    L.check(L.lib().orbg_ba_errors(_ctx(device).handle, L.ptr(poses), len(poses), L.ptr(points),
                                   len(points), L.ptr(edges), n, L.ptr(err), L.ptr(chi2),
                                   L.ptr(rho0), L.ptr(dok), ctypes.byref(tot)), "orbg_ba_errors")
    return err[:n], chi2[:n], rho0[:n], dok[:n].astype(bool), tot.value


def ba_schur_solve(poses, npoint, edges, eout, hpose, bpose, hpoint, bpoint, lam, device=0):
    """g2o BlockSolver<6,3>::solve (block_solver.hpp:354-486) after setLambda(lam), on
    linearize_local_ba's outputs.  Returns (ok, dx_pose (npose, 6), dx_point (npoint, 3))."""
    poses = np.ascontiguousarray(poses, L.POSE_DTYPE)
    edges = np.ascontiguousarray(edges, L.EDGE_DTYPE)
    eout = np.ascontiguousarray(eout, L.EDGE_OUT_DTYPE)
    arrs = [np.ascontiguousarray(a, np.float64) for a in (hpose, bpose, hpoint, bpoint)]
    dp = np.zeros((max(len(poses), 1), 6))
    dq = np.zeros((max(npoint, 1), 3))
    ok = ctypes.c_int()
    L.check(L.lib().orbg_ba_schur_solve(_ctx(device).handle, L.ptr(poses), len(poses), npoint,
                                        L.ptr(edges), len(edges), L.ptr(eout), *[L.ptr(a) for a in arrs],
                                        float(lam), L.ptr(dp), L.ptr(dq), ctypes.byref(ok)),
            "orbg_ba_schur_solve")
    return bool(ok.value), dp[:len(poses)], dq[:npoint]


def PoseOptimization(edges, Tcw, fx, fy, cx, cy, bf, device=0):
    """Optimizer::PoseOptimization (Optimizer.cc:356-631) on one frame.

    edges: PEDGE_DTYPE records, one per keypoint with a MapPoint in index order (obs =
    kpUn.pt.x, kpUn.pt.y, mvuRight; xw = world position; inv_sigma2 = mvInvLevelSigma2
    [octave]; stereo = mvuRight >= 0).  Tcw: pFrame->mTcw (3x4 or 4x4).  Returns
    (nInliers, Tcw_out (3, 4) float32 = SetPose's matrix, q (x, y, z, w), t, mvbOutlier)."""
    e = np.ascontiguousarray(edges, L.PEDGE_DTYPE)
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4].reshape(12))
    cam = L.PoseCamera(*[float(np.float32(v)) for v in (fx, fy, cx, cy, bf)], 0.0)
    q = np.zeros(4)
    t = np.zeros(3)
    To = np.zeros(12, np.float32)
    out = np.zeros(max(len(e), 1), np.uint8)
    ni = ctypes.c_int()
    L.check(L.lib().orbg_pose_optimization(_ctx(device).handle, L.ptr(e), len(e), ctypes.byref(cam),
                                           L.ptr(T), L.ptr(q), L.ptr(t), L.ptr(To), L.ptr(out),
                                           ctypes.byref(ni)), "orbg_pose_optimization")
    return ni.value, To.reshape(3, 4), q, t, out[:len(e)].astype(bool)


def _pose34(T):
    T = np.asarray(T, np.float32)
    if T.shape not in ((3, 4), (4, 4)):
        raise ValueError("a pose is 3x4 or 4x4")
    return np.ascontiguousarray(T[:3, :4]).reshape(12)


def _intrinsics(K):
    K = np.asarray(K, np.float32)
    if K.shape == (3, 3):
        return K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if K.shape == (4,):
        return tuple(K)
    raise ValueError("K is 3x3 or (fx, fy, cx, cy)")


SIM3OPT_MAX_N = 8192   # correspondences per candidate (ORBG_ENOTSUP past it)


def sim3opt_records(T1w, T2w, K1, K2, Xw1, Xw2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, index1,
                    R12, t12, s12, th2, bFixScale):
    """(orbg_sim3opt_problem [1], orbg_sim3opt_corr [n], orbg_sim3_hyp [1]) of one
    OptimizeSim3 call from its arrays."""
    Xw1 = np.asarray(Xw1, np.float32).reshape(-1, 3)
    n = len(Xw1)
    p = np.zeros(1, L.SIM3OPT_PROBLEM_DTYPE)
    p["T1w"][0], p["T2w"][0] = _pose34(T1w), _pose34(T2w)
    p["fx1"], p["fy1"], p["cx1"], p["cy1"] = _intrinsics(K1)
    p["fx2"], p["fy2"], p["cx2"], p["cy2"] = _intrinsics(K2)
    p["n"], p["fix_scale"], p["th2"] = n, 1 if bFixScale else 0, np.float32(th2)
    c = np.zeros(n, L.SIM3OPT_CORR_DTYPE)
    c["Xw1"] = Xw1
    c["Xw2"] = np.asarray(Xw2, np.float32).reshape(n, 3)
    c["obs1"] = np.asarray(obs1, np.float32).reshape(n, 2)
    c["obs2"] = np.asarray(obs2, np.float32).reshape(n, 2)
    c["inv_sigma2_1"] = np.asarray(inv_sigma2_1, np.float32).reshape(n)
    c["inv_sigma2_2"] = np.asarray(inv_sigma2_2, np.float32).reshape(n)
    c["index1"] = np.asarray(index1, np.int32).reshape(n)
    h = np.zeros(1, L.SIM3_HYP_DTYPE)
    h["R"][0] = np.asarray(R12, np.float32).reshape(9)
    h["t"][0] = np.asarray(t12, np.float32).reshape(3)
    h["s"] = np.float32(s12)
    return p, c, h


def optimize_sim3(problem, corrs, init, n1, ctx=None, device=0):
    """orbg_optimize_sim3 on records: (SIM3OPT_RESULT_DTYPE scalar, keep uint8 [n1])."""
    problem = np.ascontiguousarray(problem, L.SIM3OPT_PROBLEM_DTYPE).reshape(1)
    corrs = np.ascontiguousarray(corrs, L.SIM3OPT_CORR_DTYPE).reshape(-1)
    init = np.ascontiguousarray(init, L.SIM3_HYP_DTYPE).reshape(1)
    if len(corrs) < int(problem["n"][0]):
        raise ValueError("fewer correspondences than the problem names")
    result = np.zeros(1, L.SIM3OPT_RESULT_DTYPE)
    keep = np.zeros(int(n1), np.uint8)
    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_optimize_sim3(h, L.ptr(problem), L.ptr(corrs), L.ptr(init), int(n1),
                                       L.ptr(result), L.ptr(keep)), "orbg_optimize_sim3")
    return result[0], keep


def OptimizeSim3(T1w, T2w, K1, K2, Xw1, Xw2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, index1, n1,
                 R12, t12, s12, th2=10.0, bFixScale=False, device=0):
    """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)
    (Optimizer.cc:1366-1578) on the device.

    T1w / T2w: pKF1 / pKF2 GetPose(); K1 / K2: mK (3x3, or fx, fy, cx, cy).  Per compacted
    correspondence (the pointer tests of :1426-1463 stay with the caller): Xw1 / Xw2 the world
    positions of pMP1 / pMP2, obs1 / obs2 the undistorted keypoints, inv_sigma2_* =
    mvInvLevelSigma2[octave], index1 the slot in vpMatches1 (n1 = its size).  R12, t12, s12:
    the Sim3 to refine (float, as Sim3Solver returns it).

    Returns (nIn, (q, t, s), keep): the return value, g2oS12 in double (q = x, y, z, w) and
    keep bool [n1], True where vpMatches1[j] is still set."""
    p, c, h = sim3opt_records(T1w, T2w, K1, K2, Xw1, Xw2, obs1, obs2, inv_sigma2_1,
                              inv_sigma2_2, index1, R12, t12, s12, th2, bFixScale)
    r, keep = optimize_sim3(p, c, h, n1, device=device)
    return int(r["ninliers"]), (r["q"].copy(), r["t"].copy(), float(r["s"])), keep.astype(bool)


def OptimizeSim3Batch(problems, device=0):
    """OptimizeSim3 over a list of candidates in one launch
    (orbg_optimize_sim3_batch_device).  Each item is a dict of OptimizeSim3's arguments
    (th2 and bFixScale optional).  Returns a list of (nIn, (q, t, s), keep)."""
    if not problems:
        return []
    recs = [sim3opt_records(*[d[k] for k in ("T1w", "T2w", "K1", "K2", "Xw1", "Xw2", "obs1", "obs2",
                                             "inv_sigma2_1", "inv_sigma2_2", "index1", "R12", "t12",
                                             "s12")], d.get("th2", 10.0), d.get("bFixScale", False))
            for d in problems]
    n1s = [int(d["n1"]) for d in problems]
    nmax = max(len(c) for _, c, _ in recs)
    if nmax > SIM3OPT_MAX_N:
        raise L.OrbgError(L.ORBG_ENOTSUP, "OptimizeSim3: more than %d correspondences" % SIM3OPT_MAX_N)
    for (_, c, _), n1 in zip(recs, n1s):
        if len(c) and not (0 <= c["index1"].min() and c["index1"].max() < n1):
            raise ValueError("index1 outside [0, n1)")
    res, keep = optimize_sim3_batch(np.concatenate([p for p, _, _ in recs]), [c for _, c, _ in recs],
                                    np.concatenate([h for _, _, h in recs]), max(max(n1s), 1),
                                    device=device)
    return [(int(r["ninliers"]), (r["q"].copy(), r["t"].copy(), float(r["s"])),
             keep[i, :n1s[i]].astype(bool)) for i, r in enumerate(res)]


def optimize_sim3_batch(problems, corr_list, init, n1cap, cap=None, ctx=None, device=0):
    """orbg_optimize_sim3_batch_device from host records: uploads, launches once on the context
    stream, downloads.  corr_list[p] = candidate p's records; cap defaults to the smallest
    multiple of 64 that holds the longest.  Returns (SIM3OPT_RESULT_DTYPE [npairs], keep uint8
    [npairs][n1cap])."""
    import torch
    problems = np.ascontiguousarray(problems, L.SIM3OPT_PROBLEM_DTYPE).reshape(-1)
    init = np.ascontiguousarray(init, L.SIM3_HYP_DTYPE).reshape(-1)
    npairs = len(problems)
    if cap is None:
        cap = max(64, (max([len(c) for c in corr_list] + [1]) + 63) // 64 * 64)
    corrs = np.zeros((npairs, cap), L.SIM3OPT_CORR_DTYPE)
    for i, c in enumerate(corr_list):
        corrs[i, :len(c)] = c

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    c_ = ctx if ctx is not None else _ctx(device)
    d_p, d_c, d_h = up(problems), up(corrs), up(init)
    d_r = torch.zeros(npairs * L.SIM3OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_k = torch.zeros((npairs, int(n1cap)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().orbg_optimize_sim3_batch_device(
        c_.handle, d_p.data_ptr(), d_c.data_ptr(), d_h.data_ptr(), npairs, int(cap),
        d_r.data_ptr(), d_k.data_ptr(), int(n1cap)), "orbg_optimize_sim3_batch_device")
    c_.sync()
    return d_r.cpu().numpy().view(L.SIM3OPT_RESULT_DTYPE), d_k.cpu().numpy()


def sim3d_records(S):
    """orbg_sim3d [n] from SIM3D_DTYPE records, or from a sequence of (q, t, s) with q =
    (x, y, z, w)."""
    if isinstance(S, np.ndarray) and S.dtype == L.SIM3D_DTYPE:
        return np.ascontiguousarray(S).reshape(-1)
    out = np.zeros(len(S), L.SIM3D_DTYPE)
    for k, (q, t, s) in enumerate(S):
        out["q"][k], out["t"][k], out["s"][k] = q, t, s
    return out


def eg_edge_records(edges):
    """orbg_eg_edge [n] from EG_EDGE_DTYPE records or an (n, 3) array of (i, j, kind)."""
    if isinstance(edges, np.ndarray) and edges.dtype == L.EG_EDGE_DTYPE:
        return np.ascontiguousarray(edges).reshape(-1)
    e = np.asarray(edges, np.int64).reshape(-1, 3)
    out = np.zeros(len(e), L.EG_EDGE_DTYPE)
    out["i"], out["j"], out["kind"] = e[:, 0], e[:, 1], e[:, 2]
    return out


def _lm_report(rep):
    return dict(iterations=rep.iterations, trials=rep.trials, terminated=rep.terminated,
                initial_chi2=rep.initial_chi2, final_chi2=rep.final_chi2, lam=rep.lam)


def OptimizeEssentialGraph(Scw, Snc, edges, fixed, bFixScale, iterations=20, device=0):
    """The optimisation of Optimizer::OptimizeEssentialGraph (Optimizer.cc:1021-1286) on the
    device (orbg_optimize_essential_graph).

    Vertices are the keyframes, numbered 0 .. n - 1 by the caller.  Scw[v]: vScw, the corrected
    Sim3 where CorrectedSim3 has one, else the pose with scale 1; Snc[v]: the NonCorrectedSim3
    where one exists, else Scw[v] (both SIM3D_DTYPE, or sequences of (q, t, s)).  edges:
    (i, j, kind) per EdgeSim3, vertex 0 = i, vertex 1 = j, kind 0 a LoopConnections edge
    (measurement from Scw), 1 any other (from Snc).  fixed: pLoopKF's index.  Every free vertex
    must be connected to the fixed one.

    Returns (Siw SIM3D_DTYPE [n], Tiw float32 [n, 3, 4] = SetPose's matrices, report dict)."""
    Scw, Snc, e = sim3d_records(Scw), sim3d_records(Snc), eg_edge_records(edges)
    if len(Snc) != len(Scw):
        raise ValueError("Scw and Snc differ in length")
    n = len(Scw)
    Siw = np.zeros(n, L.SIM3D_DTYPE)
    Tiw = np.zeros((n, 3, 4), np.float32)
    rep = L.LmReport()
    L.check(L.lib().orbg_optimize_essential_graph(
        _ctx(device).handle, L.ptr(Scw), L.ptr(Snc), n, L.ptr(e), len(e), int(fixed),
        1 if bFixScale else 0, int(iterations), L.ptr(Siw), L.ptr(Tiw), ctypes.byref(rep)),
        "orbg_optimize_essential_graph")
    return Siw, Tiw, _lm_report(rep)


class EssentialGraph:
    """A planned essential graph (orbg_eg_graph): the elimination order and block pattern are
    made once, optimize() may run many times."""

    def __init__(self, edges, nvert, fixed, device=0):
        self._ctx = _ctx(device)
        self.nvert = int(nvert)
        e = eg_edge_records(edges)
        h = ctypes.c_void_p()
        L.check(L.lib().orbg_eg_graph_create(self._ctx.handle, L.ptr(e), len(e), self.nvert,
                                             int(fixed), ctypes.byref(h)), "orbg_eg_graph_create")
        self.handle = h

    def info(self):
        """(free vertices, blocks of H, blocks of L)."""
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        L.check(L.lib().orbg_eg_graph_info(self.handle, ctypes.byref(a), ctypes.byref(b),
                                           ctypes.byref(c)), "orbg_eg_graph_info")
        return a.value, b.value, c.value

    def optimize(self, Scw, Snc, bFixScale, iterations=20):
        """orbg_eg_graph_optimize from host records (uploaded and downloaded here).  Returns
        (Siw, Tiw, report dict) as OptimizeEssentialGraph."""
        import torch
        Scw, Snc = sim3d_records(Scw), sim3d_records(Snc)
        if len(Scw) != self.nvert or len(Snc) != self.nvert:
            raise ValueError("the graph has %d vertices" % self.nvert)

        def up(a):
            return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        d_c, d_n = up(Scw), up(Snc)
        d_o = torch.zeros(self.nvert * 64, dtype=torch.uint8, device="cuda")
        d_t = torch.zeros(self.nvert * 12, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rep = L.LmReport()
        L.check(L.lib().orbg_eg_graph_optimize(
            self._ctx.handle, self.handle, d_c.data_ptr(), d_n.data_ptr(), 1 if bFixScale else 0,
            int(iterations), d_o.data_ptr(), d_t.data_ptr(), ctypes.byref(rep)),
            "orbg_eg_graph_optimize")
        return (d_o.cpu().numpy().view(L.SIM3D_DTYPE).copy(),
                d_t.cpu().numpy().reshape(self.nvert, 3, 4), _lm_report(rep))

    def close(self):
        if getattr(self, "handle", None):
            L.lib().orbg_eg_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def CorrectMapPoints(Scw, Siw, ref, points, device=0):
    """The map points' correction of OptimizeEssentialGraph (Optimizer.cc:1288-1323,
    orbg_eg_correct_points_device): correctedSwr.map(Srw.map(P)) per point with r = ref[p]
    (mnCorrectedReference where the point was corrected by the current keyframe, else its
    reference keyframe), Srw = Scw[r], correctedSwr = Siw[r]^-1; double arithmetic on the float
    position, rounded once.  Returns float32 [n, 3]."""
    import torch
    Scw, Siw = sim3d_records(Scw), sim3d_records(Siw)
    if len(Scw) != len(Siw):
        raise ValueError("Scw and Siw differ in length")
    ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if len(ref) != len(pts):
        raise ValueError("one reference index per point")
    n = len(pts)
    if n == 0:
        return np.zeros((0, 3), np.float32)

    def up(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    c_ = _ctx(device)
    d_c, d_s, d_r, d_p = up(Scw), up(Siw), up(ref), up(pts)
    d_o = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().orbg_eg_correct_points_device(c_.handle, d_c.data_ptr(), d_s.data_ptr(), len(Scw),
                                                  d_r.data_ptr(), d_p.data_ptr(), n, d_o.data_ptr()),
            "orbg_eg_correct_points_device")
    c_.sync()
    return d_o.cpu().numpy().reshape(n, 3)


TH_HUBER_MONO_GBA = float(np.float32(math.sqrt(5.99)))   # const float thHuber2D (Optimizer.cc:157)
TH_HUBER_STEREO_GBA = float(np.float32(math.sqrt(7.815)))  # const float thHuber3D (:158)


def _stop_flag_address(stop_flag):
    if stop_flag is None:
        return None
    if isinstance(stop_flag, np.ndarray):
        assert stop_flag.dtype == np.uint8 and stop_flag.size >= 1
        return stop_flag.ctypes.data
    return L.C.addressof(stop_flag)


def GlobalBundleAdjustment(poses, points, edges, iterations, stop_flag=None, device=0):
    """The optimisation of Optimizer::BundleAdjustment (Optimizer.cc:113-247,
    orbg_global_ba_optimize): POSE_DTYPE poses (fixed = 1 for the keyframe with mnId 0),
    points [n, 3], EDGE_DTYPE edges (one per observation; huber_delta TH_HUBER_*_GBA and
    robust = bRobust), optimize(iterations) under `stop_flag` (a one-byte host buffer, as
    DeviceLBA.optimize_ctl).  Returns (poses, points, report): copies with the estimates (a
    fixed pose and a point without an active edge unchanged) and a dict of the LM report and
    the sparse plan's figures."""
    poses = np.array(poses, L.POSE_DTYPE)
    points = np.array(points, np.float64).reshape(-1, 3)
    e = np.ascontiguousarray(edges, L.EDGE_DTYPE)
    rep = L.GbaReport()
    ctl = L.LmControl()
    ctl.force_stop = _stop_flag_address(stop_flag)
    L.check(L.lib().orbg_global_ba_optimize(_ctx(device).handle, L.ptr(poses), len(poses),
                                            L.ptr(points), len(points), L.ptr(e), len(e),
                                            int(iterations), L.C.byref(ctl), L.C.byref(rep)),
            "orbg_global_ba_optimize")
    r = rep.lm
    report = dict(iterations=r.iterations, trials=r.trials, terminated=r.terminated,
                  initial_chi2=r.initial_chi2, final_chi2=r.final_chi2, plan=rep.plan.as_dict(),
                  **{"lambda": r.lam})
    return poses, points, report


def CorrectPointsGBA(Tcw_before, Twc_after, ref, points, device=0):
    """The map points global BA did not optimise (LoopClosing.cc:1101-1113,
    orbg_gba_correct_points_device): Rwc (Rcw X + tcw) + twc per point with its reference
    keyframe r = ref[p]: Tcw_before[r] = mTcwBefGBA, Twc_after[r] = GetPoseInverse() (float
    [n, 3, 4] or [n, 4, 4]); ref[p] < 0 leaves the point as it is.  Returns float32 [n, 3]."""
    import torch
    Tb = np.ascontiguousarray(np.asarray(Tcw_before, np.float32)[:, :3, :4])
    Ta = np.ascontiguousarray(np.asarray(Twc_after, np.float32)[:, :3, :4])
    if len(Tb) != len(Ta):
        raise ValueError("Tcw_before and Twc_after differ in length")
    ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if len(ref) != len(pts):
        raise ValueError("one reference index per point")
    n = len(pts)
    if n == 0:
        return np.zeros((0, 3), np.float32)

    def up(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    c_ = _ctx(device)
    d_b, d_a, d_r, d_p = up(Tb), up(Ta), up(ref), up(pts)
    d_o = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().orbg_gba_correct_points_device(c_.handle, d_b.data_ptr(), d_a.data_ptr(), len(Tb),
                                                   d_r.data_ptr(), d_p.data_ptr(), n, d_o.data_ptr()),
            "orbg_gba_correct_points_device")
    c_.sync()
    return d_o.cpu().numpy().reshape(n, 3)


def sparse_symbolic(edges, npose, npoint, fixed):
    """orbg_ba_sparse_symbolic (host only, no GPU): the symbolic factorisation a sparse Schur
    plan makes for these edges (`pose`, `point`, `active` fields) and fixed flags.  Returns
    (order, colptr, rowidx, level, info): the free poses in elimination order, L by columns in
    elimination positions (rows ascending, the diagonal first), each column's level, and the
    info dict."""
    ep = np.ascontiguousarray(edges["pose"], np.int32)
    eq = np.ascontiguousarray(edges["point"], np.int32)
    ea = np.ascontiguousarray(np.asarray(edges["active"]) != 0, np.uint8)
    f = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
    if len(f) != npose:
        raise ValueError("one fixed flag per pose")
    info = L.BaSparseInfo()
    args = (L.ptr(ep), L.ptr(eq), L.ptr(ea), len(ep), int(npose), int(npoint), L.ptr(f))
    L.check(L.lib().orbg_ba_sparse_symbolic(*args, None, None, None, 0, None, L.C.byref(info)),
            "orbg_ba_sparse_symbolic")
    n, nl = info.nfree, info.l_blocks
    order = np.zeros(max(n, 1), np.int32)
    colptr = np.zeros(n + 1, np.int32)
    rowidx = np.zeros(max(nl, 1), np.int32)
    level = np.zeros(max(n, 1), np.int32)
    L.check(L.lib().orbg_ba_sparse_symbolic(*args, L.ptr(order), L.ptr(colptr), L.ptr(rowidx), nl,
                                            L.ptr(level), L.C.byref(info)),
            "orbg_ba_sparse_symbolic")
    return order[:n], colptr, rowidx[:nl], level[:n], info.as_dict()


def vertex_csr(edges, field, nvert):
    """Edge lists per vertex (CSR): (off[nvert+1], edge ids[nedge]) int32, edges in input
    order within a vertex -- the layout orbg_ba_linearize_device reduces blocks over."""
    v = np.asarray(edges[field], np.int64)
    order = np.argsort(v, kind="stable").astype(np.int32)
    off = np.zeros(nvert + 1, np.int64)
    np.add.at(off, v + 1, 1)
    return np.cumsum(off).astype(np.int32), order


class DeviceLBA:
    """Device-resident batch of LBA windows (one graph; windows are independent blocks of
    it): uploads once, then linearize() runs orbg_ba_linearize_device on the context stream
    with every array in HBM -- the per-iteration work of g2o's computeActiveErrors +
    buildSystem."""

    def __init__(self, poses, points, edges, device=0, jacobians=True, edge_errors=True,
                 graph=False):
        import torch
        self.ctx = _ctx(device)
        self.graph = None  # orbg_ba_graph (packed edges in HBM): build_system / errors use it
        if graph:
            e = np.ascontiguousarray(edges, L.EDGE_DTYPE)
            h = L.C.c_void_p()
            L.check(L.lib().orbg_ba_graph_create(self.ctx.handle, e.ctypes.data, len(e), len(poses),
                                                 len(points), L.C.byref(h)),
                    "orbg_ba_graph_create")
            self.graph = h
        self.jacobians = bool(jacobians)  # eout.jp / jt stored (orbg_ba_set_jacobians)
        self.edge_errors = bool(edge_errors)  # eout.err / chi2 / rho1 (orbg_ba_set_edge_errors)
        self.np, self.nq, self.ne = len(poses), len(points), len(edges)
        off, pe = vertex_csr(edges, "pose", self.np)
        qoff, qe = vertex_csr(edges, "point", self.nq)
        dev = torch.device("cuda", device)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)

        self.d_poses = up(np.ascontiguousarray(poses, L.POSE_DTYPE))
        self.d_points = up(np.ascontiguousarray(points, np.float64))
        self.d_edges = up(np.ascontiguousarray(edges, L.EDGE_DTYPE))
        self.d_off, self.d_pe = up(off), up(pe)
        self.d_qoff, self.d_qe = up(qoff), up(qe)
        self.d_eout = torch.zeros(self.ne * L.EDGE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_hpose = torch.zeros((self.np, 6, 6), dtype=torch.float64, device=dev)
        self.d_bpose = torch.zeros((self.np, 6), dtype=torch.float64, device=dev)
        self.d_hpoint = torch.zeros((self.nq, 3, 3), dtype=torch.float64, device=dev)
        self.d_bpoint = torch.zeros((self.nq, 3), dtype=torch.float64, device=dev)
        self.d_chi2 = torch.zeros(max(self.ne, 1), dtype=torch.float64, device=dev)
        self.d_rho0 = torch.zeros(max(self.ne, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)

    def linearize(self):
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        L.check(L.lib().orbg_ba_set_jacobians(self.ctx.handle, 1 if self.jacobians else 0),
                "orbg_ba_set_jacobians")
        L.check(L.lib().orbg_ba_set_edge_errors(self.ctx.handle, 1 if self.edge_errors else 0),
                "orbg_ba_set_edge_errors")
        L.check(L.lib().orbg_ba_linearize_device(
            self.ctx.handle, p(self.d_poses), self.np, p(self.d_points), self.nq, p(self.d_edges),
            self.ne, p(self.d_off), p(self.d_pe), p(self.d_qoff), p(self.d_qe), p(self.d_eout),
            p(self.d_hpose),
            p(self.d_bpose), p(self.d_hpoint), p(self.d_bpoint)), "orbg_ba_linearize_device")

    def build_system(self):
        """buildSystem alone (orbg_ba_build_system_device): the vertex blocks and H_pl into the
        compact self.d_hpl [nedge][3][6], no per-edge Jacobian / error record (the error pass
        supplies those): the per-iteration pair of a device-resident LM is build_system() +
        errors()."""
        import torch
        if getattr(self, "d_hpl", None) is None:
            self.d_hpl = torch.zeros((max(self.ne, 1), 3, 6), dtype=torch.float64,
                                     device=self.d_hpose.device)
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        if self.graph is not None:
            L.check(L.lib().orbg_ba_graph_build_system(
                self.ctx.handle, self.graph, p(self.d_poses), p(self.d_points), p(self.d_hpl),
                p(self.d_hpose), p(self.d_bpose), p(self.d_hpoint), p(self.d_bpoint)),
                "orbg_ba_graph_build_system")
            return
        L.check(L.lib().orbg_ba_build_system_device(
            self.ctx.handle, p(self.d_poses), self.np, p(self.d_points), self.nq, p(self.d_edges),
            self.ne, p(self.d_off), p(self.d_pe), p(self.d_qoff), p(self.d_qe), p(self.d_hpl),
            p(self.d_hpose), p(self.d_bpose), p(self.d_hpoint), p(self.d_bpoint)),
            "orbg_ba_build_system_device")

    def errors(self):
        """The per-trial error pass (orbg_ba_errors_device): chi2 and the robust term of every
        edge into self.d_chi2 / self.d_rho0."""
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        if self.graph is not None:
            L.check(L.lib().orbg_ba_graph_errors(self.ctx.handle, self.graph, p(self.d_poses),
                                                 p(self.d_points), None, p(self.d_chi2),
                                                 p(self.d_rho0), None), "orbg_ba_graph_errors")
            return
        L.check(L.lib().orbg_ba_errors_device(self.ctx.handle, p(self.d_poses), p(self.d_points),
                                              p(self.d_edges), self.ne, None, p(self.d_chi2),
                                              p(self.d_rho0), None), "orbg_ba_errors_device")

    def set_active(self, active):
        """The outlier pass's setLevel (Optimizer.cc:871-901) on the graph: active[e] per edge."""
        a = np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
        if self.graph is None:
            raise ValueError("set_active needs a DeviceLBA built with graph=True")
        L.check(L.lib().orbg_ba_graph_set_active(self.ctx.handle, self.graph, a.ctypes.data),
                "orbg_ba_graph_set_active")

    def schur_plan(self, fixed, sparse=False):
        """orbg_ba_graph_schur_plan: the Schur structure of the graph for the free poses
        (fixed[i] != 0: g2o's fixed vertex), built once; set_active rebuilds it.  sparse=True:
        orbg_ba_graph_schur_plan_sparse, the block-sparse reduced camera system of a global
        BA; returns the plan's info dict (nfree, s_blocks, l_blocks, levels, tail_columns,
        updates)."""
        import torch
        if self.graph is None:
            raise ValueError("schur_plan needs a DeviceLBA built with graph=True")
        f = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
        info = None
        if sparse:
            si = L.BaSparseInfo()
            L.check(L.lib().orbg_ba_graph_schur_plan_sparse(self.ctx.handle, self.graph,
                                                            f.ctypes.data, L.C.byref(si)),
                    "orbg_ba_graph_schur_plan_sparse")
            info = si.as_dict()
        else:
            L.check(L.lib().orbg_ba_graph_schur_plan(self.ctx.handle, self.graph, f.ctypes.data),
                    "orbg_ba_graph_schur_plan")
        dev = self.d_hpose.device
        self.d_dx_pose = torch.zeros((self.np, 6), dtype=torch.float64, device=dev)
        self.d_dx_point = torch.zeros((self.nq, 3), dtype=torch.float64, device=dev)
        self.d_ok = torch.zeros(1, dtype=torch.int32, device=dev)
        return info

    def schur_solve(self, lam):
        """BlockSolver<6,3>::solve on the device blocks of the last build_system()
        (orbg_ba_graph_schur_solve): increments into self.d_dx_pose / self.d_dx_point,
        self.d_ok, on the context stream with no host copy."""
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        L.check(L.lib().orbg_ba_graph_schur_solve(
            self.ctx.handle, self.graph, float(lam), p(self.d_hpl), p(self.d_hpose),
            p(self.d_bpose), p(self.d_hpoint), p(self.d_bpoint), p(self.d_dx_pose),
            p(self.d_dx_point), p(self.d_ok)), "orbg_ba_graph_schur_solve")

    def set_robust(self, robust):
        """setRobustKernel per edge (orbg_ba_graph_set_robust): robust[e] != 0 keeps Huber."""
        r = np.ascontiguousarray(np.asarray(robust) != 0, np.uint8)
        L.check(L.lib().orbg_ba_graph_set_robust(self.ctx.handle, self.graph, r.ctypes.data),
                "orbg_ba_graph_set_robust")

    def update(self):
        """SparseOptimizer::update with the last schur_solve's increments, in place on the
        device estimates (orbg_ba_update_device; fixed poses untouched)."""
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        L.check(L.lib().orbg_ba_update_device(
            self.ctx.handle, p(self.d_poses), self.np, p(self.d_points), self.nq,
            p(self.d_dx_pose), p(self.d_dx_point), p(self.d_poses), p(self.d_points)),
            "orbg_ba_update_device")

    def optimize(self, iterations):
        """optimizer.optimize(iterations) (Optimizer.cc:857, :905) with g2o's
        Levenberg-Marquardt on the device estimates (orbg_ba_graph_optimize): build, Schur
        solve, update and error pass per trial on the context stream, three scalars read
        back per trial.  Needs schur_plan(fixed).  Returns the orbg_lm_report as a dict."""
        if self.graph is None:
            raise ValueError("optimize needs a DeviceLBA built with graph=True")
        return self.optimize_ctl(iterations)

    def optimize_ctl(self, iterations, stop_flag=None, post_iteration=None, post_trial=None,
                     last_chi2=None):
        """optimize(iterations) with g2o's force-stop flag (orbg_ba_graph_optimize_ctl):
        `stop_flag` a one-byte host buffer (e.g. numpy uint8 [1], or ctypes c_bool) polled
        before every iteration and after every trial as SparseOptimizer::terminate()
        (sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149);
        `post_iteration(it)` / `post_trial(it, trial)` Python callbacks (they may raise the
        flag); `last_chi2` a float64 CUDA tensor [nedge] that receives the chi2 g2o's edges
        hold afterwards (the last trial's).  Returns the report as a dict (terminated 3 =
        stopped by the flag)."""
        if self.graph is None:
            raise ValueError("optimize needs a DeviceLBA built with graph=True")
        rep = L.LmReport()
        ctl = L.LmControl()
        if stop_flag is not None:
            if isinstance(stop_flag, np.ndarray):
                assert stop_flag.dtype == np.uint8 and stop_flag.size >= 1
                ctl.force_stop = stop_flag.ctypes.data
            else:
                ctl.force_stop = L.C.addressof(stop_flag)
        # keep the thunks alive for the call
        pi = L.LM_POST_ITERATION((lambda u, it: post_iteration(it)) if post_iteration else 0)
        pt = L.LM_POST_TRIAL((lambda u, it, tr: post_trial(it, tr)) if post_trial else 0)
        ctl.post_iteration, ctl.post_trial = pi, pt
        if last_chi2 is not None:
            import torch
            assert last_chi2.dtype == torch.float64 and last_chi2.is_cuda
            assert last_chi2.numel() == self.ne
            ctl.d_last_chi2 = last_chi2.data_ptr()
        p = lambda t: L.C.c_void_p(t.data_ptr())  # noqa: E731
        L.check(L.lib().orbg_ba_graph_optimize_ctl(self.ctx.handle, self.graph, p(self.d_poses),
                                                   p(self.d_points), int(iterations),
                                                   L.C.byref(ctl), L.C.byref(rep)),
                "orbg_ba_graph_optimize_ctl")
        return dict(iterations=rep.iterations, trials=rep.trials, terminated=rep.terminated,
                    initial_chi2=rep.initial_chi2, final_chi2=rep.final_chi2,
                    **{"lambda": rep.lam})

    def estimates(self):
        """(poses, points) of the device estimates, host copies."""
        self.ctx.sync()
        poses = np.frombuffer(self.d_poses.cpu().numpy().tobytes(), L.POSE_DTYPE).copy()
        points = np.frombuffer(self.d_points.cpu().numpy().tobytes(), np.float64).reshape(-1, 3).copy()
        return poses, points

    def __del__(self):
        if getattr(self, "graph", None) is not None:
            L.lib().orbg_ba_graph_destroy(self.graph)
            self.graph = None

    def download(self):
        self.ctx.sync()
        eo = np.frombuffer(self.d_eout.cpu().numpy().tobytes(), L.EDGE_OUT_DTYPE)
        return (eo, self.d_hpose.cpu().numpy(), self.d_bpose.cpu().numpy(),
                self.d_hpoint.cpu().numpy(), self.d_bpoint.cpu().numpy())
