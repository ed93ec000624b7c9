"""GPU: Optimizer::LocalBundleAdjustment on the device Map through the C ABI against
tests/ref_lba_map.py, the independent pure-Python statement.

The window is compared exactly: lists, counts, flags, every orbg_edge field, and the vertices'
estimates bit for bit (IEEE add / mul / div / sqrt in one fixed order on both sides).  The
write-back with flags chosen by hand: every row, flag, reference keyframe and Observations()
exactly, the stored poses, centres and positions bit for bit, normals and depths at
ref_map.check_normal_depth_bounds' bars.  The chain against orbg_local_ba_optimize fed the
reference-built window (the same code on the same inputs: the report bit for bit) and the
reference model's write-back of its outputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from orb_slam2_test_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_lba_map as RB  # noqa: E402
import ref_map_edit as RE  # noqa: E402
import test_gpu_culling as TC  # noqa: E402
import test_gpu_loop_correct as TGL  # noqa: E402
import test_lba_map_ref as TR  # noqa: E402
import test_oracle_mapping as T  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


class GpuLbaMap(TGL.GpuLoopMap):
    """tests/ref_lba_map.py's duck-typed interface over the library's Map"""

    def lba_window(self, slot):
        return self.m.LbaWindow(slot)

    def lba_apply(self, w, poses, points, erase, cams=None):
        return self.m.LbaApply(w, poses, points, erase, cams)

    def cams_ptr(self):
        return self.attached[4].data_ptr()

    def cams_host(self):
        import torch
        torch.cuda.synchronize()
        return np.frombuffer(self.attached[4].cpu().numpy().tobytes(), L.FRUSTUM_DTYPE)


def assert_window_equal(got, want):
    assert got["nlocal"] == want["nlocal"]
    assert got["kf_slots"].tolist() == want["kf_slots"].tolist()
    assert got["point_ids"].tolist() == want["point_ids"].tolist()
    assert got["edge_feat"].tolist() == want["edge_feat"].tolist()
    for key in RB.EDGE_DTYPE.names:
        assert np.array_equal(got["edges"][key], want["edges"][key]), key
    assert got["edges"].tobytes() == want["edges"].tobytes()
    assert got["points"].tobytes() == want["points"].tobytes()
    assert got["poses"]["fixed"].tolist() == want["poses"]["fixed"].tolist()
    assert got["poses"].tobytes() == want["poses"].tobytes()


def float_state(G, nkf, npts):
    T_, has, ids, c = G.get_poses(nkf)
    return T_, has.tolist(), c, G.records(npts)


def assert_floats_equal(G, M, nkf, npts, moved):
    """poses, centres and positions bit for bit; normals and depths of the moved points at
    check_normal_depth_bounds' bars against the float64 statement; everything else bit for bit"""
    Tg, hg, cg, rg = float_state(G, nkf, npts)
    Tr, hr, _, cr = M.get_poses(nkf)
    rr = M.records(npts)
    assert hg == hr.tolist()
    assert Tg.tobytes() == Tr.tobytes() and cg.tobytes() == cr.tobytes()
    for key in ("x", "y", "z", "flags"):
        assert np.array_equal(rg[key], rr[key]), key
    moved = set(int(p) for p in moved)
    still = [p for p in range(npts) if p not in moved]
    assert rg[still].tobytes() == rr[still].tobytes()
    n_checked = 0
    for p in sorted(moved):
        nd = M.normal_and_depth64(p)
        if nd is None:
            assert rg[p].tobytes() == rr[p].tobytes()
            continue
        nrm, mind, maxd = nd
        g = rg[p]
        nobs = len(M.observations(p))
        assert np.all(np.abs(np.array([g["nx"], g["ny"], g["nz"]], np.float64) - nrm)
                      <= (nobs + 4) * EPS), p
        assert abs(float(g["min_dist"]) - mind) <= 8 * EPS * mind, p
        assert abs(float(g["max_dist"]) - maxd) <= 8 * EPS * maxd, p
        n_checked += 1
    return n_checked


# ---------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(RB.HAND_WINDOWS)), ids=RB.HAND_WINDOW_NAMES)
def test_hand_window(case):
    fn, expected = RB.HAND_WINDOWS[case]
    G = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    assert fn(G) == expected
    M = RB.RefLbaMap()
    fn(M)
    slot = expected[0][0] if case else expected[1][0][0]
    assert_window_equal(G.lba_window(slot), M.lba_window(slot))


@pytest.mark.parametrize("name", sorted(RB.SCENES))
def test_scene_window(name):
    d, M, want = TR.ref_scene(name)
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    before = (RB.state(G, RB.MAX_KF, d["npts"]), [a.tobytes() for a in float_state(G, RB.MAX_KF, d["npts"])[::2]])
    got = G.lba_window(d["cur"])
    assert_window_equal(got, want)
    assert G.m.lba_counts == [want["nlocal"], len(want["kf_slots"]), len(want["point_ids"]),
                              len(want["edges"])]
    after = (RB.state(G, RB.MAX_KF, d["npts"]), [a.tobytes() for a in float_state(G, RB.MAX_KF, d["npts"])[::2]])
    assert after == before                               # the window reads, it writes nothing


def test_window_device_form():
    """orbg_map_lba_window_device into the caller's device arrays, a second call of the same
    size, and the status word"""
    import torch
    d, M, want = TR.ref_scene("small")
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    pc, qc, ec = 16, 1024, 8192

    def buf(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ks, po, ids, pts = buf(pc * 4), buf(pc * 64), buf(qc * 4), buf(qc * 24)
    ed, ef, cnt, st = buf(ec * L.EDGE_DTYPE.itemsize), buf(ec * 4), buf(16), buf(16)
    torch.cuda.synchronize()
    for _ in range(2):
        G.m.lba_window_device(d["cur"], ks.data_ptr(), po.data_ptr(), pc, ids.data_ptr(),
                              pts.data_ptr(), qc, ed.data_ptr(), ef.data_ptr(), ec, cnt.data_ptr(),
                              st.data_ptr())
        TC.ctx().sync()
        c = np.frombuffer(cnt.cpu().numpy().tobytes(), np.int32)
        assert c.tolist() == [want["nlocal"], len(want["kf_slots"]), len(want["point_ids"]),
                              len(want["edges"])]
        assert np.frombuffer(st.cpu().numpy().tobytes(), np.int32)[0] == 0
        got = dict(nlocal=int(c[0]),
                   kf_slots=np.frombuffer(ks.cpu().numpy().tobytes(), np.int32)[:c[1]],
                   poses=np.frombuffer(po.cpu().numpy().tobytes(), L.POSE_DTYPE)[:c[1]],
                   point_ids=np.frombuffer(ids.cpu().numpy().tobytes(), np.int32)[:c[2]],
                   points=np.frombuffer(pts.cpu().numpy().tobytes(), np.float64).reshape(-1, 3)[:c[2]],
                   edges=np.frombuffer(ed.cpu().numpy().tobytes(), L.EDGE_DTYPE)[:c[3]],
                   edge_feat=np.frombuffer(ef.cpu().numpy().tobytes(), np.int32)[:c[3]])
        assert_window_equal(got, want)


# ---------------------------------------------------------------------------
# the write-back, flags chosen by hand
# ---------------------------------------------------------------------------
def test_hand_apply():
    M = RB.RefLbaMap()
    w_r, counts_r, _, _ = RB.hand_apply(M)
    G = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    w_g, counts_g, _, _ = RB.hand_apply(G)
    assert_window_equal(w_g, w_r)
    assert counts_g == counts_r == RB.HAND_APPLY
    assert RB.state(G, RB.HAND_K, RB.HAND_POINTS) == RB.state(M, RB.HAND_K, RB.HAND_POINTS)
    want = RB.HAND_APPLY_STATE
    assert G.point_bad(0, 7) == want["bad"] and G.point_refs(0, 7) == want["ref"]
    assert [s[3] for s in G.point_stats(0, 7)] == want["nobs"]
    for s, row in want["rows"].items():
        assert G.keyframe_points(s)[:len(row)] == row
    assert assert_floats_equal(G, M, RB.HAND_K, RB.HAND_POINTS, w_r["point_ids"]) >= 15
    # a later UpdateConnections reads the rebuilt index
    for s in range(5):
        G.update_connections(s)
        M.update_connections(s)
    assert RB.state(G, RB.HAND_K, RB.HAND_POINTS) == RB.state(M, RB.HAND_K, RB.HAND_POINTS)


def test_apply_writes_the_cameras():
    M = RB.RefLbaMap()
    G = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    RB.hand_main(M)
    RB.hand_main(G)
    w = M.lba_window(2)
    poses = np.array(w["poses"])
    poses["t"] += 0.25
    erase = np.zeros(len(w["edges"]), np.uint8)
    cams_r = np.array(M.d["cams"])
    before = G.cams_host().copy()
    assert G.lba_apply(w, poses, w["points"], erase, G.cams_ptr()) == (0, 0)
    assert M.lba_apply(w, poses, w["points"], erase, cams_r) == (0, 0)
    after = G.cams_host()
    assert after.tobytes() == cams_r.tobytes() and after.tobytes() != before.tobytes()
    local = w["kf_slots"][:w["nlocal"]].tolist()
    rest = [s for s in range(RB.HAND_K) if s not in local]
    assert after[rest].tobytes() == before[rest].tobytes()
    assert_floats_equal(G, M, RB.HAND_K, RB.HAND_POINTS, w["point_ids"])


# ---------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------
def lib_optimize(w, stop_flag=None, post_iteration=None):
    """orbg_local_ba_optimize on a window: (poses, points, erase, LbaReport)"""
    poses, points = np.array(w["poses"]), np.array(w["points"])
    edges = np.ascontiguousarray(w["edges"])
    erase = np.zeros(max(len(edges), 1), np.uint8)
    rep, ctl = L.LbaReport(), L.LmControl()
    if stop_flag is not None:
        ctl.force_stop = stop_flag.ctypes.data
    pi = L.LM_POST_ITERATION((lambda u, it: post_iteration(it)) if post_iteration else 0)
    ctl.post_iteration = pi
    L.check(L.lib().orbg_local_ba_optimize(TC.ctx().handle, L.ptr(poses), len(poses), L.ptr(points),
                                           len(points), L.ptr(edges), len(edges), C.byref(ctl), None,
                                           None, L.ptr(erase), C.byref(rep)),
            "orbg_local_ba_optimize")
    return poses, points, erase[:len(edges)], rep


def lm_tuple(r):
    return (r.iterations, r.trials, r.terminated, r.initial_chi2, r.final_chi2, r.lam)


def assert_report(got, rep, w, nerased, nbad):
    assert got["stopped"] == 0
    assert (got["nlocal"], got["nfixed"], got["npoints"], got["nedges"]) == (
        w["nlocal"], len(w["kf_slots"]) - w["nlocal"], len(w["point_ids"]), len(w["edges"]))
    for k in range(2):
        g = got["lm"][k]
        assert (g["iterations"], g["trials"], g["terminated"], g["initial_chi2"], g["final_chi2"],
                g["lam"]) == lm_tuple(rep.lm[k]), k
    assert (got["do_more"], got["n_outliers"], got["n_erase"]) == (rep.do_more, rep.n_outliers,
                                                                   rep.n_erase)
    assert (got["nerased"], got["npoints_bad"]) == (nerased, nbad)


_chain_cache = {}


def chain_reference(name):
    """the reference model after orbg_local_ba_optimize's outputs on its own window: computed
    once, left unchanged"""
    if name not in _chain_cache:
        import copy
        d, M0, w = TR.ref_scene(name)
        P, X, erase, rep = lib_optimize(w)
        M = copy.deepcopy(M0)
        refs = {int(p): M.mp[int(p)]["ref"] for p in w["point_ids"]}
        cams = np.array(d["cams"])
        nerased, nbad = M.lba_apply(w, P, X, erase, cams)
        handed = sum(1 for p, r in refs.items() if not M.mp[p]["bad"] and M.mp[p]["ref"] != r)
        _chain_cache[name] = (M, rep, nerased, nbad, handed, cams)
    return _chain_cache[name]


@pytest.mark.parametrize("name", sorted(RB.SCENES))
def test_chain(name):
    d, _, w = TR.ref_scene(name)
    M, rep, nerased, nbad, handed, cams = chain_reference(name)
    assert nerased >= 1 and nbad >= 1 and handed >= 1 and len(w["kf_slots"]) > w["nlocal"]
    assert rep.do_more == 1 and rep.lm[0].iterations >= 1
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    got = G.m.LocalBundleAdjustment(d["cur"], d_cams_out=G.cams_ptr())
    assert_report(got, rep, w, nerased, nbad)
    assert RB.state(G, RB.MAX_KF, d["npts"]) == RB.state(M, RB.MAX_KF, d["npts"])
    n = assert_floats_equal(G, M, RB.MAX_KF, d["npts"], w["point_ids"])
    assert n > 0.9 * (len(w["point_ids"]) - nbad)
    assert G.cams_host()[:d["nkf"]].tobytes() == cams.tobytes()
    # a second call of the same size on the changed map: the workspace is reused
    w2 = M.lba_window(d["cur"])
    got2 = G.m.LocalBundleAdjustment(d["cur"])
    assert (got2["npoints"], got2["nedges"]) == (len(w2["point_ids"]), len(w2["edges"]))


def test_stopped_before():
    d, _, w = TR.ref_scene("small")
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    before = (RB.state(G, RB.MAX_KF, d["npts"]), [a if isinstance(a, list) else a.tobytes()
                                                    for a in float_state(G, RB.MAX_KF, d["npts"])])
    flag = np.ones(1, np.uint8)
    got = G.m.LocalBundleAdjustment(d["cur"], stop_flag=flag, d_cams_out=G.cams_ptr())
    assert got["stopped"] == 1 and got["nedges"] == len(w["edges"]) and got["nerased"] == 0
    assert got["lm"][0]["iterations"] == 0 and got["do_more"] == 0
    after = (RB.state(G, RB.MAX_KF, d["npts"]), [a if isinstance(a, list) else a.tobytes()
                                                   for a in float_state(G, RB.MAX_KF, d["npts"])])
    assert after == before
    assert G.cams_host()[:d["nkf"]].tobytes() == np.array(d["cams"]).tobytes()


def test_stopped_after_optimize5():
    """the flag goes up in optimize(5)'s last postIteration: bDoMore is false, no outlier pass, no
    optimize(10), and the write-back still runs (Optimizer.cc:859-978)"""
    import copy
    d, M0, w = TR.ref_scene("small")
    last = lib_optimize(w)[3].lm[0].iterations - 1       # optimize(5)'s last iteration
    assert last >= 1

    def run(call):
        flag = np.zeros(1, np.uint8)
        seen = []

        def hook(it):
            seen.append(it)
            if it == last:
                flag[0] = 1
        return call(flag, hook), seen
    (P, X, erase, rep), seen_r = run(lambda f, h: lib_optimize(w, f, h))
    assert seen_r == list(range(last + 1)) and rep.do_more == 0 and rep.lm[1].iterations == 0
    M = copy.deepcopy(M0)
    nerased, nbad = M.lba_apply(w, P, X, erase)
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    got, seen_g = run(lambda f, h: G.m.LocalBundleAdjustment(d["cur"], stop_flag=f, post_iteration=h))
    assert seen_g == seen_r
    assert_report(got, rep, w, nerased, nbad)
    assert got["do_more"] == 0 and nerased >= 1
    assert RB.state(G, RB.MAX_KF, d["npts"]) == RB.state(M, RB.MAX_KF, d["npts"])
    assert_floats_equal(G, M, RB.MAX_KF, d["npts"], w["point_ids"])


def test_empty_edge_set_still_applies():
    M = RB.RefLbaMap()
    G = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    RB.hand_empty_current(M)
    RB.hand_empty_current(G)
    T0 = np.array(RB.RL.eye_pose((1.5, 0.0, 0.0)))
    T0[0, 0] = np.float32(1.0 - 2.0 ** -23)              # re-rounded through the quaternion
    for X in (M, G):
        X.set_poses([3], [T0])
    w = M.lba_window(3)
    M.lba_apply(w, w["poses"], w["points"], np.zeros(0, np.uint8))
    got = G.m.LocalBundleAdjustment(3)
    assert (got["nlocal"], got["nfixed"], got["npoints"], got["nedges"], got["stopped"]) == (1, 0, 0, 0, 0)
    assert got["lm"][0]["iterations"] == 0
    assert_floats_equal(G, M, RB.HAND_K, RB.HAND_POINTS, [])


def test_run_on_map_two_keyframes(oracle):
    """LocalMapping.RunOnMap(local_bundle_adjustment=True) for two consecutive keyframes with
    d_cams_out: the second SearchInNeighbors projects with the poses the first call wrote"""
    import copy
    from orb_slam2_test_amd.localmapping import LocalMapping
    d, M0, _ = TR.ref_scene("small")
    M = copy.deepcopy(M0)
    sf, isg = T._fuse_tables(oracle)
    M.search = RE.make_search(oracle.fuse_search, sf, isg)
    M.d = dict(M.d, cams=np.array(d["cams"]))
    G = GpuLbaMap(RB.MAX_KF, d["cap"], d["npts"])
    RB.build_lba_map(G, d)
    lm = LocalMapping()
    mono = not d["stereo"]
    for slot in (d["cur"] - 1, d["cur"]):
        kfid = d["mnid"][slot]
        recent, targets, nfused, second, recs = lm.RunOnMap(G.m, slot, kfid, mono, [],
                                                            local_bundle_adjustment=True,
                                                            d_cams_out=G.cams_ptr())
        want_sin = M.search_in_neighbors(slot, kfid, mono)
        assert (targets, nfused, second) == tuple(want_sin)
        w = M.lba_window(slot)
        P, X, erase, rep = lib_optimize(w)
        nerased, nbad = M.lba_apply(w, P, X, erase, M.d["cams"])
        assert_report(lm.lba_report, rep, w, nerased, nbad)
        want_cull = M.keyframe_culling(slot, mono)
        assert [tuple(int(v) for v in r) for r in recs.tolist()] == want_cull
        assert RE.state(G, RB.MAX_KF, d["npts"]) == RE.state(M, RB.MAX_KF, d["npts"])
        assert G.cams_host()[:d["nkf"]].tobytes() == M.d["cams"].tobytes()
    assert G.cams_host()[:d["nkf"]].tobytes() != np.array(d["cams"]).tobytes()


# ---------------------------------------------------------------------------
# error paths: the Map compares equal to its state before
# ---------------------------------------------------------------------------
def test_error_paths():
    lib, c = L.lib(), TC.ctx().handle
    G = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    RB.hand_main(G)
    h = G.m.handle
    rep = L.MapLbaReport()

    def snap():
        return (RB.state(G, RB.HAND_K, RB.HAND_POINTS),
                [a if isinstance(a, list) else a.tobytes()
                 for a in float_state(G, RB.HAND_K, RB.HAND_POINTS)])
    before = snap()
    # caps: ORBG_ERANGE with the full counts
    for caps in ((4, 64, 64), (8, 18, 64), (8, 64, 54)):
        with pytest.raises(L.OrbgError) as ei:
            G.m.LbaWindow(2, *caps)
        assert ei.value.code == L.ORBG_ERANGE and G.m.lba_counts == [3, 5, 19, 55]
    assert len(G.m.LbaWindow(2, 5, 19, 55)["edges"]) == 55
    # a dead slot, a slot out of range
    assert lib.orbg_map_local_ba(c, h, 7, None, None, C.byref(rep)) == L.ORBG_EINVAL
    assert lib.orbg_map_local_ba(c, h, 8, None, None, C.byref(rep)) == L.ORBG_EINVAL
    assert lib.orbg_map_local_ba(c, h, 2, None, None, None) == L.ORBG_EINVAL
    with pytest.raises(L.OrbgError):
        G.m.LbaWindow(7)
    # a fixed camera without a pose
    H = GpuLbaMap(RB.HAND_K, RB.HAND_CAP, RB.HAND_POINTS)
    RB.hand_no_fixed(H)
    H.set_keyframe(4, [3])
    before_h = RB.state(H, RB.HAND_K, RB.HAND_POINTS)
    assert lib.orbg_map_local_ba(c, H.m.handle, 1, None, None, C.byref(rep)) == L.ORBG_EINVAL
    with pytest.raises(L.OrbgError):
        H.m.LbaWindow(1)
    assert RB.state(H, RB.HAND_K, RB.HAND_POINTS) == before_h
    # a feature index past the attached count: row 0 has 16 features, 8 keypoints are attached
    H.set_poses([4], [RB.RL.eye_pose((2.0, 0.0, 0.0))])
    assert len(H.m.LbaWindow(1)["kf_slots"]) == 3
    kps = [np.zeros(8, RE.KP_DTYPE)] * RB.HAND_K
    H.attach(dict(kdesc=[np.zeros((8, 32), np.uint8)] * RB.HAND_K, kps=kps,
                  uright=[np.full(8, -1, np.float32)] * RB.HAND_K,
                  cams=np.zeros(RB.HAND_K, RE.FRUSTUM_DTYPE)))
    assert lib.orbg_map_local_ba(c, H.m.handle, 1, None, None, C.byref(rep)) == L.ORBG_EINVAL
    # nothing attached
    G.m.AttachKeyFrames(None, None, None, None, 0, None)
    assert lib.orbg_map_local_ba(c, h, 2, None, None, C.byref(rep)) == L.ORBG_EINVAL
    with pytest.raises(L.OrbgError):
        G.m.LbaWindow(2)
    assert snap() == before
