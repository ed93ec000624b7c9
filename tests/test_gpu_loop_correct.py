"""GPU: the Map's CorrectLoop state (poses, mnId, loop edges, mnCorrectedByKF / Reference), the
Sim3 propagation with its map-point loop, the loop fusion, SearchAndFuse, LoopConnections, the
essential-graph walk, Apply and CorrectLoop in one call through the C ABI against
tests/ref_loop_correct.py, the independent pure-Python statement.  Everything discrete is compared
exactly after every stage: the set and its order, every row, point flags, mpReplaced, the
mnCorrected fields, W, ordered lists, parents, the LoopConnections pairs, the loop edges.  The
floating-point outputs at the bars the project uses for the same arithmetic elsewhere
(test_gpu_essential.py, ref_map.check_normal_depth_bounds)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from orb_slam2_test_amd import _lib as L
from orb_slam2_test_amd import map as MAP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_essential as E  # noqa: E402
import ref_loop_correct as RL  # noqa: E402
import ref_map_edit as RE  # noqa: E402
import ref_sim3opt as RS  # noqa: E402
import test_gpu_culling as TC  # noqa: E402
import test_gpu_map_edit as TE  # noqa: E402
import test_loop_correct_ref as TL  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


class GpuLoopMap(TE.GpuEditMap):
    """tests/ref_loop_correct.py's duck-typed interface over the library's Map"""

    def set_poses(self, slots, Tcw=None, mnid=None):
        self.m.SetPoses(slots, None if Tcw is None else np.asarray(Tcw, np.float32), mnid)

    def get_poses(self, n):
        return self.m.poses(0, n)

    def add_loop_edge(self, a, b):
        self.m.AddLoopEdge(a, b)

    def get_loop_edges(self, s):
        return self.m.GetLoopEdges(s)

    def corrected(self, n):
        a, b = self.m.corrected(0, n)
        return a.tolist(), b.tolist()

    def point_pos(self, p):
        r = self.m.points(p, 1)[0]
        return (float(r["x"]), float(r["y"]), float(r["z"]))

    def point_normal_depth(self, p):
        r = self.m.points(p, 1)[0]
        return (float(r["nx"]), float(r["ny"]), float(r["nz"]), float(r["max_dist"]))

    def records(self, npts):
        return self.m.points(0, npts)

    def propagate(self, cur, Scw):
        members, co, nc = self.m.Propagate(cur, Scw)
        self.tables = (co, nc)

        def rec(t, s):
            return (t["q"][s][None].copy(), t["t"][s][None].copy(), t["s"][s:s + 1].copy())
        return members, {s: rec(co, s) for s in members}, {s: rec(nc, s) for s in members}

    def loop_connections(self, members):
        return [tuple(p) for p in self.m.LoopConnections(members).tolist()]

    def set_corrected(self, first, by, ref):
        self.m.SetCorrected(first, by, ref)

    def apply_correction(self, cur, verts, Scw, Siw, Tiw):
        def recs(S):
            out = np.zeros(len(S), L.SIM3D_DTYPE)
            for k, (q, t, s) in enumerate(S):
                out["q"][k], out["t"][k], out["s"][k] = q[0], t[0], s[0]
            return out
        self.m.ApplyCorrection(cur, verts, recs(Scw), recs(Siw), Tiw)

    def loop_fusion(self, cur, matched):
        return self.m.LoopFusion(cur, matched)

    def search_and_fuse(self, members, corrected, loop_ids):
        return self.m.SearchAndFuse(members, self.tables[0], loop_ids)

    def essential_graph(self, cur, loop, corrected, noncorrected, members, pairs):
        """the tables are the library's own, from the last Propagate"""
        vs, fixed, Scw, Snc, ed, skipped = self.m.EssentialGraph(cur, loop, self.tables[0],
                                                                 self.tables[1], members, pairs)
        self.graph = (vs, fixed, Scw, Snc, ed)
        return (vs.tolist(), fixed, tuples(Scw), tuples(Snc),
                [(int(e["i"]), int(e["j"]), int(e["kind"])) for e in ed], skipped)


def tuples(S):
    """SIM3D_DTYPE records as ref_essential's one-element tuples"""
    return [(S["q"][k][None].copy(), S["t"][k][None].copy(), S["s"][k:k + 1].copy())
            for k in range(len(S))]


def sim3_close(a, b):
    """ref_sim3opt.distance at ref_essential's tolerance"""
    d = RS.distance({"q": a[0][0], "t": a[1][0], "s": float(a[2][0])},
                    {"q": b[0][0], "t": b[1][0], "s": float(b[2][0])})
    return max(d) <= E.EG_TOL


def assert_float32_close(got, want):
    """stored poses, centres and corrected positions together: within one float spacing of the
    reference's float32 values (the float64 results rounded once), more than 99 % bit-equal"""
    got = np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in got])
    w32 = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in want])
    assert (np.abs(got.astype(np.float64) - w32) <= np.spacing(np.abs(w32))).all()
    assert (got == w32).mean() > 0.99


# ---------------------------------------------------------------------------
# hand cases through the ABI
# ---------------------------------------------------------------------------
def test_hand_points():
    G = GpuLoopMap(16, 8, 8)
    got, nd0 = RL.hand_points_scene(G)
    assert got == RL.HAND_POINTS_SCENE
    want = RL.HAND_POINT0_ND
    assert np.all(np.abs(np.array(nd0[:3]) - want[:3]) <= (3 + 4) * EPS)
    assert abs(nd0[3] - want[3]) <= 8 * EPS * want[3]


@pytest.mark.parametrize("members,expected", [([0, 1], RL.HAND_LC_E_FIRST),
                                              ([1, 0], RL.HAND_LC_T_FIRST)], ids=["e_first", "t_first"])
def test_hand_loop_connections(members, expected):
    assert RL.hand_loop_connections(GpuLoopMap(16, 128, 64), members) == expected


def test_repeated_member():
    """a slot listed twice is processed twice and reported once, from its last entry"""
    want = RL.hand_loop_connections(RL.RefLoopMap(), [1, 0, 1])
    assert RL.hand_loop_connections(GpuLoopMap(16, 128, 64), [1, 0, 1]) == want
    assert want[0] == [(0, 2), (1, 2)]


def test_hand_loop_fusion():
    got = RL.hand_loop_fusion(GpuLoopMap(16, 8, RE.HAND_POINTS))
    got[1] = [list(r) for r in got[1]]
    assert got == RL.HAND_LOOP_FUSION


def test_apply_maps_the_reference_by_mnid():
    assert RL.hand_apply_by_mnid(GpuLoopMap(16, 8, 8)) == RL.HAND_APPLY_BY_MNID


def test_hand_edge_rules():
    assert RL.hand_edge_rules(GpuLoopMap(16, 128, 1024)) == RL.HAND_EDGE_RULES


def test_loop_edges_and_defaults():
    G = GpuLoopMap(16, 8, 8)
    T, has, ids, _ = G.get_poses(16)
    assert not has.any() and ids.tolist() == list(range(16)) and not T.any()
    assert G.corrected(8) == ([0] * 8, [0] * 8)
    G.add_loop_edge(2, 0)
    G.add_loop_edge(0, 2)
    G.add_loop_edge(1, 0)
    assert [G.get_loop_edges(s) for s in range(3)] == [[1, 2], [0], [0]]
    lib, c = L.lib(), TC.ctx().handle
    # capacity: a slot takes MAX_LOOP_EDGES edges; one more is ORBG_ERANGE and changes nothing
    H = GpuLoopMap(32, 8, 8)
    for s in range(1, MAP.MAX_LOOP_EDGES + 1):
        H.add_loop_edge(0, s)
    assert lib.orbg_map_add_loop_edge(c, H.m.handle, 20, 0) == L.ORBG_ERANGE
    assert lib.orbg_map_add_loop_edge(c, H.m.handle, 0, 20) == L.ORBG_ERANGE
    assert H.get_loop_edges(20) == [] and len(H.get_loop_edges(0)) == MAP.MAX_LOOP_EDGES
    assert lib.orbg_map_add_loop_edge(c, H.m.handle, 0, 5) == L.ORBG_OK      # already there
    assert lib.orbg_map_add_loop_edge(c, H.m.handle, 3, 3) == L.ORBG_EINVAL
    assert lib.orbg_map_add_loop_edge(c, H.m.handle, 3, 32) == L.ORBG_EINVAL
    # erase keeps the edges, clear empties them
    H.set_keyframe(5, [1])
    H.erase_keyframe(5)
    assert H.get_loop_edges(5) == [0]
    H.m.clear()
    assert H.get_loop_edges(0) == [] and H.get_loop_edges(5) == []


# ---------------------------------------------------------------------------
# random scenes
# ---------------------------------------------------------------------------
_ref_cache = {}


def ref_scene(oracle, seed, stereo):
    """the Python reference's run of a scene, computed once and left unchanged"""
    if (seed, stereo) not in _ref_cache:
        d = RL.loop_dataset(seed, stereo)
        M = TL.ref_loop_map(oracle)
        st = []

        def check(stage):
            fl = None
            if stage == "propagate":
                fl = (M.get_poses(RL.NKF), M.records(RL.NPTS), dict(M.nd64),
                      {p: len(M.observations(p)) for p in M.nd64})
            st.append((stage, RL.state(M, RL.MAX_KF, RL.NPTS), fl))
        out = RL.run_loop_scene(M, d, check)
        assert TL.scene_is_rich(M, d, out)
        _ref_cache[(seed, stereo)] = (d, out, st, M)
    return _ref_cache[(seed, stereo)][:3]


def check_propagate_floats(tables, poses_g, rec_g, out_r, out_g, fl):
    (T_r, _, _, c_r), rec_r, nd64, nobs = fl
    for s in out_r["set"]:
        assert sim3_close(out_g["corrected"][s], out_r["corrected"][s])
        assert sim3_close(out_g["noncorrected"][s], out_r["noncorrected"][s])
    # slots outside the set are not written
    co, nc = tables
    outside = [s for s in range(RL.MAX_KF) if s not in out_r["set"]]
    assert not co["q"][outside].any() and not nc["s"][outside].any()
    T_g, _, _, c_g = poses_g
    members = out_r["set"]
    rest = [s for s in range(RL.NKF) if s not in members]
    assert T_g[rest].tobytes() == T_r[rest].tobytes() and c_g[rest].tobytes() == c_r[rest].tobytes()
    moved = sorted(nd64)
    pos_g = np.stack([rec_g[k] for k in "xyz"], 1)
    pos_r = np.stack([rec_r[k] for k in "xyz"], 1)
    assert_float32_close([T_g[members], c_g[members], pos_g[moved]],
                         [T_r[members], c_r[members], pos_r[moved]])
    still = [p for p in range(RL.NPTS) if p not in nd64]
    assert rec_g[still].tobytes() == rec_r[still].tobytes() and len(moved) > 200
    # normals and distances at check_normal_depth_bounds' bounds, for the points whose inputs
    # (position, member centres) the two runs hold bit for bit
    same_c = (c_g == c_r).all()
    n_checked = 0
    for p in moved:
        if nd64[p] is None or not same_c or not (pos_g[p] == pos_r[p]).all():
            continue
        nrm, mind, maxd = nd64[p]
        g = rec_g[p]
        assert np.all(np.abs(np.array([g["nx"], g["ny"], g["nz"]], np.float64) - nrm)
                      <= (nobs[p] + 4) * EPS), p
        assert abs(float(g["min_dist"]) - mind) <= 8 * EPS * mind, p
        assert abs(float(g["max_dist"]) - maxd) <= 8 * EPS * maxd, p
        n_checked += 1
    assert n_checked > 0.9 * len(moved) or not same_c
    return n_checked


@pytest.mark.parametrize("seed,stereo", TL.RL_SCENES)
def test_random_scene(oracle, seed, stereo):
    d, out_r, st_r = ref_scene(oracle, seed, stereo)
    G = GpuLoopMap(RL.MAX_KF, RL.KF_CAP, RL.NPTS)
    st_g, fl_g = [], []

    def check(stage):
        st_g.append((stage, RL.state(G, RL.MAX_KF, RL.NPTS)))
        if stage == "propagate":
            fl_g.extend([G.tables, G.get_poses(RL.NKF), G.records(RL.NPTS)])
    out_g = RL.run_loop_scene(G, d, check)
    assert out_g["set"] == out_r["set"] and 5 <= len(out_r["set"])
    assert out_g["fusion"] == out_r["fusion"] and min(out_r["fusion"]) >= 1
    assert out_g["saf"] == out_r["saf"] and out_r["saf"][1] >= 1      # replacements in SearchAndFuse
    assert out_g["pairs"] == out_r["pairs"] and len(out_r["pairs"]) > 1
    TE.assert_states([(s, a) for s, a, _ in st_r], st_g)
    fl = [f for s, _, f in st_r if s == "propagate"][0]
    assert check_propagate_floats(fl_g[0], fl_g[1], fl_g[2], out_r, out_g, fl) > 100
    # the essential graph: vertices, the fixed one and the edge list exactly, Scw / Snc close
    assert out_g["verts"] == out_r["verts"] == list(range(RL.NKF))
    assert out_g["fixed"] == out_r["fixed"] and out_g["skipped"] == out_r["skipped"] == 0
    assert out_g["edges"] == out_r["edges"]
    assert sum(e[2] == 0 for e in out_r["edges"]) >= 2 and len(out_r["edges"]) > RL.NKF
    for v in range(RL.NKF):
        assert sim3_close(out_g["Scw"][v], out_r["Scw"][v])
        assert sim3_close(out_g["Snc"][v], out_r["Snc"][v])
    # the library's own optimiser on the library's arrays, then Apply on both maps
    import copy
    from orb_slam2_test_amd import OptimizeEssentialGraph
    vs, fixed, Scw, Snc, ed = G.graph
    Siw, Tiw, rep = OptimizeEssentialGraph(Scw, Snc, ed, fixed, stereo)
    assert rep["iterations"] > 0 and rep["final_chi2"] < rep["initial_chi2"]
    M = copy.deepcopy(_ref_cache[(seed, stereo)][3])
    M.apply_correction(RL.CUR, out_r["verts"], out_r["Scw"], tuples(Siw), Tiw)
    G.m.ApplyCorrection(RL.CUR, vs, Scw, Siw, Tiw)
    assert RL.state(G, RL.MAX_KF, RL.NPTS) == RL.state(M, RL.MAX_KF, RL.NPTS)
    T_g, has_g, _, c_g = G.get_poses(RL.NKF)
    T_r, _, _, c_r = M.get_poses(RL.NKF)
    assert T_g.tobytes() == Tiw.tobytes() == T_r.tobytes() and c_g.tobytes() == c_r.tobytes()
    rec_g, rec_r = G.records(RL.NPTS), M.records(RL.NPTS)
    good = np.flatnonzero(rec_r["flags"] & L.MP_VALID)
    pos_g = np.stack([rec_g[k] for k in "xyz"], 1)
    pos_r = np.stack([rec_r[k] for k in "xyz"], 1)
    assert_float32_close([pos_g[good]], [pos_r[good]])
    before = np.stack([fl[1][k] for k in "xyz"], 1)
    assert np.abs(pos_r[good] - before[good]).max() > 1e-3
    bad = np.flatnonzero(~(rec_r["flags"] & L.MP_VALID).astype(bool))
    assert rec_g[bad].tobytes() == rec_r[bad].tobytes()
    n_checked = 0
    for p in good.tolist():
        nd = M.normal_and_depth64(p)
        if nd is None or not (pos_g[p] == pos_r[p]).all():
            continue
        g = rec_g[p]
        assert np.all(np.abs(np.array([g["nx"], g["ny"], g["nz"]], np.float64) - nd[0])
                      <= (len(M.observations(p)) + 4) * EPS), p
        assert abs(float(g["min_dist"]) - nd[1]) <= 8 * EPS * nd[1], p
        assert abs(float(g["max_dist"]) - nd[2]) <= 8 * EPS * nd[2], p
        n_checked += 1
    assert n_checked > 0.9 * len(good) > 400
    # CorrectLoop in one call on a fresh map: the same state, the floats bit for bit
    G2 = GpuLoopMap(RL.MAX_KF, RL.KF_CAP, RL.NPTS)
    RL.build_loop_map(G2, d)
    rep2, cnt = G2.m.CorrectLoop(RL.CUR, RL.LOOP, d["Scw"], d["matched"], d["loop_ids"], stereo)
    assert rep2 == rep
    assert cnt == dict(members=len(out_r["set"]), fusion_replaced=out_r["fusion"][0],
                       fusion_added=out_r["fusion"][1], fused=out_r["saf"][0], replaced=out_r["saf"][1],
                       pairs=len(out_r["pairs"]), vertices=RL.NKF, edges=len(out_r["edges"]))
    assert RL.state(G2, RL.MAX_KF, RL.NPTS) == RL.state(M, RL.MAX_KF, RL.NPTS)
    assert G2.records(RL.NPTS).tobytes() == rec_g.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(G2.get_poses(RL.NKF), G.get_poses(RL.NKF)))


def test_device_forms(oracle):
    """propagate_device and loop_connections_device back to back, no synchronisation between
    them, lengths on the device; a short pair buffer gets the first pair_cap pairs"""
    import torch
    d, out_r, st_r = ref_scene(oracle, 0, False)
    G = GpuLoopMap(RL.MAX_KF, RL.KF_CAP, RL.NPTS)
    RL.build_loop_map(G, d)
    cap, K = 16, RL.MAX_KF
    S = np.zeros(1, L.SIM3D_DTYPE)
    S["q"][0], S["t"][0], S["s"][0] = d["Scw"]
    t_S = TC.dev(S.view(np.uint8))
    t_set = torch.full((cap + 4,), -7, dtype=torch.int32, device="cuda")
    t_n = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    t_co = torch.zeros(K * 64, dtype=torch.uint8, device="cuda")
    t_nc = torch.zeros(K * 64, dtype=torch.uint8, device="cuda")
    t_st = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    G.m.propagate_device(RL.CUR, t_S.data_ptr(), t_set.data_ptr(), cap, t_n.data_ptr(),
                         t_co.data_ptr(), t_nc.data_ptr(), t_st.data_ptr())
    TC.ctx().sync()
    n = len(out_r["set"])
    assert t_n.tolist() == [n, -7] and t_st.tolist()[:2] == [0, n]
    assert t_set.tolist() == out_r["set"] + [-1] * (cap - n) + [-7] * 4
    assert RL.state(G, K, RL.NPTS) == st_r[1][1]
    t_m, t_l = TC.dev(np.array(d["matched"], np.int32)), TC.dev(np.array(d["loop_ids"], np.int32))
    t_c = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    G.m.loop_fusion_device(RL.CUR, t_m.data_ptr(), len(d["matched"]), t_c.data_ptr())
    G.m.search_and_fuse_device(t_set.data_ptr(), cap, t_n.data_ptr(), t_co.data_ptr(), t_l.data_ptr(),
                               len(d["loop_ids"]), 4.0, t_c[2:].data_ptr())
    TC.ctx().sync()
    assert t_c.tolist() == list(out_r["fusion"]) + list(out_r["saf"]) + [-7]
    assert RL.state(G, K, RL.NPTS) == st_r[3][1]
    pcap = len(out_r["pairs"]) - 1
    t_p = torch.full((2 * pcap + 2,), -7, dtype=torch.int32, device="cuda")
    t_np = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    G.m.loop_connections_device(t_set.data_ptr(), cap, t_n.data_ptr(), t_p.data_ptr(), pcap,
                                t_np.data_ptr())
    TC.ctx().sync()
    assert t_np.item() == len(out_r["pairs"])
    assert t_p.tolist() == [v for p in out_r["pairs"][:pcap] for v in p] + [-7, -7]
    assert RL.state(G, K, RL.NPTS) == st_r[4][1]
    # the essential graph from device arrays: the pairs uploaded in full, the counts on the device
    pr = np.array(out_r["pairs"], np.int32)
    t_pr = TC.dev(pr.reshape(-1))
    t_cnt = TC.dev(np.array([len(pr)], np.int32))
    ecap = len(out_r["edges"]) - 3
    t_vs = torch.full((K + 1,), -7, dtype=torch.int32, device="cuda")
    t_h = torch.full((8,), -7, dtype=torch.int32, device="cuda")      # nvert, fixed, nedge, -, status
    t_sc = torch.zeros(2 * K * 64, dtype=torch.uint8, device="cuda")
    t_ed = torch.full((3 * ecap + 3,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    G.m.essential_graph_device(RL.CUR, RL.LOOP, t_co.data_ptr(), t_nc.data_ptr(), t_set.data_ptr(),
                               cap, t_n.data_ptr(), t_pr.data_ptr(), len(pr), t_cnt.data_ptr(),
                               t_vs.data_ptr(), t_h.data_ptr(), t_h[1:].data_ptr(), t_sc.data_ptr(),
                               t_sc[K * 64:].data_ptr(), t_ed.data_ptr(), ecap, t_h[2:].data_ptr(),
                               t_h[4:].data_ptr())
    TC.ctx().sync()
    assert t_h.tolist()[:3] == [RL.NKF, out_r["fixed"], len(out_r["edges"])]
    assert t_h.tolist()[4:6] == [0, 0] and t_h[3].item() == -7
    assert t_vs.tolist() == out_r["verts"] + [-7] * (K + 1 - RL.NKF)
    assert t_ed.tolist() == [v for e in out_r["edges"][:ecap] for v in e] + [-7] * 3


# ---------------------------------------------------------------------------
# errors and limits
# ---------------------------------------------------------------------------
def test_error_paths():
    lib, c = L.lib(), TC.ctx().handle
    G = GpuLoopMap(16, 8, 8)
    RL.hand_points_scene(G)
    m = G.m.handle
    K = 16
    S = np.zeros(1, L.SIM3D_DTYPE)
    S["q"][0], S["s"][0] = (0, 0, 0, 1), 1.0
    st = np.full(8, -7, np.int32)
    n = C.c_int32(-7)
    co = np.full(K * 8, 7.5)
    nc = np.full(K * 8, 7.5)
    pairs = np.full(64, -7, np.int32)

    def prop(cur, s=S, set_=st, cap=8, nn=n, a=co, b=nc):
        return lib.orbg_map_propagate(c, m, cur, L.ptr(s), L.ptr(set_), cap,
                                      C.byref(nn) if nn is not None else None, L.ptr(a), L.ptr(b))
    before = RL.state(G, K, 8)
    for cur in (-1, 16):
        assert prop(cur) == L.ORBG_EINVAL
    assert "outside" in L.last_error()
    assert prop(2, s=None) == L.ORBG_EINVAL
    assert prop(2, set_=None) == L.ORBG_EINVAL
    assert prop(2, nn=None) == L.ORBG_EINVAL
    assert prop(2, a=None) == L.ORBG_EINVAL
    assert prop(2, cap=0) == L.ORBG_EINVAL
    assert prop(2, cap=MAP.MAX_LOOP_SET + 1) == L.ORBG_ENOTSUP
    assert lib.orbg_map_loop_connections(c, m, None, 2, L.ptr(pairs), 32, C.byref(n)) == L.ORBG_EINVAL
    bad_set = np.array([1, 16], np.int32)
    assert lib.orbg_map_loop_connections(c, m, L.ptr(bad_set), 2, L.ptr(pairs), 32,
                                         C.byref(n)) == L.ORBG_EINVAL
    assert lib.orbg_map_loop_connections(c, m, L.ptr(bad_set), 2, L.ptr(pairs), 32, None) == L.ORBG_EINVAL
    sl = np.array([0], np.int32)
    assert lib.orbg_map_set_keyframe_poses(c, m, L.ptr(sl), 1, None, None) == L.ORBG_EINVAL
    assert lib.orbg_map_set_keyframe_poses(c, m, None, 1, L.ptr(co), None) == L.ORBG_EINVAL
    assert lib.orbg_map_get_keyframe_poses(c, m, 10, 7, None, None, None, None) == L.ORBG_EINVAL
    assert lib.orbg_map_get_point_corrected(c, m, 6, 3, L.ptr(st), L.ptr(st)) == L.ORBG_EINVAL
    assert lib.orbg_map_get_loop_edges(c, m, 16, L.ptr(st), 8, C.byref(n)) == L.ORBG_EINVAL
    # the essential graph and Apply: cur == loop, slots out of range, NULL pointers
    vs, ne = np.full(K, -7, np.int32), C.c_int32(-7)
    tab = np.zeros(K, L.SIM3D_DTYPE)
    out_s = np.full(K * 8, 7.5)
    ed = np.full(96, -7, np.int32)
    members = np.array([1, 2], np.int32)

    def graph(cur, loop, t=tab, mem=members, v=vs, e=ed):
        return lib.orbg_map_essential_graph(c, m, cur, loop, L.ptr(t), L.ptr(t), L.ptr(mem), 2,
                                            None, 0, L.ptr(v), C.byref(n), C.byref(n), L.ptr(out_s),
                                            L.ptr(out_s), L.ptr(e), 32, C.byref(ne), None)
    assert graph(2, 2) == L.ORBG_EINVAL and "both" in L.last_error()
    assert graph(2, 16) == L.ORBG_EINVAL and graph(-1, 0) == L.ORBG_EINVAL
    assert graph(2, 0, t=None) == L.ORBG_EINVAL and graph(2, 0, v=None) == L.ORBG_EINVAL
    assert graph(2, 0, mem=bad_set) == L.ORBG_EINVAL
    assert graph(2, 9) == L.ORBG_EINVAL and "vertex" in L.last_error()     # loop is no keyframe
    assert lib.orbg_map_apply_correction(c, m, 16, L.ptr(vs), 1, L.ptr(tab), L.ptr(tab),
                                         L.ptr(out_s)) == L.ORBG_EINVAL
    assert lib.orbg_map_apply_correction(c, m, 2, L.ptr(vs), 1, L.ptr(tab), L.ptr(tab),
                                         L.ptr(out_s)) == L.ORBG_EINVAL      # vert_slot -7
    assert lib.orbg_map_apply_correction(c, m, 2, None, 1, L.ptr(tab), L.ptr(tab),
                                         L.ptr(out_s)) == L.ORBG_EINVAL
    assert n.value == -7 and ne.value == -7 and (vs == -7).all() and (ed == -7).all()
    assert (out_s == 7.5).all()
    assert RL.state(G, K, 8) == before
    # nothing attached: the fusion stages and CorrectLoop are ORBG_EINVAL
    cnt8, rep = np.full(8, -7, np.int32), L.LmReport()
    one = np.array([1], np.int32)
    assert lib.orbg_map_search_and_fuse(c, m, L.ptr(members), 2, L.ptr(tab), L.ptr(one), 1, 4.0,
                                        L.ptr(cnt8)) == L.ORBG_EINVAL and "attached" in L.last_error()
    assert lib.orbg_map_loop_fusion(c, m, 2, L.ptr(one), 1, L.ptr(cnt8)) == L.ORBG_EINVAL
    assert lib.orbg_map_correct_loop(c, m, 2, 0, L.ptr(S), L.ptr(one), 1, L.ptr(one), 1, 0,
                                     C.byref(rep), L.ptr(cnt8)) == L.ORBG_EINVAL
    assert "attached" in L.last_error()
    assert lib.orbg_map_correct_loop(c, m, 2, 2, L.ptr(S), L.ptr(one), 1, L.ptr(one), 1, 0,
                                     C.byref(rep), L.ptr(cnt8)) == L.ORBG_EINVAL
    assert lib.orbg_map_correct_loop(c, m, 2, 16, L.ptr(S), L.ptr(one), 1, L.ptr(one), 1, 0,
                                     C.byref(rep), L.ptr(cnt8)) == L.ORBG_EINVAL
    assert lib.orbg_map_correct_loop(c, m, 2, 0, None, L.ptr(one), 1, L.ptr(one), 1, 0,
                                     C.byref(rep), L.ptr(cnt8)) == L.ORBG_EINVAL
    assert (cnt8 == -7).all() and RL.state(G, K, 8) == before
    # a dead cur; a set longer than set_cap; a member without a pose: reported, outputs untouched
    assert prop(9) == L.ORBG_EINVAL and "live" in L.last_error()
    assert prop(2, cap=1) == L.ORBG_ERANGE
    G.set_keyframe(4, [0, 1, 2, 4, 5])      # shares three points with cur: its new best neighbour
    assert prop(2) == L.ORBG_EINVAL and "pose" in L.last_error()
    assert n.value == -7 and (st == -7).all() and (co == 7.5).all() and (nc == 7.5).all()
    after = RL.state(G, K, 8)
    assert after["corr"] == before["corr"] and after["bad"] == before["bad"]
    # the device form reports the same in its status word
    import torch
    t = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    t_S = TC.dev(S.view(np.uint8))
    t_tab = torch.zeros(2 * K * 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    G.m.propagate_device(2, t_S.data_ptr(), t.data_ptr(), 8, t[8:].data_ptr(), t_tab.data_ptr(),
                         t_tab[K * 64:].data_ptr(), t[12:].data_ptr())
    TC.ctx().sync()
    assert t.tolist()[:9] == [-1] * 8 + [0] and t.tolist()[12:14] == [MAP.LOOP_NO_POSE, 2]
    assert not t_tab.any()
    # a vertex outside the set without a pose (slot 4): ORBG_EINVAL, outputs untouched
    assert graph(2, 0) == L.ORBG_EINVAL and "pose" in L.last_error()
    assert n.value == -7 and ne.value == -7 and (vs == -7).all() and (out_s == 7.5).all()


# ---------------------------------------------------------------------------
# defaults: a map that never receives a pose, an mnId or a loop edge
# ---------------------------------------------------------------------------
def test_defaults_leave_the_edit_scene_alone(oracle):
    d = RE.edit_dataset(0, False)
    M, G = TE.ref_map(oracle), TE.GpuEditMap()
    out_r = RE.run_edit_scene(M, d)
    assert RE.run_edit_scene(G, d) == out_r
    assert RE.state(G, RE.MAX_KF, RE.NPTS) == RE.state(M, RE.MAX_KF, RE.NPTS)
    assert G.m.points().tobytes() == TE.records_of(M, RE.NPTS).tobytes()
    _, has, ids, _ = G.m.poses()
    assert not has.any() and ids.tolist() == list(range(RE.MAX_KF))
    by, ref = G.m.corrected()
    assert not by.any() and not ref.any()
