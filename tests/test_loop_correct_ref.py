"""CPU: hand cases with answers written out by hand pin tests/ref_loop_correct.py, the Python
statement the GPU test (tests/test_gpu_loop_correct.py) compares the library with; and the random
scenes are checked to contain what that test needs, so an empty scene cannot pass there."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402
import ref_loop_correct as RL  # noqa: E402


def test_point_owner_and_already_corrected():
    """a point in the rows of two members and an outsider is corrected once, by the lower member,
    with the centres as they stand at that moment; a second Propagate leaves the points alone"""
    M = RL.RefLoopMap()
    got, nd0 = RL.hand_points_scene(M)
    assert got == RL.HAND_POINTS_SCENE
    assert np.allclose(nd0, RL.HAND_POINT0_ND, rtol=0, atol=2e-7)
    # min distance: max / 1.2^7
    assert abs(float(M.mp[0]["min"]) - RL.S17 / 1.2 ** 7) < 1e-6


def test_loop_connections_depend_on_the_order():
    assert RL.hand_loop_connections(RL.RefLoopMap(), [0, 1]) == RL.HAND_LC_E_FIRST
    assert RL.hand_loop_connections(RL.RefLoopMap(), [1, 0]) == RL.HAND_LC_T_FIRST


def test_apply_maps_the_reference_by_mnid():
    assert RL.hand_apply_by_mnid(RL.RefLoopMap()) == RL.HAND_APPLY_BY_MNID


def test_edge_rules():
    assert RL.hand_edge_rules(RL.RefLoopMap()) == RL.HAND_EDGE_RULES


def test_exports():
    import orb_slam2_test_amd as P
    assert {"Map", "MAX_LOOP_EDGES", "MAX_LOOP_SET"} <= set(P.__all__)
    for name in ("SetPoses", "poses", "AddLoopEdge", "GetLoopEdges", "corrected", "Propagate",
                 "LoopConnections", "EssentialGraph", "ApplyCorrection", "propagate_device",
                 "LoopFusion", "SearchAndFuse", "CorrectLoop", "SetCorrected", "loop_fusion_device",
                 "search_and_fuse_device",
                 "loop_connections_device", "essential_graph_device", "apply_correction_device"):
        assert callable(getattr(P.Map, name)), name


def test_loop_edges_and_defaults():
    M = RL.RefLoopMap()
    R._plain_points(M, 4)
    for s in range(3):
        M.set_keyframe(s, [s])
    assert M.get_poses(3)[1].tolist() == [False] * 3 and M.get_poses(3)[2].tolist() == [0, 1, 2]
    assert M.corrected(4) == ([0] * 4, [0] * 4)
    M.add_loop_edge(2, 0)
    M.add_loop_edge(0, 2)
    M.add_loop_edge(1, 0)
    assert [M.get_loop_edges(s) for s in range(3)] == [[1, 2], [0], [0]]


def test_cv_products():
    """SetPose's centre and Tiw * Twc against float64 NumPy: one float rounding each"""
    rng = np.random.default_rng(5)
    Rm = RL._rot(rng.normal(size=3))
    T = np.concatenate([Rm, rng.normal(size=(3, 1)) * 4], 1).astype(RL.F)
    O = RL.cv_centre(T)
    want = -(T[:, :3].astype(np.float64).T @ T[:, 3].astype(np.float64))
    assert np.all(np.abs(O - want) <= np.spacing(np.abs(want).astype(RL.F)))
    A = np.concatenate([T, [[0, 0, 0, 1]]]).astype(RL.F)
    P = RL.cv_mul44(A, A)
    want = A.astype(np.float64) @ A.astype(np.float64)
    assert np.all(np.abs(P - want) <= np.spacing(np.abs(want).astype(RL.F)))


def ref_loop_map(oracle):
    import test_oracle_mapping as T
    M = RL.RefLoopMap()
    M.search_sim3 = RL.make_search_sim3(oracle.fuse_sim3_search, T._fuse_tables(oracle)[0])
    return M


def test_loop_fusion_rules():
    got = RL.hand_loop_fusion(RL.RefLoopMap())
    got[1] = [list(r) for r in got[1]]
    assert got == RL.HAND_LOOP_FUSION


def test_scenes_are_not_empty(oracle):
    """chosen here, on the CPU: each scene has a set of several members, points shared by two
    members, replacements in the stand-in fusion and LoopConnections pairs on more than one
    member; the reference alone decides"""
    for seed, stereo in RL_SCENES:
        d = RL.loop_dataset(seed, stereo)
        M = ref_loop_map(oracle)
        out = RL.run_loop_scene(M, d)
        assert scene_is_rich(M, d, out), (seed, stereo)


RL_SCENES = ((0, False), (1, True))


def scene_is_rich(M, d, out):
    members = out["set"]
    if not (5 <= len(members) <= 12 and members[-1] == RL.CUR):
        return False
    by, ref = M.corrected(d["npts"])
    curid = d["mnid"][RL.CUR]
    owners = {r for b, r in zip(by, ref) if b == curid}
    shared = sum(1 for p in range(d["npts"])
                 if len([s for s, _ in M.observations(p) if s in members]) >= 2)
    groups = {i for i, _ in out["pairs"]}
    kind0 = [e for e in out["edges"] if e[2] == 0]
    covis = connected(len(out["verts"]), out["edges"])
    return (len(owners) >= 3 and shared >= 20 and out["saf"][1] >= 1 and out["saf"][0] > out["saf"][1]
            and out["fusion"][0] >= 1 and out["fusion"][1] >= 1
            and len(groups) >= 2 and (RL.CUR, RL.LOOP) in out["pairs"]
            and len(kind0) >= 2 and len(kind0) < len(out["pairs"]) and covis
            and out["fixed"] == out["verts"].index(RL.LOOP))


def connected(n, edges):
    """every vertex reaches vertex 0 (the optimiser's precondition)"""
    adj = {v: set() for v in range(n)}
    for i, j, _ in edges:
        adj[i].add(j)
        adj[j].add(i)
    seen, todo = {0}, [0]
    while todo:
        for w in adj[todo.pop()]:
            if w not in seen:
                seen.add(w)
                todo.append(w)
    return len(seen) == n
