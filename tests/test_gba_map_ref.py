"""CPU: tests/ref_gba_map.py, the pure-Python statement of global bundle adjustment's window, store
and map update over the map, against expectations written out by hand; the scenes of
tests/test_gpu_gba_map.py really contain the cases that file claims to cover; and the interface
the library declares."""
import copy
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_gba_map as RG  # noqa: E402
import ref_lba_map as RB  # noqa: E402
import ref_map as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------
def test_hand_window():
    w = RG.hand_window(RG.RefGbaMap())
    assert RG.window_lists(w) == RG.HAND_WINDOW
    e = w["edges"]
    assert (e["robust"] == 1).all() and (e["active"] == 1).all() and (e["pad"] == 0).all()
    assert e["point"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4] and e["pose"].tolist() == [0, 2, 0, 1, 0, 1, 1, 2, 1]
    # 5.99, not LocalBundleAdjustment's 5.991
    assert e["huber_delta"][0] == float(F(np.sqrt(5.99))) != float(F(np.sqrt(5.991)))
    assert e["huber_delta"][5] == float(F(np.sqrt(7.815)))
    # edge 5: point 2 at slot 1's stereo feature 0: (10, 100), mvuRight 8, camera 1
    assert e["obs"][5].tolist() == [10.0, 100.0, 8.0] and (e["fx"][5], e["fy"][5]) == (501.0, 511.0)
    # edge 3: slot 1's mono feature 1, octave 1
    assert e["obs"][3].tolist() == [11.0, 101.0, 0.0]
    assert e["inv_sigma2"][3] == float(F(1.0) / F(F(1.2) * F(1.2)))
    assert w["poses"]["q"].tolist() == [[0.0, 0.0, 0.0, 1.0]] * 4
    assert w["poses"]["t"][:, 0].tolist() == [0.0, -0.5, -1.0, -2.5]
    assert w["points"][4].tolist() == [float(F(0.09)), 0.0, 5.0]


def test_hand_window_not_robust_and_mono():
    w = RG.hand_window(RG.RefGbaMap(), stereo_slots=())
    assert (w["edges"]["robust"] == 1).all() and (w["edges"]["stereo"] == 0).all()
    M = RG.RefGbaMap()
    RG.hand_window(M)
    w0 = M.gba_window(False)
    assert (w0["edges"]["robust"] == 0).all() and int(w0["edges"]["stereo"].sum()) == 2


def test_window_errors():
    M = RG.RefGbaMap()
    RG.hand_window(M)
    M.set_keyframe(6, [1])                                  # live, not bad, no pose
    with pytest.raises(RB.WindowError):
        M.gba_window(True)
    M = RG.RefGbaMap()
    RG.hand_window(M)
    M.d = dict(M.d, kps=[k[:2] for k in M.d["kps"]])        # two keypoints attached per slot
    with pytest.raises(RB.WindowError):
        M.gba_window(True)
    M = RG.RefGbaMap()
    R._plain_points(M, 4)
    M.set_keyframe(0, [0])
    with pytest.raises(RB.WindowError):
        M.gba_window(True)                                  # nothing attached


def test_win_scene_holds_its_cases():
    M = RG.RefGbaMap()
    RG.win_scene(M)
    w = M.gba_window(True)
    assert [len(w["kf_slots"]), len(w["point_ids"]), len(w["edges"]), w["left_out"]] == RG.WIN_COUNTS
    assert w["kf_slots"].tolist() == [3, 5, 11, 254, 255, 256, 257, 258]
    assert w["poses"]["fixed"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert w["point_ids"].tolist() == [0, 1, 2, 3, 4, 5, 103, 2046, 2047, 2048, 2049, 2050, 4095,
                                       4096, 4097]
    e = w["edges"]
    assert set(e["stereo"].tolist()) == {0, 1}
    octs = {float(v) for v in e["inv_sigma2"]}
    assert octs == {float(RB.inv_level_sigma2()[0]), float(RB.inv_level_sigma2()[7])}
    by_point = {int(p): [] for p in w["point_ids"]}
    for k in range(len(e)):
        by_point[int(w["point_ids"][e["point"][k]])].append(int(w["kf_slots"][e["pose"][k]]))
    assert by_point[103] == [5] and by_point[2] == [3] and by_point[2050] == [254]
    assert by_point[0] == [3, 5, 257]
    # Eigen's three diagonal branches and the trace branch are all taken
    traces = [float(np.trace(M.pose[int(s)][:, :3].astype(np.float64))) for s in w["kf_slots"]]
    assert sum(t <= 0 for t in traces) >= 3 and sum(t > 0 for t in traces) >= 1
    diag = {int(np.argmax(np.diag(M.pose[s][:, :3]))) for s in (254, 255, 256)}
    assert diag == {0, 1, 2}
    w2 = RG.RefGbaMap()
    RG.win_scene(w2, stereo=False)
    assert (w2.gba_window(False)["edges"]["stereo"] == 0).all()


# ---------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------
def test_store_modes():
    M = RG.RefGbaMap()
    w = RG.hand_window(M)
    poses, points = RG.store_estimates(w)
    M.set_keyframe(1, [2, 1, 9, 3], bad=True)               # gone bad since the window
    M.set_point_bad(3)
    before = copy.deepcopy((M.pose, {p: m["pos"].copy() for p, m in M.mp.items()}))
    assert M.gba_store(w, poses, points, 7) == (3, 4)
    assert {s: v for s, v in M.kf_gba.items() if v} == {0: 7, 2: 7, 5: 7}
    assert {p: v for p, v in M.mp_gba.items() if v} == {0: 7, 1: 7, 2: 7, 9: 7}
    assert all(np.array_equal(M.pose[s], before[0][s]) for s in M.pose)
    assert all(np.array_equal(M.mp[p]["pos"], before[1][p]) for p in M.mp)
    assert np.array_equal(M.TcwGBA[2], RB.tcw_of(poses["q"][2], poses["t"][2]))
    assert np.array_equal(M.PosGBA[9], points[4].astype(F))
    assert M.gba_store(w, poses, points, 0) == (3, 4)
    assert np.array_equal(M.pose[2], M.TcwGBA[2]) and np.array_equal(M.pose[1], before[0][1])
    assert np.array_equal(M.mp[9]["pos"], M.PosGBA[9]) and np.array_equal(M.mp[3]["pos"], before[1][3])
    assert np.array_equal(M.kf[2]["centre"], RG.RL.cv_centre(M.pose[2]))


# ---------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------
def test_hand_tree():
    M, M0 = RG.RefGbaMap(), RG.RefGbaMap()
    RG.hand_tree_build(M0)                                  # the state before, for the formulas below
    assert RG.hand_tree(M) == RG.HAND_TREE
    A = lambda T: np.concatenate([np.asarray(T, np.float64), [[0, 0, 0, 1]]], 0)   # noqa: E731
    # slot 2: (Tcw_2 * Twc_0) * mTcwGBA_0 with the poses from before the call
    want2 = A(M0.pose[2]) @ np.linalg.inv(A(M0.pose[0])) @ A(M0.TcwGBA[0])
    assert np.abs(A(M.TcwGBA[2]) - want2).max() < 1e-5
    want3 = A(M0.pose[3]) @ np.linalg.inv(A(M0.pose[2])) @ want2
    assert np.abs(A(M.TcwGBA[3]) - want3).max() < 1e-5
    # slot 4 is in the BA: its own mTcwGBA; every visited slot: mTcwBefGBA = the old pose, pose = mTcwGBA
    assert np.array_equal(M.TcwGBA[4], M0.TcwGBA[4])
    for s in (0, 1, 2, 3, 4):
        assert np.array_equal(M.TcwBef[s], M0.pose[s]) and np.array_equal(M.pose[s], M.TcwGBA[s])
        assert M.kf_gba[s] == 7
    assert np.array_equal(M.pose[6], M0.pose[6]) and 6 not in M.TcwBef and M.kf_gba[5] == 0
    # the points
    assert M.mp[0]["pos"].tolist() == [9.0, 8.0, 7.0]
    for p, r in ((1, 1), (2, 3)):
        X = np.append(M0.mp[p]["pos"].astype(np.float64), 1.0)
        want = np.linalg.inv(A(M.pose[r])) @ A(M0.pose[r]) @ X
        assert np.abs(M.mp[p]["pos"] - want[:3]).max() < 1e-4
    for p in (3, 4, 5, 6, 7):
        assert np.array_equal(M.mp[p]["pos"], M0.mp[p]["pos"])


def test_update_errors_change_nothing():
    def fresh():
        M = RG.RefGbaMap()
        RG.hand_tree_build(M)
        return M
    for origins, loop_kf, prep in (([5], 7, None), ([2], 7, None), ([0], 0, None), ([0], 8, None),
                                   ([0], 7, lambda M: M.set_parent(2, 3)),
                                   ([0], 7, lambda M: M.pose.pop(0))):
        M = fresh()
        if prep:
            prep(M)
        before = RG.state_bytes(M, 7, 8) if 0 in M.pose else None
        with pytest.raises(RG.UpdateError):
            M.gba_update(loop_kf, origins)
        if before is not None:
            assert RG.state_bytes(M, 7, 8) == before


def test_tree_scene_holds_its_cases():
    M = RG.RefGbaMap()
    RG.tree_scene(M, 7)
    M0 = copy.deepcopy(M)
    assert M.gba_update(7, RG.TREE_ORIGINS) == RG.TREE_COUNTS
    par = RG.tree_parents()

    def run_length(s):
        n = 0
        while M0.kf_gba.get(s, 0) != 7:
            s, n = par[s], n + 1
        return n
    assert {run_length(s) for s in (8, 11, 12, 22, 329, 14)} == {1, 3, 70, 260}
    assert run_length(22) == 70 and run_length(329) == 260 and run_length(12) == 3
    assert M0.kf[RG.TREE_BAD]["bad"] and M.kf_gba[RG.TREE_BAD] == 7
    assert np.array_equal(M.TcwGBA[13], M0.TcwGBA[13])
    for s in (16, 17):
        assert np.array_equal(M.pose[s], M0.pose[s]) and s not in M.TcwBef
    moved = [p for p in range(RG.TREE_POINTS) if not np.array_equal(M.mp[p]["pos"], M0.mp[p]["pos"])]
    assert moved == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14] + list(range(16, RG.TREE_POINTS))
    # a second loop on the same map: the marks of the first are stale
    RG.tree_ba_state(M, 9, np.random.default_rng(5))
    assert M.gba_update(9, RG.TREE_ORIGINS) == [277, 269, 2, 17, 2, 0]


def test_a_slot_that_becomes_live_starts_unmarked():
    M = RG.RefGbaMap()
    M.set_keyframe(3, [])
    M.set_gba_state(3, kf_gba=[5])
    M.set_keyframe(3, [])                                   # still live: kept
    assert M.kf_gba[3] == 5
    M.erase_keyframe(3)
    M.set_keyframe(3, [])
    assert M.kf_gba[3] == 0


# ---------------------------------------------------------------------------
# the declared interface
# ---------------------------------------------------------------------------
def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "orbg.h")).read()
    for name in ("orbg_map_set_gba_state", "orbg_map_get_gba_state", "orbg_map_gba_window_device",
                 "orbg_map_gba_window", "orbg_map_gba_store_device", "orbg_map_gba_store",
                 "orbg_map_gba_update_device", "orbg_map_gba_update", "orbg_map_global_ba",
                 "orbg_map_run_global_ba"):
        assert re.search(r"\bint %s\(" % name, text), name
    assert "} orbg_map_gba_report;" in text
    for bit, value in (("ORIGIN", 1), ("CYCLE", 2)):
        assert re.search(r"#define ORBG_GBA_%s %d\b" % (bit, value), text)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "GlobalBundleAdjustment on the Map" in design
