"""CPU: tests/ref_map.py, the pure-Python statement of KeyFrame::UpdateConnections,
Tracking::UpdateLocalKeyFrames / UpdateLocalPoints and MapPoint::UpdateNormalAndDepth, pinned
by hand-built cases with literal expected lists, and the scenes tests/test_gpu_map.py runs
checked for what that test relies on: the capacities hold the reference's results, the
histogram and the row sort of the wide map span more than 256 entries, and the float statement
of UpdateNormalAndDepth meets the float64 bounds.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402


@pytest.mark.parametrize("case", range(len(R.HAND_CASES)), ids=R.HAND_NAMES)
def test_hand_case(case):
    fn, expected = R.HAND_CASES[case]
    got = fn(R.RefMap())
    assert got == expected


def test_update_best_covisibles_is_the_pair_sort_reversed():
    M = R.RefMap()
    R._plain_points(M, 8)
    for s in range(5):
        M.set_keyframe(s, [])
    M.kf[0]["W"] = {1: 4, 2: 9, 3: 4, 4: 1}
    M.update_best_covisibles(0)
    assert M.ordered(0) == [(2, 9), (3, 4), (1, 4), (4, 1)]
    M.add_connection(0, 4, 1)          # unchanged: no re-sort
    M.kf[0]["ord"] = "untouched"
    M.add_connection(0, 4, 1)
    assert M.kf[0]["ord"] == "untouched"
    M.add_connection(0, 4, 4)          # changed
    assert M.ordered(0) == [(2, 9), (4, 4), (3, 4), (1, 4)]


def test_erase_connection_resorts_and_leaves_the_tree():
    M = R.RefMap()
    R.hand_bad_skipped(M)
    assert M.weights(0) == {3: 20, 4: 16}
    assert M.parent(2) == 0 and M.is_bad_kf(2) and M.ordered(2) == []


def test_local_points_order_first_occurrence_and_flags():
    M = R.RefMap()
    R._plain_points(M, 16)
    M.set_keyframe(0, [5, -1, 3, 7], root=True)
    M.set_keyframe(1, [3, 9, 5, 2])
    M.set_point_bad(7)
    got = M.local_points([1, 0, 1], [9, -1, 4])
    assert got == [(3, 3), (9, 2), (5, 3), (2, 3)]
    assert M.local_points([0], []) == [(5, 3), (3, 3)]


def test_normal_and_depth_float_statement():
    M = R.RefMap()
    M.set_points(0, [(0.0, 0.0, 4.0), (1.0, 2.0, 8.0)], [False, True], [[0] * 32] * 2, [1, 0])
    M.set_keyframe(0, [0, 1], [2, 3], (0.0, 0.0, 0.0), root=True)
    M.set_keyframe(1, [1, 0], [0, 5], (0.0, 3.0, 0.0))
    n, mind, maxd = M.normal_and_depth(0)
    # from (0,0,0): (0,0,1); from (0,3,0): (0,-3,4)/5; the reference keyframe is 1, octave 5
    assert np.allclose(n, [0.0, -0.3, 0.9], atol=1e-7)
    assert maxd == np.float32(np.float32(5.0) * M.scale[5])
    assert mind == np.float32(maxd / M.scale[7])
    assert M.normal_and_depth(1) is None            # bad
    assert R.check_normal_depth_bounds(M, [0, 1]) == 1


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_random_scenes_fit_the_capacities_and_bounds(seed):
    d = R.map_dataset(seed)
    M = R.RefMap()
    R.build_map(M, d)
    assert R.check_normal_depth_bounds(M, range(d["npts"])) > 1000
    for stage in range(2):
        below = sum(1 for s in M.kf for w in M.weights(s).values() if w < R.TH)
        listed = sum(len(M.ordered(s)) for s in M.kf)
        assert below > 20 and listed > 200
        nonempty = 0
        for fp in d["frames"]:
            assert len(fp) <= R.FRAME_CAP
            lk, ref, fp2 = M.local_keyframes(fp)
            if lk is None:
                continue
            nonempty += 1
            assert len(lk) <= R.LKF_CAP and ref is not None
            lp = M.local_points(lk, fp2)
            assert 0 < len(lp) <= R.LP_CAP
            assert any(not fl & R.MP_VALID for _, fl in lp) and any(fl & R.MP_VALID for _, fl in lp)
        assert nonempty >= R.NFRAMES - 2
        R.mutate_map(M, d)


def test_wide_scene_spans_more_than_256():
    d = R.wide_dataset()
    M = R.RefMap()
    R.build_wide(M, d)
    assert len(M.ordered(R.WIDE_HUB)) > 300 and len(M.weights(R.WIDE_HUB)) > 300
    o = M.ordered(R.WIDE_HUB)
    assert all(a[1] > b[1] or (a[1] == b[1] and a[0] > b[0]) for a, b in zip(o, o[1:]))
    lk, ref, _ = M.local_keyframes(d["frame"])
    assert len(lk) > 256 and lk == sorted(lk) and ref == R.WIDE_HUB
    assert max(lk) < R.WIDE_K and len(lk) <= 512
    assert len(M.local_points(lk, d["frame"])) <= 2048
