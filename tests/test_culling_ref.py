"""CPU: tests/ref_culling.py, the pure-Python statement of KeyFrame::SetBadFlag and
LocalMapping::KeyFrameCulling / MapPointCulling, pinned by hand-built cases with literal expected
values, and the scenes tests/test_gpu_culling.py runs checked for what that test relies on: the
random scenes erase keyframes, overturn start-of-call decisions, turn points bad, adopt through
promoted candidates and fall back; the wide map crosses a wave, a 256-lane pass and rec_cap.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_culling as RC  # noqa: E402


@pytest.mark.parametrize("case", range(len(RC.HAND_CASES)), ids=RC.HAND_NAMES)
def test_hand_case(case):
    fn, expected = RC.HAND_CASES[case]
    assert fn(RC.RefCullMap()) == expected


def test_threshold_is_the_double_comparison():
    """9 > 0.9 * 10 is false in double (0.9 * 10 rounds to 9.0); 10 > 9.0 and 1 > 0.9 hold;
    0 > 0.0 does not"""
    assert not float(9) > 0.9 * float(10)
    assert float(10) > 0.9 * float(10) and float(1) > 0.9 * float(1)
    assert not float(0) > 0.9 * float(0)


def test_new_state_defaults_and_overwrite():
    M = RC.RefCullMap()
    RC.R._plain_points(M, 8)
    assert M.point_stats(0, 2) == [(0, 1, 1, 0), (0, 1, 1, 0)]
    M.set_keyframe(3, [0, 1, 2])
    assert [M.feat(3, i) for i in range(3)] == [0, 0, 0]
    M.set_keyframe_features(3, [1, 2, 3])
    M.set_not_erase(3, True)
    M.set_keyframe(3, [0, 1, 5])                    # an overwrite keeps the keypoints' flags
    assert [M.feat(3, i) for i in range(3)] == [1, 2, 3] and M.kf[3]["not_erase"]
    assert M.point_stats(0, 3) == [(0, 1, 1, 2), (0, 1, 1, 1), (0, 1, 1, 0)]
    M.set_point_stats(1, visible=[7, 8])
    M.set_point_stats(2, first_kf=[4], found=[5])
    assert M.point_stats(1, 2) == [(0, 7, 1, 1), (4, 8, 5, 0)]
    M.increase_visible([1, -1, 1, 2], 2, mask=[1, 1, 0, 1])
    M.increase_found([2, 2], 3)
    assert M.point_stats(1, 2) == [(0, 9, 1, 1), (4, 10, 11, 0)]
    M.erase_keyframe(3)                             # the table side only: the point stays good
    M.set_keyframe(3, [4])                          # live again: everything cleared
    assert M.feat(3, 0) == 0 and not M.kf[3]["not_erase"] and not M.kf[3]["to_be_erased"]
    M.set_keyframe_features(9, [1])                 # a dead slot: no change
    assert 9 not in M.kf and M.set_bad_flag(9) == 0 and not M.set_not_erase(9, False)


def scene_figures(seed, stereo):
    d = RC.cull_dataset(seed, stereo)
    M = RC.RefCullMap()
    RC.build_cull_map(M, d)
    bad0 = sum(M.point_bad(0, RC.NPTS))
    erased = overturned = 0
    for s in RC.CULL_SLOTS:
        start = {}
        for t, _ in M.ordered(s):
            if M.cullable(t):
                nmps, nred = M.cull_score(t, not stereo)
                start[t] = float(nred) > 0.9 * float(nmps)
        rec = M.keyframe_culling(s, not stereo)
        assert len(rec) <= RC.MAX_KF
        erased += sum(1 for r in rec if r[1] == RC.ERASED)
        overturned += sum(1 for r in rec if r[1] != RC.SKIPPED and start[r[0]] != (r[1] != RC.KEPT))
    turned_bad = sum(M.point_bad(0, RC.NPTS)) - bad0
    keep, status = M.point_culling(d["recent"], RC.CURRENT_KF_ID, not stereo)
    return erased, overturned, turned_bad, M.n_promoted, M.n_fallback, status, M


@pytest.mark.parametrize("stereo", (False, True), ids=("mono", "stereo"))
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_random_scenes_exercise_the_culling(seed, stereo):
    erased, overturned, turned_bad, promoted, fallback, status, M = scene_figures(seed, stereo)
    assert erased >= 6 and overturned >= 5 and turned_bad >= 1
    assert promoted >= 2 and fallback >= 1
    assert all(status.count(k) >= 5 for k in range(5))
    # the spanning tree is still one: every live keyframe reaches the root through live ones
    for s in [s for s, k in M.kf.items() if k["live"]]:
        seen = set()
        while not M.kf[s]["root"]:
            assert M.kf[s]["live"] and s not in seen
            seen.add(s)
            s = M.kf[s]["parent"]


def test_not_erase_occurs_in_a_random_scene():
    d = RC.cull_dataset(0, False)
    plain = RC.run_cull_scene(RC.RefCullMap(), d)
    erased = [r[0] for rec in plain[:3] for r in rec if r[1] == RC.ERASED]
    marked = RC.run_cull_scene(RC.RefCullMap(), d, not_erase=erased[1])
    flat = [r for rec in marked[:3] for r in rec]
    assert any(r[0] == erased[1] and r[1] == RC.MARKED for r in flat)
    assert plain != marked


def test_wide_scene_spans_more_than_256():
    M = RC.RefCullMap()
    RC.build_wide_cull(M)
    lst = M.ordered(RC.WIDE_HUB)
    assert 256 < len(lst) <= RC.WIDE_K
    assert max(len(M.keyframe_points(s)) for s, _ in lst) > 256
    assert max(len(M.observations(p)) for p in range(15)) > 64
    rec = M.keyframe_culling(RC.WIDE_HUB, True)
    n = [sum(1 for r in rec if r[1] == k) for k in range(4)]
    assert n[RC.ERASED] > 64 and n[RC.KEPT] > 64
    assert [r[1] for r in rec[256:]].count(RC.ERASED) > 0      # past the first 256-entry pass
