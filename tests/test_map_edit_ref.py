"""CPU: tests/ref_map_edit.py, the pure-Python statement of MapPoint::Replace / AddObservation /
ComputeDistinctiveDescriptors, Fuse's map update and SearchInNeighbors, pinned with literal hand
cases; and a guard over the random scenes tests/test_gpu_map_edit.py uses: for each seed the
reference alone must reach every branch the GPU test is there to compare.  The guard's search is
the CPU oracle's fuse_search, the one the GPU test feeds to the reference.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_map as R  # noqa: E402
import ref_culling as RC  # noqa: E402
import ref_map_edit as RE  # noqa: E402

SCENES = ((0, False), (1, True), (2, False))


def no_search(M, slot, ids):
    return [-1] * len(ids), [256] * len(ids)


@pytest.mark.parametrize("case", range(len(RE.HAND_CASES)), ids=RE.HAND_NAMES)
def test_hand_case(case):
    fn, expected = RE.HAND_CASES[case]
    assert fn(RE.RefEditMap()) == expected


def _fuse_map(rows, feats=None):
    M = RE.RefEditMap()
    RE._hand_map(M, rows, feats)
    return M


def test_fuse_strict_tie():
    """equal Observations(): the feature's point is the one replaced"""
    M = _fuse_map({0: [10], 1: [10], 2: [11], 3: [11]})
    assert M.fuse(0, [11], [0], [10]) == (1, [RE.REPLACED_KF])
    assert [M.keyframe_points(s) for s in range(4)] == [[11], [11], [11], [11]]
    assert M.point_bad(10, 2) == [True, False] and M.point_replaced(10, 2) == [11, -1]
    # one more observation on the feature's side (a STEREO feature counts 2): the point goes
    M = _fuse_map({0: [10], 1: [10], 2: [11], 3: [11]}, {1: [RE.STEREO]})
    assert M.fuse(0, [11], [0], [10]) == (1, [RE.REPLACED_BY_KF])
    assert [M.keyframe_points(s) for s in range(4)] == [[10], [10], [10], [10]]
    assert M.point_stats(10, 1)[0][3] == 5


def test_fuse_status_0_4_5():
    M = _fuse_map({0: [10, -1, -1], 1: [10], 2: [11]})
    M.set_point_bad(10)
    # a bad point on the feature: counted, nothing done; no feature; too far; idx past the row
    assert M.fuse(0, [11, 12, 13, 14], [0, -1, 1, 3], [10, 256, 51, 5]) == (1, [4, 0, 0, 0])
    assert M.keyframe_points(0) == [10, -1, -1] and M.point_bad(11, 1) == [False]
    # the second occurrence is in the keyframe by its turn; a point that went bad by its turn
    M = _fuse_map({0: [10, -1, -1], 1: [10], 2: [11], 3: [12]})
    assert M.fuse(0, [11, 11, 12, 12], [1, 1, 0, 2], [5, 5, 50, 0]) == (2, [1, 5, 2, 5])
    assert M.keyframe_points(0) == [10, 11, -1] and M.keyframe_points(3) == [10]


def test_fuse_chain():
    """i is replaced by the feature's point S; j, with more observations, then replaces S:
    every observation i handed to S arrives at j"""
    M = _fuse_map({0: [10], 1: [10], 2: [-1, 11], 3: [12], 4: [12], 5: [12], 6: [12, 10]})
    assert M.fuse(0, [11, 12], [0, 0], [3, 3]) == (2, [RE.REPLACED_BY_KF, RE.REPLACED_KF])
    # keyframe 6 held both S and j: S's entry there is erased, not moved
    assert [M.keyframe_points(s) for s in range(7)] == [[12], [12], [-1, 12], [12], [12], [12],
                                                        [12, -1]]
    assert M.point_bad(10, 3) == [True, True, False]
    assert M.point_replaced(10, 3) == [12, 10, -1]
    assert M.point_stats(12, 1)[0][3] == 7


def test_distinctive_median_and_ties():
    M = _fuse_map({0: [10], 1: [10], 2: [10], 3: [10]})
    z = np.zeros(32, np.uint8)

    def d(nbits):
        v = np.zeros(256, np.uint8)
        v[:nbits] = 1
        return np.packbits(v)
    # distances from row i: sorted, then vDists[int(0.5 * 3)] = vDists[1]
    M.kfdesc = {0: np.stack([d(8)]), 1: np.stack([z]), 2: np.stack([d(2)]), 3: np.stack([d(4)])}
    # rows: [0,8,6,4] [0,8,2,4] [0,6,2,2] [0,4,4,2] -> medians 4, 2, 2, 2: the first of the ties
    M.distinctive(10)
    assert M.mp[10]["desc"] == bytes(32)
    M.set_keyframe(1, [10], bad=True)          # a bad keyframe's descriptor is left out
    M.distinctive(10)                          # rows [0,6,4] [0,6,2] [0,4,2] -> medians 4, 2, 2
    assert M.mp[10]["desc"] == d(2).tobytes()


def test_target_list_duplicates():
    rows = {s: [s] for s in range(8)}
    M = _fuse_map(rows)
    M.set_keyframe(7, [7], bad=True)
    lists = {0: [1, 2, 3], 1: [0, 4, 3, 5], 2: [4, 1, 6], 3: [7], 4: [], 5: [], 6: [], 7: []}
    for s, l in lists.items():
        M.kf[s]["ord"] = [(t, 20 - i) for i, t in enumerate(l)]
    # 4 twice (second level of 1 and of 2); 3 as second level of 1, then as a first-level entry
    want = [1, 4, 3, 5, 2, 4, 6, 3]
    assert M.target_keyframes(0, 9, True) == want
    assert M.search_in_neighbors(0, 9, True, no_search) == (want, [0] * 8, 0)
    assert M.target_keyframes(0, 0, True) == []
    assert M.search_in_neighbors(0, 0, True, no_search) == ([], [], 0)


# ---------------------------------------------------------------------------
# the random scenes of the GPU test
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_run(oracle, seed, stereo):
    import test_oracle_mapping as T
    sf, isg = T._fuse_tables(oracle)
    d = RE.edit_dataset(seed, stereo)
    M = RE.RefEditMap()
    M.search = RE.make_search(oracle.fuse_search, sf, isg)
    states = []
    out = RE.run_edit_scene(M, d, lambda stage: states.append((stage, RE.state(M, RE.MAX_KF, RE.NPTS))))
    return d, M, out, states


def test_chain_scene(oracle):
    import test_oracle_mapping as T
    sf, isg = T._fuse_tables(oracle)
    M = RE.RefEditMap()
    M.search = RE.make_search(oracle.fuse_search, sf, isg)
    assert RE.hand_chain(M) == RE.HAND_CHAIN


@pytest.mark.parametrize("seed,stereo", SCENES)
def test_random_scene_reaches_every_branch(oracle, seed, stereo):
    d, M, out, states = reference_run(oracle, seed, stereo)
    fuse, repl, add, sin0, sin1, sin_id0 = out
    for st in (1, 2, 3, 5):
        assert fuse[1].count(st) >= 1, st
    assert repl.count(0) >= 5 and repl[-2:] == [1, 3] and set(add) == {0, 5}
    for targets, nfused, second in (sin0, sin1):
        assert len(targets) > len(set(targets))          # a duplicate in the target list
        assert sum(nfused) > 0 and second > 0            # both passes fuse something
    assert sin_id0 == ([], [], 0)
    assert M.n_desc_changed > 0
    before, after = dict(states)["add"], dict(states)["sin0"]
    assert before["rows"] != after["rows"] and before["graph"] != after["graph"]
