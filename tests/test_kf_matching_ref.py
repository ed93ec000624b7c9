"""CPU: the oracle's KeyFrame-side matchers against tests/ref_kf_matching.py.

ref_kf_matching states both SearchByBoW forms, SearchForTriangulation, both Fuse forms and
SearchBySim3 from the reference's text, in float64 with a margin on every float decision.
Here the oracle (bow_oracle.c, mapping_oracle.c, loop_oracle.c) is held to it on the scenes
of kf_matching_scenes.py, exactly, after the margin filter.
test_scenes_exercise_what_they_claim reads the counters the reference runs return and proves
that every boundary the scenes were designed for was reached;
test_scenes_tell_the_rules_apart proves, per wrong-rule variant, that a scene would notice.

Measured here (the cap asserted is the project's 2 %): the filter drops nothing on a designed
scene and at most 0.05 % of a generated one.
"""
from collections import Counter

import numpy as np
import pytest

import kf_matching_scenes as S
import ref_kf_matching as R


# ---------------------------------------------------------------- the module's own statements
def _kps(xy, octave=0):
    k = np.zeros(len(xy), S.KP_DTYPE)
    k["x"], k["y"] = [p[0] for p in xy], [p[1] for p in xy]
    k["octave"] = octave
    return k


def test_grid_on_image_bounds():
    """640 x 480: cells of 10 px, PosInGrid rounds half away, the last half cell is in no
    cell; candidates come cell by cell, column outer, row inner, index order inside."""
    k = _kps([(4.9, 4.9), (5.1, 5.1), (634.9, 474.9), (635.1, 100.0), (100.0, 475.1), (0.0, 0.0),
              (107.0, 100.0), (93.0, 107.0), (93.0, 93.0), (101.0, 101.0), (102.0, 101.0)])
    g = R.KeyFrameGrid(k, S.IMG)
    assert g.cell_of[:6] == [(0, 0), (1, 1), (63, 47), None, None, (0, 0)]
    # (93, 93) is cell (9, 9), (93, 107) cell (9, 11), (101 / 102, 101) cell (10, 10), (107, 100)
    # cell (11, 10)
    assert g.features_in_area(100.0, 100.0, 8.0) == [8, 7, 9, 10, 6]
    assert g.features_in_area(100.0, 100.0, 7.0) == [9, 10]          # |dx| == r is outside
    area = lambda variant, r: R.KeyFrameGrid(k, S.IMG, variant).features_in_area(100.0, 100.0, r)
    assert area("window_le", 7.0) == [8, 7, 9, 10, 6]
    assert area("tie_by_index", 8.0) == [6, 7, 8, 9, 10]
    assert g.is_in_image(0.0, 0.0) and g.is_in_image(639.99, 479.99)
    assert not g.is_in_image(640.0, 10.0) and not g.is_in_image(10.0, 480.0)
    assert not g.is_in_image(-0.01, 10.0)
    assert R.KeyFrameGrid(k, S.IMG, "grid_floor").cell_of[:4] == [(0, 0), (0, 0), (63, 47),
                                                                  (63, 10)]


def test_grid_on_fractional_bounds():
    """The grid on the float bounds, IsInImage and the cell range on the truncated ones."""
    b = S.TUM1                                  # int bounds (10, 1230, 14, 370)
    cw = (np.float32(b[1]) - np.float32(b[0])) / 64.0
    k = _kps([(12.5, 16.25), (float(np.float32(b[0])) + 63.49 * cw, 100.0),
              (float(np.float32(b[0])) + 63.51 * cw, 100.0)])
    g = R.KeyFrameGrid(k, b)
    assert g.ib == (10.0, 1230.0, 14.0, 370.0)
    assert g.cell_of == [(0, 0), (63, 12), None]
    assert g.is_in_image(10.0, 14.0) and g.is_in_image(10.5, 14.25)      # left of / above the grid
    assert not g.is_in_image(1230.0, 100.0) and not g.is_in_image(1230.03125, 100.0)
    assert not g.is_in_image(100.0, 370.0) and g.is_in_image(1229.9, 369.9)
    assert g.features_in_area(10.5, 14.25, 4.0) == [0]
    f = R.KeyFrameGrid(k, b, "kf_float_bounds")
    assert not f.is_in_image(10.5, 14.25) and f.is_in_image(1230.03125, 100.0)
    # exact half cells on power-of-two bounds
    g = R.KeyFrameGrid(_kps([(508.0, 8.0), (-4.0, 8.0), (507.9, 8.0), (8.0, 380.0), (4.0, 4.0)]),
                       S.POW2)
    assert g.cell_of == [None, None, (63, 1), None, (1, 1)]


def test_predict_scale():
    lsf = S.LOG_SF
    assert R.predict_scale(4.0, 4.0, lsf, 8) == 0                        # ratio 1: log 0
    assert R.predict_scale(4.0, 4.8, lsf, 8) == 0                        # v about -1: clamped
    assert R.predict_scale(4.0, 4.0 / 1.2 ** 2.5, lsf, 8) == 3
    assert R.predict_scale(4.0, 4.0 / 1.2 ** 3.5, lsf, 8) == 4
    assert R.predict_scale(4.0, 4.0 / 1.2 ** 6.5, lsf, 8) == 7
    assert R.predict_scale(4.0, 4.0 / 1.2 ** 11, lsf, 8) == 7            # clamped
    assert R.predict_scale(4.0, 4.0 / 1.2 ** 11, lsf, 4) == 3
    M = R.Margins()
    R.predict_scale(4.0, 4.0, lsf, 8, M, ("q", 0))
    assert not M.ambiguous()                                             # exact, margin 0
    R.predict_scale(4.0, float(np.float32(4.0 / 1.2 ** 3)), lsf, 8, M, ("q", 1))
    assert M.who("q") == [1]                                             # v within rounding of 3
    sf, s2, inv = R.level_tables()
    assert float(s2[1]) == float(np.float32(1.2) * np.float32(1.2)) and s2[0] == 1 and inv[0] == 1
    assert float(inv[2]) == float(np.float32(1.0) / s2[2])


def test_epipolar_rule():
    s2 = R.level_tables()[1]
    F = np.array(S.F_ROWS, np.float32)          # the line of (x1, y1) is y = y1
    assert R.epipolar_ok((100.0, 100.0, 0), (50.0, 101.5, 0), F, s2)         # 2.25 < 3.84
    assert not R.epipolar_ok((100.0, 100.0, 0), (50.0, 102.0, 0), F, s2)     # 4
    assert R.epipolar_ok((100.0, 100.0, 0), (50.0, 107.0, 7), F, s2)         # 49 < 49.30
    assert not R.epipolar_ok((100.0, 100.0, 0), (50.0, 107.25, 7), F, s2)
    # a general line: l = (1, 2, -3) for kp1 = (0, 0); (1, 1) is on it, (2, 2) at 9 / 5
    F = np.array([0, 0, 0, 0, 0, 0, 1, 2, -3], np.float32)
    assert R.epipolar_ok((0.0, 0.0, 0), (1.0, 1.0, 0), F, s2)
    assert R.epipolar_ok((0.0, 0.0, 0), (2.0, 2.0, 0), F, s2)                # 1.8
    assert not R.epipolar_ok((0.0, 0.0, 0), (3.0, 3.0, 0), F, s2)            # 36 / 5
    assert not R.epipolar_ok((0.0, 0.0, 0), (1.0, 1.0, 0), np.zeros(9, np.float32), s2)   # den 0
    (ex, _, x), (ey, _, y) = R.epipole(S.tri_geom(Cw1=(0.25, -0.5, 2.0)))
    assert (ex, ey) == (384.0, 112.0) and x and y


def test_node_walk():
    C = Counter()
    assert R.common_nodes(np.array([1, 4, 6, 9]), np.array([0, 4, 5, 9, 12]), C) == [(1, 1), (3, 3)]
    assert C["only_side1"] == 2 and C["only_side2"] == 2
    assert R.common_nodes(np.array([], np.int64), np.array([3]), C) == []


# ---------------------------------------------------------------- oracle == reference
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_oracle_equals_reference(oracle, name):
    s = S.scene(name)       # margin filter: nothing ambiguous left, at most 2 % dropped
    r = S.check_equal(S.run_oracle(oracle, s), s, name)
    assert s["dropped"] <= S.DROP_CAP
    assert not (name in S.DESIGNED_ROTATION and s["ori_dropped"])
    if "designed" in name or name.split("_", 1)[1] in ("chunks", "ties", "second", "walk", "shared"):
        assert s["dropped"] == 0
    print("%s: %s, dropped %.4f, decisions %d" % (name, S.outputs(r, s["kind"])[0], s["dropped"],
                                                  r.margins.count))


def _counters(kinds):
    C = Counter()
    for name in S.SCENE_NAMES:
        s = S.scene(name)
        if s["kind"] in kinds:
            C.update(S.run_ref(s).counters)
    return C


BOW_KEYS = (["cand_node_size=%d" % n for n in (1, 63, 64, 65, 127, 128, 129, 192, 193)]
            + ["walk_node_size=%d" % n for n in (1, 64, 65, 129)]
            + ["walk_skip_pos=%d" % p for p in (0, 63, 64)]
            + ["best_at_chunk_end=%d" % c for c in (0, 1, 2, 3)]
            + ["taken_nearest_chunk%d" % c for c in (0, 1, 2)]
            + ["walk_last_matched", "bow_tie_first_kept", "bow_tie_across_chunks",
               "best_second_same_lane", "best_second_same_chunk", "second_equals_best",
               "later_walker_takes_next", "later_walker_fails_ratio", "ratio_equal",
               "walk_node_index%1024=0", "walk_node_index%1024=1023", "only_side1", "only_side2",
               "common_at_other_index0", "common_at_other_last", "rot_removed"])
TRI_KEYS = (["cand_node_size=%d" % n for n in (1, 63, 64, 65, 127, 128, 129, 192, 193)]
            + ["walk_node_size=%d" % n for n in (1, 64, 65, 129)]
            + ["walk_skip_pos=%d" % p for p in (0, 63, 64)]
            + ["best_at_chunk_end=%d" % c for c in (0, 1, 2, 3)]
            + ["tri_epipole_%s_oct%d" % (w, o) for w in ("pass", "reject") for o in (0, 7)]
            + ["tri_epipolar_%s_oct%d" % (w, o) for w in ("pass", "reject") for o in (0, 7)]
            + ["walk_last_matched", "tri_tie_last_wins", "tri_tie_across_chunks",
               "tri_uright_zero_stereo", "tri_only_stereo_skip1", "tri_only_stereo_skip2",
               "tri_epipole_skipped_stereo", "tri_den_zero", "tri_shared_kf2_by3",
               "walk_node_index%1024=0", "walk_node_index%1024=1023", "only_side1", "only_side2",
               "common_at_other_index0", "common_at_other_last", "rot_removed"])
GRID_KEYS = (["kp_pos_hi_no_cell", "kp_pos_lo_no_cell", "kp_pos_last_cell",
              "in_image_left_of_grid", "out_by_int_max", "u_eq_int_min", "u_eq_int_max",
              "z_zero", "z_neg", "z_tiny", "dist_eq_min", "dist_lt_min", "dist_eq_max",
              "dist_gt_max", "lvl_exact0", "lvl_clamp_lo", "lvl_clamp_hi",
              "level_reject_nearest_below", "level_reject_nearest_above", "window_edge",
              "tie_ix_higher_index_wins", "tie_iy_higher_index_wins",
              "tie_cell_lower_index_wins", "invalid_point"]
             + ["lvl=%d" % n for n in (0, 1, 3, 4, 7)])


def test_scenes_exercise_what_they_claim():
    """Every boundary the scenes were designed for is reached by a reference run (counters of
    ref_kf_matching; each at least 1)."""
    for kinds, keys in ((("bow",), BOW_KEYS + ["bow_kff_best=%d" % d for d in (49, 50, 51)]),
                        (("bowkf",), BOW_KEYS + ["bow_kfkf_best=%d" % d for d in (49, 50, 51)]
                         + ["invalid_nearest_chunk%d" % c for c in (0, 1, 2)]
                         + ["invalid_skip_chunk%d" % c for c in (0, 1, 2)]),
                        (("tri",), TRI_KEYS),
                        (("fuse",), GRID_KEYS + ["cos_eq_half", "cos_lt_half", "chi2_mono_pass",
                                                 "chi2_mono_reject", "chi2_stereo_pass",
                                                 "chi2_stereo_reject", "uright_zero_stereo",
                                                 "no_uright_array", "fuse_best=50",
                                                 "fuse_best=51"]),
                        (("fuse_sim3",), GRID_KEYS + ["cos_lt_half", "fuse_sim3_best=50",
                                                      "fuse_sim3_best=51"]),
                        (("sim3",), GRID_KEYS + ["sim3_best=100", "sim3_best=101", "sim3_mutual",
                                                 "sim3_one_way_only", "sim3_dir1_matched_skip",
                                                 "sim3_dir2_matched_skip"])):
        C = _counters(kinds)
        missing = [k for k in keys if C[k] < 1]
        assert not missing, (kinds, missing)
    # decided exactly on a boundary (margin 0, every value on the path a float32 number), per
    # kind of decision; and the designed scenes hold no ambiguity at all
    B = Counter()
    for name in S.SCENE_NAMES:
        s = S.scene(name)
        B.update({(s["kind"], k): v for k, v in S.run_ref(s).margins.on_boundary.items()})
        if "designed" in name:
            assert s["dropped"] == 0, name
    want = [(k, "ratio") for k in ("bow", "bowkf")]
    want += [("tri", k) for k in ("epipole", "epipolar_den")]
    want += [(k, d) for k in ("fuse", "fuse_sim3", "sim3")
             for d in ("in_image", "dist_gate", "window", "predict_scale", "pos_in_grid")]
    want += [("fuse", "view_cos")]
    assert not [w for w in want if B[w] < 1], [w for w in want if B[w] < 1]
    # the rotation filter removes and keeps on every designed histogram, with no ambiguity
    for name in S.DESIGNED_ROTATION:
        s = S.scene(name)
        r = S.run_ref(s)
        assert s["ori"] and r.counters["rot_removed"] > 0 and r.nmatches > 0, name
    # a KF2 feature serving several KF1 features is counted once per KF1 feature
    r = S.run_ref(S.scene("tri_shared"))
    assert r.nmatches > len(set(r.match[r.match >= 0].tolist()))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_scenes_tell_the_rules_apart(variant):
    """Every wrong-rule variant changes the reference's result on at least one filtered scene
    (nothing ambiguous is left in those, under the right rule or the variant)."""
    hit = []
    for name in S.SCENE_NAMES:
        s = S.scene(name)
        a, b = S.run_ref(s), S.run_ref(s, variant)
        if [x for x in b.margins.ambiguous() if x[1][0] != "range"]:
            continue
        if any(not np.array_equal(x, y) for x, y in zip(S.outputs(a, s["kind"]),
                                                        S.outputs(b, s["kind"]))):
            hit.append(name)
    print(variant, hit)
    assert hit, variant


def test_filter_share():
    worst = max((S.scene(n)["dropped"], n) for n in S.SCENE_NAMES)
    print("largest dropped share %.4f (%s)" % worst)
    assert worst[0] <= S.DROP_CAP
