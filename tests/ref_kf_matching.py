"""An independent NumPy statement of the KeyFrame-side matchers.

The HIP kernels k_bow_match (csrc/bow_match_kernels.hip) and k_tri_match, k_fuse, k_sim3_match
and k_sim3_resolve (csrc/mapping_kernels.hip) are compared bit for bit with oracle/bow_oracle.c,
mapping_oracle.c and loop_oracle.c, C written next to the kernels from one reading of the
reference.  This module states the same operations a second time from the reference's text, in
float64 and exact integers, without importing oracle/ or the package:

    search_by_bow             SearchByBoW(KeyFrame*, Frame&, ...), ORBmatcher.cc:195-348
    search_by_bow_kf          SearchByBoW(KeyFrame*, KeyFrame*, ...), ORBmatcher.cc:634-769
    search_for_triangulation  ORBmatcher.cc:779-957, CheckDistEpipolarLine :165-182
    KeyFrameGrid              the Frame's grid (Frame.cc:292-307, PosInGrid :510-520) under
                              KeyFrame::GetFeaturesInArea (KeyFrame.cc:750-789) and IsInImage
                              (:792-795) on the int bounds of KeyFrame.h:288-291
    predict_scale             MapPoint::PredictScale, MapPoint.cc:557-572; the distance
                              gates are GetMin/MaxDistanceInvariance, :520-530
    fuse                      Fuse(pKF, vpMapPoints, th), ORBmatcher.cc:968-1124
    fuse_sim3                 Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), :1133-1260
    search_by_sim3            ORBmatcher.cc:1262-1486
    level_tables              mvLevelSigma2 / mvInvLevelSigma2, ORBextractor.cc:438-457

tests/test_kf_matching_ref.py holds the oracle to it on the CPU, tests/
test_gpu_kf_matching_ref.py the kernels on the GPU.

Interface conventions (of the test interface, shared with orb_slam2_test_amd/orbmatcher.py;
they are not rules of the reference).  A FeatureVector is (nodes, off, feats): node ids
ascending, node k's features feats[off[k]:off[k + 1]] in their order.  search_by_bow returns
per Frame feature the KeyFrame feature whose MapPoint was written to vpMapPointMatches, -1 for
NULL; search_by_bow_kf and search_for_triangulation return per KF1 feature the KF2 feature,
-1.  valid[i] stands for "pMP && !pMP->isBad()", has_mp[i] for "GetMapPoint(i) != NULL".  A
map point is a record (x, y, z, nx, ny, nz, min_dist, max_dist, flags) with flags & 1 = the
loop's guards pass.  fuse / fuse_sim3 return (n, bestIdx, bestDist) per map point with
bestIdx = -1 unless bestDist <= 50, and bestDist = 256 where nothing was a candidate (the
reference starts the Sim3 form at INT_MAX; 256 is the interface's "none", not the
reference's); the Replace / AddObservation update that follows is the caller's.
search_by_sim3 returns per KF1 feature the KF2 feature newly written to vpMatches12, -1;
matched1 / matched2 are vbAlreadyMatched1 / 2 as flags.

Float decisions follow ref_matching.py's method: the reference computes in float32, this
module in float64 from the same float32 inputs; every comparison whose outcome could differ
is recorded in a Margins with its margin and a derived bound; a decision is ambiguous when
margin < bound, unless margin == 0 and every intermediate value on the path is a float32
number (then float32 arithmetic computes the same values and the outcome is the same).  The
same argument makes the error of a value 0, whatever the margin, where the value and
everything it was computed from are float32 numbers: the scenes that sit one float32 step
either side of a gate depend on it.

Derived bounds.  U = 2^-24.  cv::Mat products (R * x + t, -R^T * t) are cv::gemm: double
accumulation, one float32 rounding per component; Mat::dot and cv::norm
accumulate in double; scalar float expressions round at every operation.
  camera point     Pc = Rcw x + tcw by gemm: e(Pc_k) = U |Pc_k|.  In the Sim3 forms the
                   matrix has a relative error eM (below): e(Pc_k) = sum_j |M_kj| e(x_j)
                   + eM sum_j |M_kj x_j| + e(t_k) + U |Pc_k|.
  Sim3 scale       fuse_sim3: scw = sqrt(row0 . row0) (double dot, 1 rounding), Rcw = sRcw /
                   scw and tcw = t / scw as Mat * (float)(1 / scw): 3 roundings, eM = 3 U.
                   search_by_sim3: sR12 = s12 * R12 1 rounding (eM = U); sR21 = (1 / s12)
                   R12^T 2 roundings (eM = 2 U); t21 = -sR21 t12 by gemm.  Not a comparison:
                   reported as kind "sim3_scale" with margin 1 and bound eM, and carried into
                   every projection as the error of an inexact input.  A power-of-two scale
                   and an axis-aligned rotation make it exact.
  sign of z        margin |z|, bound e(z): never ambiguous for the plain gemm (U |z| < |z|).
  u, v             invz = 1 / z, x = Pc_x invz, u = fx x + cx: 4 roundings after Pc_x and
                   Pc_z (U each): e(u) = 6 U max(|fx x|, |cx|, |u|) + fx (e(Pc_x) + |x| e(z))
                   / z - the last term only where Pc carries more than its own rounding.
  u, v in image    against (float)(int)bound: margin |u - bound|, bound e(u).
  dist3D           Fuse: Ow = -Rcw^T tcw by gemm (U |Ow|), PO = x - Ow (1 rounding), norm in
                   double and 1 rounding: e = 5 U max(|x|, |Ow|, dist3D) (+ 6 U |Ow| in the
                   Sim3 form for eM on both factors).  SearchBySim3: norm of Pc:
                   e = sum_k e(Pc_k) + U dist3D.
  distance gates   0.8f * min_dist, 1.2f * max_dist: 1 rounding each.  Margin |dist3D -
                   gate|, bound e(dist3D) + U gate.
  viewing cosine   PO . Pn in double against 0.5 * dist3D in double: no rounding of its own;
                   bound sum_k |Pn_k| e(PO_k) + 0.5 e(dist3D), e(PO_k) <= 2 U max(|x|, |Ow|).
  PredictScale     ratio = max_dist / dist3D (1 rounding), v = log(ratio) / logScaleFactor,
                   ceil.  log may be float or double depending on the overload the compiler
                   picks, so both are covered: e(v) = (e(dist3D) / dist3D + U + 3 U |log
                   ratio|) / logScaleFactor + U |v|.  Margin: distance of v from the nearest
                   integer, recorded only where that integer is 0 .. nlevels - 2 (elsewhere
                   the clamp gives one level either way).  ratio == 1 exactly gives v = 0.
  radius           th * scale[lvl]: 1 rounding.
  cell range       (u - (float)(int)mnMinX -+ r) * inv: 5 roundings at the largest magnitude
                   times inv, plus (e(u) + e(r)) inv.  A flip cannot change the result (see
                   ref_matching.py); reported all the same.
  pos_in_grid      as ref_matching.py: 4 U |pos|.
  window           |kp.x - u| < r: U |kp.x - u| + e(u) + e(r).
  chi-square       ex = u - kp.x (1), e2 = ex^2 + ey^2 (3; with er^2 5, er = ur - kp.ur with
                   ur = u - bf invz 2 more), q = e2 invSigma2 (1), compared in double with
                   5.99 / 7.8: e(q) = invSigma2 sum 2 |e_k| (e(u) + U |e_k|) + 6 U q (8 U q).
  epipole          C2 by gemm, invz, ex = fx C2_x invz + cx: e(ex) = 6 U max(|fx C2_x invz|,
                   |cx|, |ex|).  d2 = (ex - x)^2 + (ey - y)^2 against 100 * scale[octave]
                   (1 rounding): e(d2) = 2 |dx| (e(ex) + U |dx|) + 2 |dy| (...) + 3 U d2.
  epipolar dist    a, b, c: 4 roundings each at their largest term; num 4 more; den 3;
                   dsqr = num^2 / den 2; against 3.84 * sigma2 in double (no rounding):
                   e(dsqr) = (2 |num| e(num) + e(num)^2) / den + dsqr (e(den) / den + 3 U).
                   den == 0: margin den, bound e(den).
  ratio            bestDist1 against mfNNratio * bestDist2: 1 rounding at the product.
  rotation bin, three-maxima cut: ref_matching.py's.
Exact without a bound: Hamming distances, the TH_LOW / TH_HIGH tests, the octave window, the
taken / valid / has_mp flags, uRight >= 0 (inputs), the node walk.

Wrong-rule variants (variant=..., for the tests' sharpness check only): tie_by_index,
window_le, grid_floor, kf_float_bounds, level_window_wide, tri_first_min, tri_taken,
no_epipole_test, kfkf_le_th_low, kff_lt_th_low, bow_not_taken, second_is_next_distinct,
sim3_one_way, fuse_th_high.

Line ranges are those of the reference tree.  The kernels' and the oracle's headers cite
the same starts; a few of their ends stop short of the function (Fuse's search runs to :1098
and the function to :1124, not :1069; the Sim3 Fuse to :1260, not :1238; SearchBySim3 to
:1486, not :1470) and two single lines are a few off (vbMatched2 is declared at :804, the
`dist>TH_LOW || dist>bestDist` test is :869).  None of that changes a rule.

Rules this module had wrong at first:
  * No matching rule: the oracle equalled the first draft on every scene.  What the draft had
    wrong was the bookkeeping of exactness.  It charged U |value| to every cv::gemm result
    and U * gate to every distance gate even where the value was a float32 number computed
    from float32 numbers, so the designed scenes that sit exactly on a bound, or one float32
    step either side of 0.8f * min_dist, 1.2f * max_dist and cos = 0.5, were flagged
    ambiguous and filtered away - the opposite of what they are for.  An exact value now
    carries error 0 (see "Float decisions").
  * A premise of the scenes, not of the module: Fuse's chi-square gate (5.99 at level 0)
    rejects a keypoint 3.5 px away before any tie or window rule can show, so the grid ties
    use offsets of 1 px around a cell boundary and the |dx| == r case of Fuse runs at th = 2.
    Across TUM1's 9.5 px half cell in x no monocular or stereo candidate passes the gate at
    any level: that boundary is checked in y, and in x by the two Sim3 searches.
Rules the oracle had wrong: none found; the kernels equalled this module on every scene too.

Measured maxima (the cap the tests assert is the project's, not a measurement):
  CPU, oracle against this module (tests/test_kf_matching_ref.py): all 93 scenes equal in
    every output array and count after the margin filter.  Dropped share per scene: 0 on
    every designed scene and on the generated BoW / triangulation / Fuse scenes; 0.05 % on
    sim3_n1025 (one keypoint of 2050), the largest (cap 2 %).
  GPU (MI355X), kernels against this module (tests/test_gpu_kf_matching_ref.py): every scene
    and every batch call equal, at every capacity.
"""
import math
from collections import Counter

import numpy as np

from ref_matching import Margins as _Margins
from ref_matching import Result, U, _round, hamming, rot_bin, scale_factors, three_maxima

GRID_COLS, GRID_ROWS = 64, 48
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
MP_VALID = 1
NONE_DIST = 256
VARIANTS = ("tie_by_index", "window_le", "grid_floor", "kf_float_bounds", "level_window_wide",
            "tri_first_min", "tri_taken", "no_epipole_test", "kfkf_le_th_low", "kff_lt_th_low",
            "bow_not_taken", "second_is_next_distinct", "sim3_one_way", "fuse_th_high")


class Margins(_Margins):
    """ref_matching's Margins, counting per kind the decisions that sit exactly on their
    boundary (margin 0) and are exact."""

    def __init__(self):
        super().__init__()
        self.on_boundary = Counter()

    def add(self, kind, who, margin, bound, exact=False):
        if margin == 0 and exact:
            self.on_boundary[kind] += 1
        super().add(kind, who, margin, bound, exact)


def _f32(v):
    return float(np.float32(v))


def _is_f32(*vals):
    return all(math.isfinite(v) and float(np.float32(v)) == float(v) for v in vals)


def level_tables(scale_factor=1.2, nlevels=8):
    """(mvScaleFactor, mvLevelSigma2, mvInvLevelSigma2) as float32 arrays."""
    sf = scale_factors(scale_factor, nlevels)
    s2 = (sf * sf).astype(np.float32)
    s2[0] = 1.0
    return sf, s2, (np.float32(1.0) / s2).astype(np.float32)


# ---------------------------------------------------------------- the FeatureVector walk
def _fv(fv):
    nodes, off, feats = (np.asarray(a, np.int64) for a in fv)
    return nodes, off, feats


def common_nodes(nodes1, nodes2, C=None):
    """The two-iterator walk with lower_bound (ORBmatcher.cc:225-320): (a, b) index pairs."""
    a = b = 0
    out = []
    while a < len(nodes1) and b < len(nodes2):
        if nodes1[a] == nodes2[b]:
            out.append((a, b))
            a += 1
            b += 1
        elif nodes1[a] < nodes2[b]:
            a2 = a + int(np.searchsorted(nodes1[a:], nodes2[b], "left"))
            if C is not None:
                C["only_side1"] += a2 - a
            a = a2
        else:
            b2 = b + int(np.searchsorted(nodes2[b:], nodes1[a], "left"))
            if C is not None:
                C["only_side2"] += b2 - b
            b = b2
    if C is not None:
        for a, b in out:
            C["walk_node_index%%1024=%d" % (a % 1024)] += (a % 1024) in (0, 1023)
            C["common_at_other_index0"] += b == 0
            C["common_at_other_last"] += b == len(nodes2) - 1
            C["common_at_walk_index0"] += a == 0
            C["common_at_walk_last"] += a == len(nodes1) - 1
    return out


def _size_class(n):
    return n if n in (1, 63, 64, 65, 127, 128, 129, 192, 193) else None


def _ori_filter(hist, M):
    keep = three_maxima([len(h) for h in hist], M)
    return [x for b in range(HISTO_LENGTH) if b not in keep for x in hist[b]]


# ---------------------------------------------------------------- the two SearchByBoW forms
def _bow(desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2, nnratio, check_ori, kfkf,
         variant):
    """Side 1 is walked (the KeyFrame / pKF1), side 2 holds the candidates (F / pKF2)."""
    M, C = Margins(), Counter()
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    n1, n2 = len(desc1), len(desc2)
    valid1 = np.ones(n1, bool) if valid1 is None else np.asarray(valid1).astype(bool)
    valid2 = np.ones(n2, bool) if valid2 is None else np.asarray(valid2).astype(bool)
    nodes1, off1, feats1 = _fv(fv1)
    nodes2, off2, feats2 = _fv(fv2)
    nn = _f32(nnratio)
    taken = np.zeros(n2, bool)
    m12 = np.full(n1, -1, np.int64)
    m21 = np.full(n2, -1, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    le = (variant == "kfkf_le_th_low") if kfkf else (variant != "kff_lt_th_low")
    for a, b in common_nodes(nodes1, nodes2, C):
        f1 = feats1[off1[a]:off1[a + 1]]
        f2 = feats2[off2[b]:off2[b + 1]]
        if _size_class(len(f2)):
            C["cand_node_size=%d" % len(f2)] += 1
        if len(f1) in (1, 64, 65, 129):
            C["walk_node_size=%d" % len(f1)] += 1
        for p1, i1 in enumerate(f1):
            who = ("n1", int(nodes1[a]))
            if not valid1[i1]:
                if p1 in (0, 63, 64):
                    C["walk_skip_pos=%d" % p1] += 1
                continue
            d = hamming(desc1[i1], desc2[f2]) if len(f2) else []
            best = best2 = 256
            bi = bpos = spos = -1
            skipped = []
            for p2, i2 in enumerate(f2):
                dd = int(d[p2])
                if taken[i2] and variant != "bow_not_taken":
                    skipped.append(("taken", p2, dd))
                    continue
                if kfkf and not valid2[i2]:
                    skipped.append(("invalid", p2, dd))
                    continue
                if dd < best:
                    best2, spos = best, bpos
                    best, bi, bpos = dd, int(i2), p2
                elif dd < best2 and not (variant == "second_is_next_distinct" and dd == best):
                    best2, spos = dd, p2
                if dd == best and p2 != bpos:
                    C["bow_tie_first_kept"] += 1
                    if bpos % 64 == 63 and p2 == bpos + 1:
                        C["bow_tie_across_chunks"] += 1
            for kind, p2, dd in skipped:
                C["%s_skip_chunk%d" % (kind, min(p2 // 64, 2))] += 1
                if dd < best:
                    C["%s_nearest_chunk%d" % (kind, min(p2 // 64, 2))] += 1
            if best in (49, 50, 51) and best2 >= 100:
                C["bow_%s_best=%d" % ("kfkf" if kfkf else "kff", best)] += 1
            if not (best <= TH_LOW if le else best < TH_LOW):
                continue
            thr = nn * float(best2)
            M.add("ratio", who, abs(best - thr), U * thr, _is_f32(thr))
            if best == thr:
                C["ratio_equal"] += 1
            if best2 == best:
                C["second_equals_best"] += 1
            if not best < thr:
                if skipped:
                    C["later_walker_fails_ratio"] += 1
                continue
            if spos >= 0:
                if spos % 64 == bpos % 64:
                    C["best_second_same_lane"] += 1
                elif spos // 64 == bpos // 64:
                    C["best_second_same_chunk"] += 1
            if bpos % 64 == 63 or bpos == len(f2) - 1:
                C["best_at_chunk_end=%d" % (bpos // 64)] += 1
            if p1 == len(f1) - 1:
                C["walk_last_matched"] += 1
            if any(k == "taken" and dd < best for k, _, dd in skipped):
                C["later_walker_takes_next"] += 1
            m12[i1] = bi
            m21[bi] = i1
            taken[bi] = True
            nmatches += 1
            if check_ori:
                hist[rot_bin(angle1[i1], angle2[bi], M, ("ori", 0))].append(bi if not kfkf else i1)
    if check_ori:
        for x in _ori_filter(hist, M):
            C["rot_removed"] += 1
            nmatches -= 1
            if kfkf:
                m12[x] = -1
            else:
                m21[x] = -1
    return Result(match=m12 if kfkf else m21, nmatches=nmatches, margins=M, counters=C)


def search_by_bow(kf_desc, kf_angle, kf_valid, kf_fv, f_desc, f_angle, f_fv, nnratio=0.75,
                  check_ori=True, variant=None):
    """KeyFrame to Frame: bestDist1 <= TH_LOW (:282); match[iF] = the KeyFrame feature."""
    return _bow(kf_desc, kf_angle, kf_valid, kf_fv, f_desc, f_angle, None, f_fv, nnratio,
                check_ori, False, variant)


def search_by_bow_kf(desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2, nnratio=0.75,
                     check_ori=True, variant=None):
    """KeyFrame to KeyFrame: bestDist1 < TH_LOW (:712); match12[i1] = the KF2 feature."""
    return _bow(desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2, nnratio, check_ori,
                True, variant)


# ---------------------------------------------------------------- SearchForTriangulation
def epipolar_ok(kp1, kp2, F12, sigma2, M=None, who=None, C=None):
    """CheckDistEpipolarLine.  kp = (x, y, octave); F12 row-major 3x3."""
    x1, y1 = float(kp1[0]), float(kp1[1])
    x2, y2, o2 = float(kp2[0]), float(kp2[1]), int(kp2[2])
    F = np.asarray(F12, np.float32).astype(np.float64).reshape(3, 3)
    line, errs, mids = [], [], []
    for k in range(3):
        t = (x1 * F[0, k], y1 * F[1, k], F[2, k])
        v = t[0] + t[1] + t[2]
        line.append(v)
        errs.append(4 * U * max(abs(t[0]), abs(t[1]), abs(t[2]), abs(v)))
        mids += [t[0], t[1], t[0] + t[1], v]
    a, b, c = line
    t = (a * x2, b * y2)
    num = t[0] + t[1] + c
    e_num = abs(x2) * errs[0] + abs(y2) * errs[1] + errs[2] + 4 * U * max(abs(t[0]), abs(t[1]),
                                                                         abs(c), abs(num))
    den = a * a + b * b
    e_den = 2 * abs(a) * errs[0] + 2 * abs(b) * errs[1] + 3 * U * den
    exact = _is_f32(*mids, t[0], t[1], t[0] + t[1], num, a * a, b * b, den)
    if M is not None:
        M.add("epipolar_den", who, den, e_den, exact)
    if den == 0:
        if C is not None:
            C["tri_den_zero"] += 1
        return False
    dsqr = num * num / den
    lim = 3.84 * float(sigma2[o2])
    if M is not None:
        e = (2 * abs(num) * e_num + e_num * e_num) / den + dsqr * (e_den / den + 3 * U)
        M.add("epipolar", who, abs(dsqr - lim), e, exact and _is_f32(num * num, dsqr))
    ok = dsqr < lim
    if C is not None and o2 in (0, 7):
        C["tri_epipolar_%s_oct%d" % ("pass" if ok else "reject", o2)] += 1
    return ok


def epipole(geom, M=None):
    """ex, ey of ORBmatcher.cc:787-797 and their error bounds and exactness."""
    T = np.asarray(geom["Tcw2"], np.float32).astype(np.float64).reshape(3, 4)
    Cw = np.asarray(geom["Cw1"], np.float32).astype(np.float64).reshape(3)
    C2 = T[:, :3] @ Cw + T[:, 3]
    with np.errstate(all="ignore"):
        invz = np.float64(1.0) / C2[2]
        out = []
        for f, c, o in ((_f32(geom["fx2"]), C2[0], _f32(geom["cx2"])),
                        (_f32(geom["fy2"]), C2[1], _f32(geom["cy2"]))):
            p1 = f * c
            p2 = p1 * invz
            w = p2 + o
            out.append((float(w), 6 * U * max(abs(p2), abs(o), abs(w)),
                        _is_f32(*C2, float(invz), p1, p2, w)))
    return out


def search_for_triangulation(kf1, kf2, geom, scale, sigma2, only_stereo=False, check_ori=False,
                             variant=None):
    """kf = dict(kps, desc, uright or None (all < 0), has_mp or None (none), fv)."""
    M, C = Margins(), Counter()
    (ex, e_ex, x_ex), (ey, e_ey, x_ey) = epipole(geom, M)
    sf = np.asarray(scale, np.float32).astype(np.float64)
    s2 = np.asarray(sigma2, np.float32).astype(np.float64)

    def side(kf):
        n = len(kf["kps"])
        ur = kf.get("uright")
        ur = np.full(n, -1.0) if ur is None else np.asarray(ur, np.float32).astype(np.float64)
        mp = kf.get("has_mp")
        mp = np.zeros(n, bool) if mp is None else np.asarray(mp).astype(bool)
        k = kf["kps"]
        return (n, np.asarray(kf["desc"], np.uint8).reshape(-1, 32), ur, mp,
                np.asarray(k["x"], np.float64), np.asarray(k["y"], np.float64),
                np.asarray(k["octave"], np.int64), np.asarray(k["angle"], np.float64),
                _fv(kf["fv"]))
    n1, d1, ur1, mp1, x1, y1, o1, a1, (nodes1, off1, feats1) = side(kf1)
    n2, d2, ur2, mp2, x2, y2, o2, a2, (nodes2, off2, feats2) = side(kf2)
    match = np.full(n1, -1, np.int64)
    matched2 = np.zeros(n2, bool)
    chosen = Counter()
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for a, b in common_nodes(nodes1, nodes2, C):
        f1 = feats1[off1[a]:off1[a + 1]]
        f2 = feats2[off2[b]:off2[b + 1]]
        if _size_class(len(f2)):
            C["cand_node_size=%d" % len(f2)] += 1
        if len(f1) in (1, 64, 65, 129):
            C["walk_node_size=%d" % len(f1)] += 1
        for p1, i1 in enumerate(f1):
            who = ("f1", int(i1))
            if mp1[i1]:
                if p1 in (0, 63, 64):
                    C["walk_skip_pos=%d" % p1] += 1
                continue
            stereo1 = ur1[i1] >= 0
            if stereo1 and ur1[i1] == 0:
                C["tri_uright_zero_stereo"] += 1
            if only_stereo and not stereo1:
                C["tri_only_stereo_skip1"] += 1
                continue
            d = hamming(d1[i1], d2[f2]) if len(f2) else []
            best, bi, bpos = TH_LOW, -1, -1
            for p2, i2 in enumerate(f2):
                if mp2[i2] or matched2[i2]:
                    continue
                stereo2 = ur2[i2] >= 0
                if only_stereo and not stereo2:
                    C["tri_only_stereo_skip2"] += 1
                    continue
                dd = int(d[p2])
                if dd > TH_LOW or dd > best:
                    continue
                if variant == "tri_first_min" and bi >= 0 and dd == best:
                    continue
                if not stereo1 and not stereo2:
                    if variant != "no_epipole_test":
                        dx, dy = ex - x2[i2], ey - y2[i2]
                        q = dx * dx + dy * dy
                        lim = 100 * sf[o2[i2]]
                        e = (2 * abs(dx) * (e_ex + U * abs(dx)) + 2 * abs(dy) * (e_ey + U * abs(dy))
                             + 3 * U * q + U * lim)
                        M.add("epipole", who, abs(q - lim), e,
                              x_ex and x_ey and _is_f32(dx, dy, dx * dx, dy * dy, q, lim))
                        if o2[i2] in (0, 7):
                            C["tri_epipole_%s_oct%d" % ("reject" if q < lim else "pass",
                                                        o2[i2])] += 1
                        if q < lim:
                            continue
                elif stereo1 and not stereo2:
                    dx, dy = ex - x2[i2], ey - y2[i2]
                    if dx * dx + dy * dy < 100 * sf[o2[i2]]:
                        C["tri_epipole_skipped_stereo"] += 1
                if epipolar_ok((x1[i1], y1[i1], o1[i1]), (x2[i2], y2[i2], o2[i2]), geom["F12"], s2,
                               M, who, C):
                    if bi >= 0 and dd == best:
                        C["tri_tie_last_wins"] += 1
                        if bpos % 64 == 63 and p2 == bpos + 1:
                            C["tri_tie_across_chunks"] += 1
                    best, bi, bpos = dd, int(i2), p2
            if bi >= 0:
                match[i1] = bi
                nmatches += 1
                chosen[bi] += 1
                if bpos % 64 == 63 or bpos == len(f2) - 1:
                    C["best_at_chunk_end=%d" % (bpos // 64)] += 1
                if p1 == len(f1) - 1:
                    C["walk_last_matched"] += 1
                if variant == "tri_taken":
                    matched2[bi] = True
                if check_ori:
                    hist[rot_bin(a1[i1], a2[bi], M, ("ori", 0))].append(int(i1))
    C["tri_shared_kf2_by3"] = sum(1 for v in chosen.values() if v >= 3)
    if check_ori:
        for x in _ori_filter(hist, M):
            C["rot_removed"] += 1
            match[x] = -1
            nmatches -= 1
    return Result(match=match, nmatches=nmatches, margins=M, counters=C)


# ---------------------------------------------------------------- the KeyFrame's grid
class KeyFrameGrid:
    """mGrid as the Frame built it (float bounds, PosInGrid by round, increasing index inside a
    cell); GetFeaturesInArea's cell range and IsInImage on the KeyFrame's int bounds."""

    def __init__(self, kps, bounds, variant=None, margins=None, counters=None):
        self.variant, self.M = variant, margins
        self.C = Counter() if counters is None else counters
        self.x = np.asarray(kps["x"], np.float64)
        self.y = np.asarray(kps["y"], np.float64)
        self.octave = np.asarray(kps["octave"], np.int64)
        self.fb = tuple(_f32(v) for v in bounds)                 # min_x, max_x, min_y, max_y
        self.ib = tuple(float(int(v)) for v in self.fb)          # (int) truncates toward zero
        if variant == "kf_float_bounds":
            self.ib = self.fb
        self.inv_w = GRID_COLS / (self.fb[1] - self.fb[0])
        self.inv_h = GRID_ROWS / (self.fb[3] - self.fb[2])
        self.cells, self.cell_of = {}, []
        for i in range(len(self.x)):
            c = self.pos_in_grid(self.x[i], self.y[i], ("kp", i))
            self.cell_of.append(c)
            if c is not None:
                self.cells.setdefault(c, []).append(i)

    def pos_in_grid(self, x, y, who=None):
        px = (x - self.fb[0]) * self.inv_w
        py = (y - self.fb[2]) * self.inv_h
        if self.M is not None and who is not None:
            for p in (px, py):
                self.M.add("pos_in_grid", who, abs(abs(p - math.floor(p)) - 0.5),
                           4 * U * max(abs(p), 1.0), _is_f32(p, self.inv_w, self.inv_h))
        if self.variant == "grid_floor":
            ix, iy = math.floor(px), math.floor(py)
        else:
            ix, iy = _round(px), _round(py)
        for p, n in ((px, GRID_COLS), (py, GRID_ROWS)):
            self.C["kp_pos_hi_no_cell"] += p >= n - 0.5
            self.C["kp_pos_lo_no_cell"] += p <= -0.5
            self.C["kp_pos_last_cell"] += n - 1 < p < n - 0.5
        if ix < 0 or ix >= GRID_COLS or iy < 0 or iy >= GRID_ROWS:
            return None
        return ix, iy

    def is_in_image(self, u, v, who=None, eu=0.0, ev=0.0, exu=True, exv=True):
        b, f = self.ib, self.fb
        if self.M is not None and who is not None:
            self.M.add("in_image", who, abs(u - b[0]), eu, exu)
            self.M.add("in_image", who, abs(u - b[1]), eu, exu)
            self.M.add("in_image", who, abs(v - b[2]), ev, exv)
            self.M.add("in_image", who, abs(v - b[3]), ev, exv)
        ok = u >= b[0] and u < b[1] and v >= b[2] and v < b[3]
        if math.isfinite(u) and math.isfinite(v):
            self.C["in_image_left_of_grid"] += ok and (b[0] <= u < f[0] or b[2] <= v < f[2])
            self.C["out_by_int_max"] += (not ok) and (b[1] <= u < f[1] or b[3] <= v < f[3]) \
                and b[1] < f[1]
            self.C["u_eq_int_min"] += ok and (u == b[0] or v == b[2])
            self.C["u_eq_int_max"] += (not ok) and (u == b[1] or v == b[3])
        return ok

    def features_in_area(self, x, y, r, who=None, xy_err=0.0, r_err=0.0):
        M = self.M if who is not None else None
        qs = []
        for c, lo, inv in ((x, self.ib[0], self.inv_w), (y, self.ib[2], self.inv_h)):
            for sgn in (-1.0, 1.0):
                q = (c - lo + sgn * r) * inv
                qs.append(q)
                if M is not None:
                    mag = max(abs(c), abs(lo), abs(c - lo), r, abs(c - lo + sgn * r)) * inv
                    M.add("cell_range", ("range",) + who, abs(q - round(q)),
                          5 * U * mag + (xy_err + r_err) * inv)
        x0 = max(0, math.floor(qs[0]))
        if x0 >= GRID_COLS:
            return []
        x1 = min(GRID_COLS - 1, math.ceil(qs[1]))
        if x1 < 0:
            return []
        y0 = max(0, math.floor(qs[2]))
        if y0 >= GRID_ROWS:
            return []
        y1 = min(GRID_ROWS - 1, math.ceil(qs[3]))
        if y1 < 0:
            return []
        out = []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for i in self.cells.get((ix, iy), ()):
                    dx, dy = self.x[i] - x, self.y[i] - y
                    if M is not None:
                        for d in (dx, dy):
                            M.add("window", who, abs(abs(d) - r), xy_err + r_err + U * abs(d),
                                  xy_err == 0 and r_err == 0 and _is_f32(d))
                    if abs(dx) == r or abs(dy) == r:
                        self.C["window_edge"] += 1
                    if self.variant == "window_le":
                        inside = abs(dx) <= r and abs(dy) <= r
                    else:
                        inside = abs(dx) < r and abs(dy) < r
                    if inside:
                        out.append(i)
        if self.variant == "tie_by_index":
            out.sort()
        return out


def predict_scale(max_dist, dist, log_scale_factor, nlevels, M=None, who=None, e_dist=0.0,
                  exact_dist=True, C=None):
    """MapPoint::PredictScale(currentDist, pKF)."""
    ratio = float(max_dist) / dist
    L = math.log(ratio)
    v = L / float(log_scale_factor)
    n = math.ceil(v)
    k = round(v)
    if M is not None and 0 <= k <= nlevels - 2:
        e = (e_dist / dist + U + 3 * U * abs(L)) / float(log_scale_factor) + U * abs(v)
        M.add("predict_scale", who, abs(v - k), e, exact_dist and ratio == 1.0)
    if C is not None:
        C["lvl_exact0"] += ratio == 1.0
        C["lvl_clamp_lo"] += v < 0
        C["lvl_clamp_hi"] += n >= nlevels
    return 0 if n < 0 else (nlevels - 1 if n >= nlevels else n)


def _gemm(Mx, x, t, eM=0.0, ex=None, et=None):
    """M x + t as cv::gemm: (value, error bound, exact) per component."""
    Mx = np.asarray(Mx, np.float64).reshape(3, 3)
    x = np.asarray(x, np.float64)
    ex = np.zeros(3) if ex is None else ex
    et = np.zeros(3) if et is None else et
    terms = Mx * x[None, :]
    val = terms.sum(1) + t
    err = np.abs(Mx) @ ex + eM * np.abs(terms).sum(1) + et + U * np.abs(val)
    clean = eM == 0 and not ex.any() and not et.any()
    exact = np.array([clean and _is_f32(v) for v in val])
    err[exact] = 0.0      # a float32 number from exact inputs: float32 computes it too
    return val, err, exact


def _project(Pc, ePc, xPc, fx, fy, cx, cy, plain):
    """(u, v), their bounds and exactness, invz (ORBmatcher.cc:1005-1010)."""
    with np.errstate(all="ignore"):
        invz = np.float64(1.0) / Pc[2]
        out = []
        for f, c, ec, xc, o in ((fx, Pc[0], ePc[0], xPc[0], cx), (fy, Pc[1], ePc[1], xPc[1], cy)):
            x = c * invz
            p = f * x
            w = p + o
            e = 6 * U * max(abs(p), abs(o), abs(w))
            if not plain:
                e += f * (ec + abs(x) * ePc[2]) * abs(invz)
            exact = bool(xc and xPc[2]) and _is_f32(float(invz), float(x), float(p), float(w))
            out.append((float(w), 0.0 if exact else float(e), exact))
    return out, float(invz)


def _search_points(kf, grid, mps, mdesc, cams, th, sf, inv_sigma2, mode, skip, variant, M, C):
    """The per-MapPoint loop shared by Fuse, the Sim3 Fuse and one direction of SearchBySim3.
    cams = dict(chain=[(M, t, eM, et)], fx, fy, cx, cy, bf, Ow, eOw, lsf, nlevels)."""
    kps = kf["kps"]
    desc = np.asarray(kf["desc"], np.uint8).reshape(-1, 32)
    ur_kp = kf.get("uright")
    ur_kp = None if ur_kp is None else np.asarray(ur_kp, np.float32).astype(np.float64)
    if mode == "fuse" and ur_kp is None:
        C["no_uright_array"] += 1
    mdesc = np.asarray(mdesc, np.uint8).reshape(-1, 32)
    n = len(mps)
    best_idx = np.full(n, -1, np.int64)
    best_dist = np.full(n, NONE_DIST, np.int64)
    fx, fy, cx, cy, bf = (cams[k] for k in ("fx", "fy", "cx", "cy", "bf"))
    plain = len(cams["chain"]) == 1 and cams["chain"][0][2] == 0
    wide = variant == "level_window_wide"
    for i in range(n):
        who = ("q", i)
        if not (int(mps["flags"][i]) & MP_VALID):
            C["invalid_point"] += 1
            continue
        if skip is not None and skip[i]:
            C["already_matched_skip"] += 1
            continue
        P = np.array([mps["x"][i], mps["y"][i], mps["z"][i]], np.float64)
        val, err, xx = P, np.zeros(3), np.ones(3, bool)
        for Mx, t, eM, et in cams["chain"]:
            val, err, x2 = _gemm(Mx, val, t, eM, err, et)
            xx = xx & x2 if eM == 0 else np.zeros(3, bool)
        Pc, ePc = val, err
        M.add("z_sign", who, abs(Pc[2]), 0.0 if plain else ePc[2], bool(xx[2]))
        C["z_zero"] += Pc[2] == 0
        C["z_tiny"] += 0 < Pc[2] < 1e-6
        if Pc[2] < 0:
            C["z_neg"] += 1
            continue
        ((u, eu, exu), (v, ev, exv)), invz = _project(Pc, ePc, xx, fx, fy, cx, cy, plain)
        if not grid.is_in_image(u, v, who, eu, ev, exu, exv):
            continue
        # dist3D
        if mode == "sim3":
            dist = float(np.sqrt((Pc * Pc).sum()))
            e_dist = float(ePc.sum()) + U * dist
            x_dist = bool(xx.all()) and _is_f32(dist)
            e_dist = 0.0 if x_dist else e_dist
        else:
            PO = P - cams["Ow"]
            dist = float(np.sqrt((PO * PO).sum()))
            mag = max(np.abs(P).max(), np.abs(cams["Ow"]).max(), dist)
            e_dist = 5 * U * mag + cams["eOw"]
            x_dist = cams["xOw"] and _is_f32(*PO, dist)
            e_dist = 0.0 if x_dist else e_dist
        lo, hi = _f32(0.8) * float(mps["min_dist"][i]), _f32(1.2) * float(mps["max_dist"][i])
        M.add("dist_gate", who, abs(dist - lo), e_dist + (0.0 if _is_f32(lo) else U * lo),
              x_dist and _is_f32(lo))
        M.add("dist_gate", who, abs(dist - hi), e_dist + (0.0 if _is_f32(hi) else U * hi),
              x_dist and _is_f32(hi))
        C["dist_eq_min"] += dist == lo
        C["dist_eq_max"] += dist == hi
        if dist < lo or dist > hi:
            C["dist_lt_min" if dist < lo else "dist_gt_max"] += 1
            continue
        if mode != "sim3":
            Pn = np.array([mps["nx"][i], mps["ny"][i], mps["nz"][i]], np.float64)
            dot = float(PO @ Pn)
            e_po = 0.0 if x_dist else (2 * U * max(np.abs(P).max(), np.abs(cams["Ow"]).max())
                                       + cams["eOw"])
            M.add("view_cos", who, abs(dot - 0.5 * dist),
                  float(np.abs(Pn).sum()) * e_po + 0.5 * e_dist, x_dist)
            C["cos_eq_half"] += dot == 0.5 * dist
            if dot < 0.5 * dist:
                C["cos_lt_half"] += 1
                continue
        lvl = predict_scale(float(mps["max_dist"][i]), dist, cams["lsf"], cams["nlevels"], M, who,
                            e_dist, x_dist, C)
        C["lvl=%d" % lvl] += 1
        radius = _f32(th) * float(sf[lvl])
        r_err = 0.0 if _is_f32(radius) else U * radius
        cand = grid.features_in_area(u, v, radius, who, 0.0 if (exu and exv) else max(eu, ev),
                                     r_err)
        if not cand:
            continue
        d = hamming(mdesc[i], desc[cand])
        best, bi = NONE_DIST, -1
        seen = []
        for idx, dd in zip(cand, d):
            dd, o = int(dd), int(grid.octave[idx])
            if o < lvl - 1 or o > lvl + (1 if wide else 0):
                seen.append((dd, o - lvl))
                continue
            if mode == "fuse":
                stereo = ur_kp is not None and ur_kp[idx] >= 0
                e = [u - grid.x[idx], v - grid.y[idx]]
                es = [eu, ev]
                if stereo:
                    prod = bf * invz
                    ur = u - prod
                    e.append(ur - ur_kp[idx])
                    es.append(eu + 2 * U * max(abs(prod), abs(ur)))
                    C["uright_zero_stereo"] += ur_kp[idx] == 0
                e2 = sum(t * t for t in e)
                q = e2 * float(inv_sigma2[o])
                lim = 7.8 if stereo else 5.99
                eq = float(inv_sigma2[o]) * sum(2 * abs(t) * (s + U * abs(t))
                                                for t, s in zip(e, es))
                eq += (8 if stereo else 6) * U * q
                M.add("chi2", who, abs(q - lim), eq, exu and exv and _is_f32(*e, e2, q))
                C["chi2_%s_%s" % ("stereo" if stereo else "mono",
                                  "reject" if q > lim else "pass")] += 1
                if q > lim:
                    continue
            if dd < best:
                best, bi = dd, idx
            elif dd == best:
                cw, cl = grid.cell_of[bi], grid.cell_of[idx]
                kind = "ix" if cw[0] != cl[0] else ("iy" if cw[1] != cl[1] else "cell")
                C["tie_%s_%s_index_wins" % (kind, "higher" if bi > idx else "lower")] += 1
        for dd, rel in seen:
            if dd < best:
                C["level_reject_nearest_%s" % ("below" if rel < 0 else "above")] += 1
        best_dist[i] = best
        gate = TH_HIGH if (mode == "sim3" or variant == "fuse_th_high") else TH_LOW
        if best in (gate, gate + 1):
            C["%s_best=%d" % (mode, best)] += 1
        if best <= gate:
            best_idx[i] = bi
    return best_idx, best_dist


def _pose(T):
    T = np.asarray(T, np.float32).astype(np.float64).reshape(3, 4)
    return T[:, :3], T[:, 3]


def _fuse(kf, fcam, mps, mdesc, th, sf, inv_sigma2, sim3, variant):
    M, C = Margins(), Counter()
    fcam = np.asarray(fcam).reshape(-1)[0] if isinstance(fcam, np.ndarray) else fcam
    R, t = _pose(fcam["Tcw"])
    eM, x_pose = 0.0, True
    if sim3:
        scw = math.sqrt(float((R[0] * R[0]).sum()))
        alpha = 1.0 / scw
        x_pose = _is_f32(scw, alpha, *(R * alpha).reshape(-1), *(t * alpha))
        eM = 0.0 if x_pose else 3 * U
        M.add("sim3_scale", ("pose", 0), 1.0, eM, x_pose)
        R, t = R * alpha, t * alpha
    Ow = -(R.T @ t)
    eOw = (U + 2 * eM) * float(np.abs(Ow).max()) if len(Ow) else 0.0
    x_ow = _is_f32(*Ow) and x_pose
    cams = dict(chain=[(R, t, eM, eM * np.abs(t))], Ow=Ow, eOw=0.0 if x_ow else eOw, xOw=x_ow,
                lsf=_f32(fcam["log_scale_factor"]),
                nlevels=int(fcam["nlevels"]),
                **{k: _f32(fcam[k]) for k in ("fx", "fy", "cx", "cy", "bf")})
    grid = KeyFrameGrid(kf["kps"], [fcam[k] for k in ("min_x", "max_x", "min_y", "max_y")],
                        variant, M, C)
    bi, bd = _search_points(kf, grid, mps, mdesc, cams, th, sf, inv_sigma2,
                            "fuse_sim3" if sim3 else "fuse", None, variant, M, C)
    return Result(n=int((bi >= 0).sum()), best_idx=bi, best_dist=bd, margins=M, counters=C)


def fuse(kf, fcam, mps, mdesc, th, scale, inv_sigma2, variant=None):
    """Fuse(pKF, vpMapPoints, th)'s search: kf = dict(kps, desc, uright or None)."""
    return _fuse(kf, fcam, mps, mdesc, th, scale, inv_sigma2, False, variant)


def fuse_sim3(kf, fcam, mps, mdesc, th, scale, variant=None):
    """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)'s search: fcam["Tcw"] = Scw rows 0..2."""
    return _fuse(dict(kf, uright=None), fcam, mps, mdesc, th, scale, None, True, variant)


def search_by_sim3(kf1, mp1, md1, matched1, kf2, mp2, md2, matched2, g, th, scale, variant=None):
    M, C = Margins(), Counter()
    g = np.asarray(g).reshape(-1)[0] if isinstance(g, np.ndarray) else g
    R1, t1 = _pose(g["T1w"])
    R2, t2 = _pose(g["T2w"])
    R12 = np.asarray(g["R12"], np.float32).astype(np.float64).reshape(3, 3)
    t12 = np.asarray(g["t12"], np.float32).astype(np.float64)
    s12 = _f32(g["s12"])
    sR12, a = s12 * R12, 1.0 / s12
    sR21 = a * R12.T
    t21 = -(sR21 @ t12)
    x12 = _is_f32(*sR12.reshape(-1))
    x21 = _is_f32(a, *sR21.reshape(-1), *t21)
    e12, e21 = (0.0 if x12 else U), (0.0 if x21 else 2 * U)
    M.add("sim3_scale", ("pose", 0), 1.0, max(e12, e21), x12 and x21)
    et21 = np.zeros(3) if x21 else e21 * (np.abs(sR21) @ np.abs(t12)) + U * np.abs(t21)
    common = dict(Ow=None, eOw=0.0, xOw=True, lsf=_f32(g["log_scale_factor"]),
                  nlevels=int(g["nlevels"]), bf=0.0,
                  **{k: _f32(g[k]) for k in ("fx", "fy", "cx", "cy")})
    bounds = [g[k] for k in ("min_x", "max_x", "min_y", "max_y")]
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    C1, C2 = Counter(), Counter()
    z3 = np.zeros(3)
    vn1, _ = _search_points(kf2, KeyFrameGrid(kf2["kps"], bounds, variant, M, C1), mp1, md1,
                            dict(common, chain=[(R1, t1, 0.0, z3), (sR21, t21, e21, et21)]),
                            th, scale, None, "sim3", matched1, variant, M, C1)
    M2 = Margins()
    vn2, _ = _search_points(kf1, KeyFrameGrid(kf1["kps"], bounds, variant, M2, C2), mp2, md2,
                            dict(common, chain=[(R2, t2, 0.0, z3), (sR12, t12, e12, z3)]),
                            th, scale, None, "sim3", matched2, variant, M2, C2)
    # the second direction's decisions name KF2's points and KF1's keypoints
    ren = {"q": "q2", "kp": "kp1"}
    for kind, who, m, b in M2.amb:
        who = (("range", ren.get(who[1], who[1])) + who[2:]) if who[0] == "range" \
            else (ren.get(who[0], who[0]),) + who[1:]
        M.amb.append((kind, who, m, b))
    M.count += M2.count
    M.on_boundary.update(M2.on_boundary)
    C = C1 + C2
    C["sim3_dir1_matched_skip"] = C1["already_matched_skip"]
    C["sim3_dir2_matched_skip"] = C2["already_matched_skip"]
    match = np.full(n1, -1, np.int64)
    for i1 in range(n1):
        i2 = vn1[i1]
        if i2 >= 0:
            if vn2[i2] == i1:
                C["sim3_mutual"] += 1
            else:
                C["sim3_one_way_only"] += 1
            if vn2[i2] == i1 or variant == "sim3_one_way":
                match[i1] = i2
    return Result(match=match, nmatches=int((match >= 0).sum()), vn1=vn1, vn2=vn2, margins=M,
                  counters=C)
