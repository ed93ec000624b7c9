"""An independent NumPy statement of the per-frame matchers and of stereo matching.

The HIP kernels of match_kernels.hip, track_kernels.hip and stereo_kernels.hip are compared
bit for bit with oracle/match_oracle.c, track_oracle.c, stereo_oracle.c and orc_grid.h, C
written next to the kernels from one reading of the reference.  This module states the same
operations a second time from the reference's text (src/ORBmatcher.cc, src/Frame.cc), in
float64 and exact integers, without importing oracle/ or the package:

    hamming                           bit count of a XOR b, by np.unpackbits
    scale_factors                     mvScaleFactor of ORBextractor.cc:439-455 (float32 products)
    Grid.pos_in_grid                  Frame::PosInGrid, Frame.cc:510-520
    Grid.features_in_area             Frame::GetFeaturesInArea, Frame.cc:421-504, in its order
    three_maxima, rot_bin             ORBmatcher.cc:1800-1841 and the bin of :584-589
    search_for_initialization         ORBmatcher.cc:487-631
    search_by_projection_lastframe    ORBmatcher.cc:1503-1667
    search_by_projection_local        ORBmatcher.cc:59-154, RadiusByViewingCos :156-162
    stereo_matches                    Frame::ComputeStereoMatches, Frame.cc:619-834

tests/test_matching_ref.py holds the oracle to it on the CPU, tests/test_gpu_matching_ref.py
the kernels on the GPU.  Interface conventions shared with both (they are conventions of the
test interface, not rules of the reference): a search returns, per keypoint of the searched
frame, the index of the query written to its mvpMapPoints slot, -1 where nothing was written
and -2 where the rotation filter of the last-frame search set the slot to NULL; a map point
is a record with the fields the loop reads and two flag bits, 1 = the loop's guards pass
(pMP, !mvbOutlier / mbTrackInView, !isBad()), 2 = Observations() > 0.  min_z of stereo_matches
stands for Frame::mb, which the reference reads before assigning it (Frame.cc:661); min_z <= 0
means no upper disparity limit.

Float decisions.  The reference computes in float32, this module in float64 from the same
float32 inputs.  Every comparison whose outcome could differ is recorded in a Margins object
with its margin (the distance, in float64, of the compared value from the point where the
outcome changes) and a bound on |float32 value - float64 value|.  A decision is ambiguous when
margin < bound, unless margin == 0 and every intermediate float64 value on the path is a
float32 number: then float32 arithmetic computes the same values (a float64 result that is a
float32 number is within half a float64 ulp of the exact result, so float32 rounds the exact
result to it too) and the outcome is the same.  Scene builders drop what an ambiguous
decision names and the comparison with the oracle or the kernels is then exact.

Derived bounds.  U = 2^-24 is half a float32 ulp relative to the magnitude.  A bound is
(number of float32 roundings on the path) x U x (largest magnitude on the path, brought to the
unit of the compared value), plus the bound of any inexact input:
  pos_in_grid      (x - mnMinX) * inv with inv = 64 / (mnMaxX - mnMinX): 4 roundings
                   (difference of the bounds, quotient, difference, product) at |pos| <= 64:
                   4 U |pos| <= 1.6e-5 cells.  Margin: distance of pos to k + 1/2.
  cell range       (x - mnMinX -+ r) * inv: 5 roundings at max(|x|, |mnMinX|, r) * inv, plus
                   (err(x) + err(r)) * inv.  Margin: distance to the nearest integer.  A flip
                   cannot change the result: a keypoint at pos p > q lies in cell
                   round(p) >= floor(q), and p >= 63.5 or p < -0.5 is in no cell, so the cell
                   range always covers the window; it is reported all the same.
  window           |kp.x - x| < r: 1 rounding at |kp.x - x|, plus err(x) + err(r).  In
                   SearchForInitialization x and r are inputs (err 0); in the local-map
                   search r = {2.5, 4} * th * scale has 2 roundings; in the last-frame search
                   r = th * scale has 1 and x = u (below).
  projection u, v  x3Dc = Rcw x + tcw, 6 roundings per component at M3 = max(|x|, |tcw|,
                   |x3Dc|); invzc 1; fx * xc * invzc + cx 3 more: err(u) = 10 U max(fx |invzc| M3,
                   |fx xc invzc|, |cx|, |u|), about 4e-4 px for the scenes of the tests.
                   invzc < 0 can flip only through the sign of z: margin |z|, bound 6 U M3.
  bounds test      u < mnMinX, u > mnMaxX: margin |u - bound|, bound err(u).
  direction        tlc = Rlw (-Rcw^T tcw) + tlw against mb: 12 roundings at
                   max(|tcw|, |tlw|, |twc|, |tlc|, mb).
  uRight test      last frame: |u - bf * invzc - uRight| > radius: err(u) + 4 roundings (product,
                   two differences, radius) at max(|bf invzc|, |ur|, |uRight|, radius), and
                   |bf invzc| err(z) / |z|.  Local map: |ur - uRight| > r with ur an input:
                   1 rounding at |er| plus err(r).
  ratio            bestDist against nnratio * bestDist2: 1 rounding at the product.
  rotation bin     round((a1 - a2 [+ 360]) / 30): 4 roundings (difference, sum, 1.0f / 30,
                   product) at 12 bins.  0.1f * max1 against max2, max3: 1 rounding.
  stereo rows      ceil(y + r), floor(y - r) with r = 2 * scale (exact doubling): 1 rounding
                   at |y +- r|; margin: distance to the nearest integer.  Within the bound
                   the right keypoint is listed in one more row or not; a left keypoint of
                   that row is flagged if the two candidate lists have different winners.
  stereo columns   uR >= uL - maxD: 2 roundings (maxD = bf / minZ, difference) at
                   max(maxD, |uL - maxD|).  uR <= uL compares two inputs.
  round(x * inv)   1 rounding at |x inv| (the float64 product is exact); margin: distance to
                   k + 1/2.  For uR0 the other rounding is evaluated too and the keypoint
                   flagged if the outcome differs.
  |deltaR| <= 1    1 rounding (the quotient; the SADs are integers below 2^24) at 1.
  disparity        bestuR = scale * (uR0s + inc + deltaR), disparity = uL - bestuR: 4 roundings
                   at max(|uL|, |bestuR|): err(disparity) <= 4 U 320 = 7.7e-5 px at the test's
                   320 px width.  Margins |disparity| (>= 0 and <= 0) and |disparity - maxD|.
  median           SAD against 1.5f * 1.4f * median: the constant is one float32 product
                   (2.0999999046...), the threshold 1 rounding at its own magnitude.  With k
                   keypoints flagged before the cut the median is only known to lie between
                   elements n/2 - k and n/2 + k of the sorted list; every SAD that this
                   interval of thresholds leaves undecided is flagged.
  mvuRight         |float32 - float64| <= 3 U max(|bestuR|, |uR0s + inc + deltaR| scale)
                   (deltaR, sum, product), 1 U |uL| on the 0.01 branch.
  mvDepth          relative: err(disparity) / disparity + U (the quotient); 2 U on the 0.01
                   branch (0.01f, quotient).
Exact without a bound: Hamming distances, SADs (integers), the octave tests, (size_t)vL,
iniu < 0 || endu >= cols (integer-valued floats), bestincR == -+L, the taken flags.

Rules this module had wrong at first (the kind of rule it exists to pin):
  * No matching rule: the oracle equalled the first draft on every scene.  What the draft had
    wrong was how far an ambiguity reaches in stereo_matches.  It flagged every left keypoint
    of a row that some right keypoint may or may not be listed in, and every keypoint whose
    round(uR0 * inv) lies within float32 rounding of k + 1/2.  Both are common, not rare:
    y + 2 * scale is an integer for one level-1 keypoint in five ((yl + 2) * 1.2), and uR0
    comes from a neighbouring level, so uR0 * inv hits k + 1/2 exactly in real numbers
    (3 / 1.2 = 2.5) for 1.2-1.5 % of the left keypoints, above the 1 % cap.  Now both outcomes
    are evaluated and the keypoint is flagged only if they differ: the other candidate list
    must change the winner, the other rounding (which shifts the SAD range by one column) the
    result.  That leaves 0-0.7 % flagged on twelve seeds tried.
  * A premise of a test, not of the module: identical images do not take the 0.01 branch as
    a rule.  Disparity is exactly 0 only where deltaR is 0, that is SAD(-1) == SAD(+1), and
    the median of an identical pair is 0, so the cut clears every match anyway.  The branch is
    pinned by a designed scene with mirror-symmetric patches instead
    (test_stereo_zero_disparity_and_median_element).

Wrong-rule variants (variant=..., for the tests' sharpness check only): tie_by_index
(candidates in index order), window_le (|d| <= r), grid_floor (PosInGrid by floor),
no_level_rule (ratio test whatever the levels), second_is_next_distinct (a second best equal
to the best does not count), median_lo (element (n - 1) / 2), sad_last_min (last minimum).

Measured maxima (the bounds the tests assert are derived, not these):
  CPU, oracle against this module (tests/test_matching_ref.py)
    matchers: every scene equal in match and nmatches after the margin filter; the filter
        dropped at most 0.31 % of a scene (cap 2 %)
    stereo, two 320x240 pairs: 3 of 952 and 2 of 980 left keypoints flagged (0.32 %, cap
        1 %), matched sets equal on the rest, |mvuRight - ref| <= 2.3e-5 px (bound per
        keypoint, at most 5.7e-5), |mvDepth - ref| / ref <= 3.5e-6 (bound per keypoint)
  GPU (MI355X), kernels against this module (tests/test_gpu_matching_ref.py)
    matchers: every scene and the three-frame batch call equal in match and nmatches
    stereo, the same two pairs: the same 3 and 2 keypoints flagged, matched sets equal on the
        rest, |mvuRight - ref| <= 2.3e-5 px, |mvDepth - ref| / ref <= 3.5e-6, on the default
        path; ORBG_ST_FUSED=0 and ORBG_ST_LCAP=64 pass the same bounds (maxima unmeasured)
"""
import math

import numpy as np

GRID_COLS, GRID_ROWS = 64, 48
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
INT_MAX = 2 ** 31 - 1
U = 2.0 ** -24
MP_VALID, MP_HAS_OBS = 1, 2
VARIANTS = ("tie_by_index", "window_le", "grid_floor", "no_level_rule", "median_lo",
            "sad_last_min", "second_is_next_distinct")


def _f32(v):
    return float(np.float32(v))


def _is_f32(*vals):
    return all(math.isfinite(v) and float(np.float32(v)) == float(v) for v in vals)


def _round(v):
    """round(): half away from zero."""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def hamming(a, b):
    return np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8)),
                         axis=-1).sum(-1).astype(np.int64)


def scale_factors(scale_factor=1.2, nlevels=8):
    s = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * np.float32(scale_factor)
    return s


class Margins:
    """The float decisions of one call.  who = ("kp", i) a keypoint of the searched frame,
    ("q", i) a query, ("l", i) a left keypoint, ("call", 0) the call as a whole."""

    def __init__(self):
        self.count = 0
        self.amb = []
        self.smallest = {}   # kind -> smallest margin / bound among the unambiguous

    def add(self, kind, who, margin, bound, exact=False):
        self.count += 1
        if margin < bound and not (margin == 0 and exact):
            self.amb.append((kind, who, margin, bound))
        elif bound > 0 and margin > 0:
            self.smallest[kind] = min(self.smallest.get(kind, math.inf), margin / bound)

    def flag(self, kind, who):
        self.count += 1
        self.amb.append((kind, who, 0.0, 0.0))

    def ambiguous(self):
        return list(self.amb)

    def who(self, tag):
        return sorted({w[1] for _, w, _, _ in self.amb if w[0] == tag})


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------- the frame grid
class Grid:
    """mGrid of a Frame: cell (ix, iy) lists its keypoints in increasing index
    (AssignFeaturesToGrid, Frame.cc:292-307)."""

    def __init__(self, kps, bounds, variant=None, margins=None):
        self.variant = variant
        self.M = margins
        self.x = np.asarray(kps["x"], np.float64)
        self.y = np.asarray(kps["y"], np.float64)
        self.octave = np.asarray(kps["octave"], np.int64)
        self.min_x, self.max_x, self.min_y, self.max_y = (_f32(v) for v in bounds)
        self.inv_w = GRID_COLS / (self.max_x - self.min_x)
        self.inv_h = GRID_ROWS / (self.max_y - self.min_y)
        self.cells = {}
        self.cell_of = []
        for i in range(len(self.x)):
            c = self.pos_in_grid(self.x[i], self.y[i], ("kp", i))
            self.cell_of.append(c)
            if c is not None:
                self.cells.setdefault(c, []).append(i)

    def pos_in_grid(self, x, y, who=None):
        px = (x - self.min_x) * self.inv_w
        py = (y - self.min_y) * self.inv_h
        if self.M is not None and who is not None:
            for p in (px, py):
                self.M.add("pos_in_grid", who, abs(abs(p - math.floor(p)) - 0.5),
                           4 * U * max(abs(p), 1.0))
        if self.variant == "grid_floor":
            ix, iy = math.floor(px), math.floor(py)
        else:
            ix, iy = _round(px), _round(py)
        if ix < 0 or ix >= GRID_COLS or iy < 0 or iy >= GRID_ROWS:
            return None
        return ix, iy

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1, who=None, xy_err=0.0,
                         r_err=0.0):
        M = self.M if who is not None else None
        qs = []
        for c, lo, inv in ((x, self.min_x, self.inv_w), (y, self.min_y, self.inv_h)):
            for sgn in (-1.0, 1.0):
                q = (c - lo + sgn * r) * inv
                qs.append(q)
                if M is not None:
                    mag = max(abs(c), abs(lo), abs(c - lo), r, abs(c - lo + sgn * r)) * inv
                    M.add("cell_range", who, abs(q - round(q)),
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
        check_levels = (min_level > 0) or (max_level >= 0)
        idx = []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                c = self.cells.get((ix, iy))
                if c:
                    idx += c
        if not idx:
            return []
        idx = np.asarray(idx, np.int64)
        keep = np.ones(len(idx), bool)
        if check_levels:
            keep &= self.octave[idx] >= min_level
            if max_level >= 0:
                keep &= self.octave[idx] <= max_level
        dx, dy = self.x[idx] - x, self.y[idx] - y
        if self.variant == "window_le":
            inside = (np.abs(dx) <= r) & (np.abs(dy) <= r)
        else:
            inside = (np.abs(dx) < r) & (np.abs(dy) < r)
        if M is not None:
            for d in (dx, dy):
                m = np.abs(np.abs(d) - r)
                b = xy_err + r_err + U * np.abs(d)
                ex = (d.astype(np.float32).astype(np.float64) == d) & (xy_err == 0) & (r_err == 0)
                M.count += int(keep.sum())
                for k in np.nonzero(keep & (m < b) & ~((m == 0) & ex))[0]:
                    M.amb.append(("window", who, float(m[k]), float(b[k])))
        return idx[keep & inside].tolist()


def three_maxima(sizes, M=None):
    """ComputeThreeMaxima, ORBmatcher.cc:1800-1841."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    cut = _f32(0.1) * max1
    if M is not None:
        for m in (max2, max3):
            M.add("three_maxima", ("call", 0), abs(m - cut), U * cut, _is_f32(cut))
    if max2 < cut:
        ind2 = ind3 = -1
    elif max3 < cut:
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(a1, a2, M=None, who=None):
    """ORBmatcher.cc:584-589 / :1629-1634."""
    rot = float(a1) - float(a2)
    if rot < 0.0:
        rot += 360.0
    v = rot / HISTO_LENGTH
    if M is not None:
        M.add("rot_bin", who, abs(abs(v - math.floor(v)) - 0.5), 4 * U * 12.0)
    b = _round(v)
    return 0 if b == HISTO_LENGTH else b


def _best_two(cand, dist, variant, skip=None):
    """The strict-< update of the three loops.  Returns (best, second, index, position)."""
    if variant == "tie_by_index":
        o = np.argsort(np.asarray(cand), kind="stable")
        cand, dist = [cand[k] for k in o], dist[o]
    best = best2 = None
    bi = bk = -1
    for k, (i2, d) in enumerate(zip(cand, dist)):
        if skip is not None and skip(i2, d):
            continue
        d = int(d)
        if best is None or d < best:
            best2, best, bi, bk = best, d, i2, k
        elif (best2 is None or d < best2) and not (variant == "second_is_next_distinct"
                                                   and d == best):
            best2 = d
    return best, best2, bi, cand


# ---------------------------------------------------------------- SearchForInitialization
def search_for_initialization(kps1, desc1, kps2, desc2, prev_xy, bounds, window=100,
                              nnratio=0.9, check_ori=True, variant=None):
    M = Margins()
    g = Grid(kps2, bounds, variant, M)
    n1, n2 = len(kps1), len(kps2)
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    prev = np.array(prev_xy, np.float32).reshape(-1, 2)
    nn = _f32(nnratio)
    m12 = np.full(n1, -1, np.int64)
    m21 = np.full(n2, -1, np.int64)
    mdist = np.full(n2, INT_MAX, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i1 in range(n1):
        level1 = int(kps1["octave"][i1])
        if level1 > 0:
            continue
        cand = g.features_in_area(float(prev[i1, 0]), float(prev[i1, 1]), float(int(window)),
                                  level1, level1, who=("q", i1))
        if not cand:
            continue
        d = hamming(desc1[i1], desc2[cand])
        best, best2, bi, _ = _best_two(cand, d, variant, skip=lambda i2, dd: mdist[i2] <= dd)
        best = INT_MAX if best is None else best
        best2 = INT_MAX if best2 is None else best2
        if best <= TH_LOW:
            thr = float(best2) * nn      # (float)INT_MAX is 2^31; no match either way
            M.add("ratio", ("q", i1), abs(best - thr), U * thr, _is_f32(thr))
            if best < thr:
                if m21[bi] >= 0:
                    m12[m21[bi]] = -1
                    nmatches -= 1
                m12[i1], m21[bi], mdist[bi] = bi, i1, best
                nmatches += 1
                if check_ori:
                    hist[rot_bin(kps1["angle"][i1], kps2["angle"][bi], M, ("q", i1))].append(i1)
    if check_ori:
        keep = three_maxima([len(h) for h in hist], M)
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in hist[i]:
                if m12[idx1] >= 0:
                    m12[idx1] = -1
                    nmatches -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1] = (kps2["x"][m12[i1]], kps2["y"][m12[i1]])
    return Result(match=m12, nmatches=nmatches, prev=prev, margins=M)


# ---------------------------------------------------------------- SearchByProjection, last frame
def track_direction(cam, M=None):
    """bForward / bBackward, ORBmatcher.cc:1513-1524."""
    Tcw = np.asarray(cam["Tcw"], np.float32).astype(np.float64).reshape(3, 4)
    Tlw = np.asarray(cam["Tlw"], np.float32).astype(np.float64).reshape(3, 4)
    twc = -Tcw[:, :3].T @ Tcw[:, 3]
    tlc = Tlw[:, :3] @ twc + Tlw[:, 3]
    b = _f32(cam["b"])
    if M is not None and not cam["mono"]:
        mag = max(np.abs(Tcw[:, 3]).max(), np.abs(Tlw[:, 3]).max(), np.abs(twc).max(),
                  np.abs(tlc).max(), abs(b))
        ex = _is_f32(*twc, *tlc)
        M.add("direction", ("call", 0), abs(tlc[2] - b), 12 * U * mag, ex)
        M.add("direction", ("call", 0), abs(-tlc[2] - b), 12 * U * mag, ex)
    return (tlc[2] > b and not cam["mono"]), (-tlc[2] > b and not cam["mono"])


def search_by_projection_lastframe(kps, desc, uright, taken0, bounds, scale, pts, pdesc, cam,
                                   th, check_ori=True, variant=None):
    M = Margins()
    g = Grid(kps, bounds, variant, M)
    n, npts = len(kps), len(pts)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    pdesc = np.asarray(pdesc, np.uint8).reshape(-1, 32)
    sf = np.asarray(scale, np.float32).astype(np.float64)
    taken = np.zeros(n, bool) if taken0 is None else np.asarray(taken0).astype(bool).copy()
    ur_kp = None if uright is None else np.asarray(uright, np.float32).astype(np.float64)
    Tcw = np.asarray(cam["Tcw"], np.float32).astype(np.float64).reshape(3, 4)
    Rcw, tcw = Tcw[:, :3], Tcw[:, 3]
    fx, fy, cx, cy, bf = (_f32(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    th = _f32(th)
    fwd, bwd = track_direction(cam, M)
    match = np.full(n, -1, np.int64)
    pushes = []
    nmatches = 0
    for i in range(npts):
        who = ("q", i)
        if not (int(pts["flags"][i]) & MP_VALID):
            continue
        xw = np.array([pts["x"][i], pts["y"][i], pts["z"][i]], np.float64)
        terms = Rcw * xw[None, :]
        xc3 = terms.sum(1) + tcw
        exact = _is_f32(*terms.reshape(-1), *(terms[:, 0] + terms[:, 1]), *terms.sum(1), *xc3)
        m3 = max(np.abs(xw).max(), np.abs(tcw).max(), np.abs(xc3).max())
        xc, yc, zc = xc3
        M.add("invzc_sign", who, abs(zc), 6 * U * m3, exact)
        if zc == 0:
            continue
        invzc = 1.0 / zc
        if invzc < 0:
            continue
        uv, errs, exs = [], [], []
        for f, c, o in ((fx, xc, cx), (fy, yc, cy)):
            p1 = f * c
            p2 = p1 * invzc
            w = p2 + o
            uv.append(w)
            errs.append(10 * U * max(f * abs(invzc) * m3, abs(p2), abs(o), abs(w)))
            exs.append(exact and _is_f32(invzc, p1, p2, w))
        (u, v), (eu, ev), (exu, exv) = uv, errs, exs
        M.add("bounds", who, abs(u - g.min_x), eu, exu)
        M.add("bounds", who, abs(u - g.max_x), eu, exu)
        if u < g.min_x or u > g.max_x:
            continue
        M.add("bounds", who, abs(v - g.min_y), ev, exv)
        M.add("bounds", who, abs(v - g.max_y), ev, exv)
        if v < g.min_y or v > g.max_y:
            continue
        octv = int(pts["octave"][i])
        radius = th * sf[octv]
        r_err = 0.0 if _is_f32(radius) else U * radius
        xy_err = 0.0 if (exu and exv) else max(eu, ev)
        if fwd:
            lv = (octv, -1)
        elif bwd:
            lv = (0, octv)
        else:
            lv = (octv - 1, octv + 1)
        cand = g.features_in_area(u, v, radius, lv[0], lv[1], who=who, xy_err=xy_err,
                                  r_err=r_err)
        if not cand:
            continue
        if variant == "tie_by_index":
            cand = sorted(cand)
        dist = hamming(pdesc[i], desc[cand])
        best, bi = 256, -1
        for i2, d in zip(cand, dist):
            if taken[i2]:
                continue
            if ur_kp is not None and ur_kp[i2] > 0:
                prod = bf * invzc
                ur = u - prod
                er = abs(ur - ur_kp[i2])
                mag = max(abs(prod), abs(ur), abs(ur_kp[i2]), radius)
                ex = exu and r_err == 0 and _is_f32(prod, ur, er)
                M.add("uright", who, abs(er - radius),
                      (0.0 if exu else eu) + 4 * U * mag + abs(prod) * 6 * U * m3 / abs(zc), ex)
                if er > radius:
                    continue
            if d < best:
                best, bi = int(d), i2
        if best <= TH_HIGH:
            match[bi] = i
            taken[bi] = bool(int(pts["flags"][i]) & MP_HAS_OBS)
            nmatches += 1
            if check_ori:
                pushes.append((rot_bin(pts["angle"][i], kps["angle"][bi], M, who), bi))
    if check_ori:
        sizes = [0] * HISTO_LENGTH
        for b, _ in pushes:
            sizes[b] += 1
        keep = three_maxima(sizes, M)
        for b, i2 in pushes:
            if b not in keep:
                match[i2] = -2
                nmatches -= 1
    return Result(match=match, nmatches=nmatches, margins=M, forward=fwd, backward=bwd)


# ---------------------------------------------------------------- SearchByProjection, local map
def search_by_projection_local(kps, desc, uright, taken0, bounds, scale, mps, mdesc, th=1.0,
                               nnratio=0.8, variant=None):
    M = Margins()
    g = Grid(kps, bounds, variant, M)
    n = len(kps)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    mdesc = np.asarray(mdesc, np.uint8).reshape(-1, 32)
    sf = np.asarray(scale, np.float32).astype(np.float64)
    taken = np.zeros(n, bool) if taken0 is None else np.asarray(taken0).astype(bool).copy()
    ur_kp = None if uright is None else np.asarray(uright, np.float32).astype(np.float64)
    th, nn = _f32(th), _f32(nnratio)
    b_factor = th != 1.0
    match = np.full(n, -1, np.int64)
    nmatches = 0
    for i in range(len(mps)):
        who = ("q", i)
        if not (int(mps["flags"][i]) & MP_VALID):
            continue
        level = int(mps["level"][i])
        r = 2.5 if float(mps["view_cos"][i]) > 0.998 else 4.0   # float against a double constant
        if b_factor:
            r *= th
        rs = r * sf[level]
        r_err = 0.0 if _is_f32(r, rs) else 2 * U * rs
        u, v = float(mps["u"][i]), float(mps["v"][i])
        cand = g.features_in_area(u, v, rs, level - 1, level, who=who, r_err=r_err)
        if not cand:
            continue
        d = hamming(mdesc[i], desc[cand])

        def skip(idx, dd):
            if taken[idx]:
                return True
            if ur_kp is not None and ur_kp[idx] > 0:
                er = abs(float(mps["ur"][i]) - ur_kp[idx])
                M.add("uright", who, abs(er - rs), r_err + U * er, r_err == 0 and _is_f32(er))
                if er > rs:
                    return True
            return False

        # bestLevel / bestLevel2 follow bestDist / bestDist2 (ORBmatcher.cc:125-137)
        if variant == "tie_by_index":
            o = np.argsort(np.asarray(cand), kind="stable")
            cand, d = [cand[k] for k in o], d[o]
        best, best2, lev, lev2, bi = 256, 256, -1, -1, -1
        for idx, dd in zip(cand, d):
            if skip(idx, dd):
                continue
            dd = int(dd)
            if dd < best:
                best2, lev2 = best, lev
                best, lev, bi = dd, int(g.octave[idx]), idx
            elif dd < best2 and not (variant == "second_is_next_distinct" and dd == best):
                lev2, best2 = int(g.octave[idx]), dd
        if best <= TH_HIGH:
            thr = nn * best2
            same = lev == lev2 or variant == "no_level_rule"
            if lev == lev2:
                M.add("ratio", who, abs(best - thr), U * thr, _is_f32(thr))
            if same and best > thr:
                continue
            match[bi] = i
            taken[bi] = bool(int(mps["flags"][i]) & MP_HAS_OBS)
            nmatches += 1
    return Result(match=match, nmatches=nmatches, margins=M)


# ---------------------------------------------------------------- ComputeStereoMatches
MEDIAN_FACTOR = float(np.float32(1.5) * np.float32(1.4))


def stereo_matches(kps_l, desc_l, kps_r, desc_r, pyr_l, pyr_r, scale, bf, min_z, variant=None):
    """Returns Result(uright, depth: float64, -1 where unmatched; uright_bound, depth_bound:
    the derived |float32 - float64| bounds per keypoint; sad; pre: the (iL, uright, depth, sad)
    list before the median cut; flagged: left keypoints with an ambiguous decision; margins)."""
    M = Margins()
    nl, nr = len(kps_l), len(kps_r)
    desc_l = np.asarray(desc_l, np.uint8).reshape(-1, 32)
    desc_r = np.asarray(desc_r, np.uint8).reshape(-1, 32)
    sf32 = np.asarray(scale, np.float32)
    sf = sf32.astype(np.float64)
    inv = (np.float32(1.0) / sf32).astype(np.float64)
    n_rows = pyr_l[0].shape[0]
    xl, yl = np.asarray(kps_l["x"], np.float64), np.asarray(kps_l["y"], np.float64)
    xr, yr = np.asarray(kps_r["x"], np.float64), np.asarray(kps_r["y"], np.float64)
    ol, orr = np.asarray(kps_l["octave"], np.int64), np.asarray(kps_r["octave"], np.int64)
    uright = np.full(nl, -1.0)
    depth = np.full(nl, -1.0)
    ub = np.zeros(nl)
    db = np.zeros(nl)
    sad_of = np.full(nl, -1, np.int64)

    # row table (:638-658); rows outside the image cannot occur for extractor keypoints
    rows = [[] for _ in range(n_rows)]
    contested = {}      # row -> right keypoints that float32 may list there or not
    for iR in range(nr):
        r = 2.0 * sf[orr[iR]]
        hi, lo = yr[iR] + r, yr[iR] - r
        for v, row in ((hi, round(hi) + 1), (lo, round(lo) - 1)):
            m = abs(v - round(v))
            M.count += 1
            if m < U * abs(v) and not (m == 0 and _is_f32(v)):
                contested.setdefault(row, set()).add(iR)
        for yi in range(max(math.floor(lo), 0), min(math.ceil(hi), n_rows - 1) + 1):
            rows[yi].append(iR)

    bf, min_z = _f32(bf), _f32(min_z)
    max_d = bf / min_z if min_z > 0 else math.inf
    th_orb = (TH_HIGH + TH_LOW) // 2
    W = L = 5
    pre = []
    for iL in range(nl):
        who = ("l", iL)
        lvl, uL, vL = int(ol[iL]), xl[iL], yl[iL]
        row = int(vL)
        if row < 0 or row >= n_rows:
            continue
        min_u, max_u = uL - max_d, uL

        def winner(cands, report):
            """(best right keypoint, distance) over a candidate list in iR order."""
            c = np.asarray(cands, np.int64)
            c = c[(orr[c] >= lvl - 1) & (orr[c] <= lvl + 1)]
            if report and math.isfinite(max_d) and len(c):
                m = np.abs(xr[c] - min_u)
                b = 2 * U * max(max_d, abs(min_u))
                if np.any((m < b) & ~((m == 0) & _is_f32(max_d, min_u))):
                    M.flag("column_range", who)
            c = c[(xr[c] >= min_u) & (xr[c] <= max_u)]
            if not len(c):
                return None
            d = hamming(desc_l[iL], desc_r[c])
            k = int(np.argmin(d))        # first strictly smaller, starting from TH_HIGH
            return (int(c[k]), int(d[k])) if d[k] < TH_HIGH else None

        if row in contested:
            # float32 may list these in the row or not: ambiguous if that changes the winner
            a = winner(sorted(set(rows[row]) | contested[row]), False) if max_u >= 0 else None
            b = winner([i for i in rows[row] if i not in contested[row]], False) \
                if max_u >= 0 and len(rows[row]) else None
            if a != b:
                M.flag("row_table", who)
        cands = rows[row]
        if not cands:
            continue
        if max_u < 0:
            continue
        win = winner(cands, True)
        if win is None or win[1] >= th_orb:
            continue
        uR0 = xr[win[0]]
        s = inv[lvl]
        scaled, other = [], None
        for k, p in enumerate((uL * s, vL * s, uR0 * s)):
            m = abs(abs(p - math.floor(p)) - 0.5)
            if k == 2 and 0 < m < U * abs(p):
                # uR0 comes from another level, so uR0 * s can sit on k + 1/2 (3 / 1.2): the
                # other rounding shifts the SAD range by one column, which is ambiguous only
                # if that changes the outcome (below)
                M.count += 1
                other = math.floor(p) + (math.floor(p) == _round(p))
            else:
                M.add("round_scaled", who, m, U * abs(p), m == 0)
            scaled.append(_round(p))
        su, sv, su0 = scaled
        imL, imR = pyr_l[lvl], pyr_r[lvl]
        cols = imR.shape[1]
        IL = imL[sv - W:sv + W + 1, su - W:su + W + 1].astype(np.int64)
        assert sv - W >= 0 and su - W >= 0 and IL.shape == (11, 11), "patch leaves the image"
        IL = IL - IL[W, W]

        def refine(su0, MM):
            """SAD search, parabola and disparity tests from scaleduR0 on:
            (mvuRight, mvDepth, SAD, their two bounds) or None."""
            if su0 + L - W < 0 or su0 + L + W + 1 >= cols:
                return None
            sads = []
            for inc in range(-L, L + 1):
                IR = imR[sv - W:sv + W + 1, su0 + inc - W:su0 + inc + W + 1].astype(np.int64)
                assert IR.shape == (11, 11), "right patch leaves the image"
                sads.append(int(np.abs(IL - (IR - IR[W, W])).sum()))
            best = min(sads)
            if variant == "sad_last_min":
                best_inc = max(k2 for k2 in range(11) if sads[k2] == best) - L
            else:
                best_inc = sads.index(best) - L
            if best_inc == -L or best_inc == L:
                return None
            d1, d2, d3 = (float(sads[L + best_inc + t]) for t in (-1, 0, 1))
            den = 2.0 * (d1 + d3 - 2.0 * d2)
            if den == 0:
                return None     # +-inf fails |deltaR| <= 1; NaN fails disparity >= minD
            delta = (d1 - d3) / den
            MM.add("delta_range", who, abs(abs(delta) - 1.0), U, _is_f32(delta))
            if delta < -1 or delta > 1:
                return None
            t = su0 + best_inc + delta
            best_ur = sf[lvl] * t
            disparity = uL - best_ur
            ex = _is_f32(delta, t, best_ur, disparity)
            e_d = 4 * U * max(abs(uL), abs(best_ur))
            MM.add("disparity_min", who, abs(disparity), e_d, ex)
            if math.isfinite(max_d):
                MM.add("disparity_max", who, abs(disparity - max_d), e_d + U * max_d,
                       ex and _is_f32(max_d))
            if not (disparity >= 0 and disparity < max_d):
                return None
            if disparity <= 0:
                return (uL - 0.01, bf / _f32(0.01), best, U * abs(uL), 2 * U)
            return (best_ur, bf / disparity, best, 3 * U * max(abs(best_ur), abs(t) * sf[lvl]),
                    e_d / disparity + U)

        out = refine(su0, M)
        if other is not None and refine(other, Margins()) != out:
            M.flag("round_scaled", who)
        if out is not None:
            pre.append((iL, out[0], out[1], out[2]))
            sad_of[iL], ub[iL], db[iL] = out[2], out[3], out[4]

    # median cut (:820-833)
    if pre:
        order = sorted(pre, key=lambda e: (e[3], e[0]))
        S = [e[3] for e in order]
        nv = len(S)
        mid = (nv - 1) // 2 if variant == "median_lo" else nv // 2
        doubt = len(M.who("l"))
        lo, hi = S[max(0, mid - doubt)], S[min(nv - 1, mid + doubt)]
        thr = MEDIAN_FACTOR * float(S[mid])
        for iL, u_r, z, sad in order:
            if lo == hi:
                M.add("median_cut", ("l", iL), abs(sad - thr), U * thr, _is_f32(thr))
            elif MEDIAN_FACTOR * lo * (1 - U) <= sad < MEDIAN_FACTOR * hi * (1 + U):
                M.flag("median_cut", ("l", iL))
            if sad < thr:
                uright[iL], depth[iL] = u_r, z
    return Result(uright=uright, depth=depth, uright_bound=ub, depth_bound=db, sad=sad_of,
                  pre=pre, flagged=set(M.who("l")), margins=M)
