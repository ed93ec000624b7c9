"""CPU: the oracle's ORB front end (oracle/orb_oracle.c: resize, GaussianBlur, FAST cells,
IC_Angle, rBRIEF) against tests/ref_frontend.py, a second statement of the same operations
written from their definitions in NumPy float64 / exact integers.

The GPU suite is bit-exact against the oracle; this module pins the oracle from the other
side, so a misreading shared by oracle and kernels (an NMS edge rule, a cell clip, a rounding,
a border reflection) no longer stays green.  Exact stages (blur, candidates) are compared
exactly; the others against bounds derived in ref_frontend (resize_bound, ANGLE_TOL_DEG,
AMBIGUOUS_CAP).  Every test prints the figure it measured before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_frontend as R  # noqa: E402

from orb_slam2_test_amd import synthetic as S  # noqa: E402

INI_TH, MIN_TH = 20, 7
SHAPES = [(97, 131, 2), (160, 200, 3)]  # h, w, levels
KINDS = ("frame", "noise", "lowc")
LEGACY_K = (18, 34, 49, 55, 49, 34, 18)  # sums to 257: the saturating path


def image(kind, h, w, seed):
    if kind == "frame":
        return S.frame(h, w, seed=seed)
    if kind == "noise":
        return S.pure_noise(h, w, seed=seed)
    if kind == "lowc":
        return R.low_contrast(S.frame(h, w, seed=seed))
    if kind == "blocks":
        return R.blocks_0_255(h, w, seed)
    if kind == "plateaus":
        return R.plateaus(h, w)
    if kind == "edges":
        return R.window_edge_dots(h, w)
    raise KeyError(kind)


_CACHE = {}


def extraction(oracle, kind, h, w, nlevels, seed, nfeatures=3000):
    """oracle.extract of one image with its pyramid, computed once and shared."""
    key = (kind, h, w, nlevels, seed, nfeatures)
    if key not in _CACHE:
        p = oracle.params(nfeatures=nfeatures, nlevels=nlevels, ini_th_fast=INI_TH,
                          min_th_fast=MIN_TH)
        r = oracle.extract(p, image(kind, h, w, seed), with_pyramid=True)
        r["params"] = p
        r["scale"] = np.array(p.scale[:nlevels], np.float32)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def oracle_candidates(oracle, p, lvl, l):
    """oracle.level_candidates as (x, y, response) in level coordinates."""
    k = oracle.level_candidates(p, lvl, l)
    b = R.EDGE_THRESHOLD - 3
    return np.stack([k["x"].astype(np.int64) + b, k["y"].astype(np.int64) + b,
                     k["response"].astype(np.int64)], 1).reshape(-1, 3)


def level_coords(kps, scale):
    """Keypoints (image coordinates) back to integer coordinates on their own level."""
    s = scale[kps["octave"]].astype(np.float64)
    return np.rint(kps["x"] / s).astype(np.int64), np.rint(kps["y"] / s).astype(np.int64)


ALL_IMAGES = [(k, h, w, L, 1 + i) for (h, w, L) in SHAPES for i, k in enumerate(KINDS)] + \
             [("blocks", 97, 131, 2, 5), ("plateaus", 97, 131, 2, 0), ("edges", 97, 131, 2, 0),
              ("blocks", 160, 200, 3, 6), ("plateaus", 160, 200, 3, 0), ("edges", 160, 200, 3, 0)]


# ------------------------------------------------------------------ candidates
@pytest.mark.parametrize("kind,h,w,nlevels,seed", ALL_IMAGES)
def test_candidates_equal_in_order(oracle, kind, h, w, nlevels, seed):
    r = extraction(oracle, kind, h, w, nlevels, seed)
    for l, lvl in enumerate(r["pyramid"]):
        got = oracle_candidates(oracle, r["params"], lvl, l)
        ref = R.level_candidates(lvl, INI_TH, MIN_TH)
        print("%s %dx%d level %d: %d candidates" % (kind, w, h, l, len(ref)))
        assert got.shape == ref.shape and np.array_equal(got, ref), (kind, l)
        assert len(ref) == r["cand_counts"][l]


def test_crafted_inputs_hold_their_cases(oracle):
    """The crafted images contain what they are for (conditions on the inputs)."""
    # score 254, the largest there is: 255 against nine contiguous zeros
    c = R.level_candidates(image("blocks", 97, 131, 5), INI_TH, MIN_TH)
    assert len(c) and c[:, 2].max() == 254
    # plateaus: corners with an equal-scoring neighbour exist, and no window emits one (taken
    # as one window here: in the cell grid a neighbour outside the window's scored area is 0)
    img = image("plateaus", 97, 131, 0)
    s = np.where(R.fast_score_map(img) >= INI_TH, R.fast_score_map(img), 0)
    tie = np.zeros(s.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                tie[1:-1, 1:-1] |= (s[1:-1, 1:-1] > 0) & (
                    s[1:-1, 1:-1] == s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx])
    assert tie.sum() > 100, tie.sum()
    c = R.fast_window(img, INI_TH)
    assert len(c) > 0 and not tie[c[:, 1], c[:, 0]].any()
    # window edges: every dot of every window is emitted by that window, on rows 3 / h-4 and
    # columns 3 / w-4 of it, and nothing else is
    img = image("edges", 97, 131, 0)
    want = []
    for x0, y0, x1, y1 in R.cell_windows(131, 97):
        want += [(x, y, 254) for y in (y0 + 3, y1 - 4) for x in (x0 + 3, x1 - 4)]
    assert len(want) == 4 * len(R.cell_windows(131, 97)) > 0
    assert R.level_candidates(img, INI_TH, MIN_TH).tolist() == [list(t) for t in want]
    # low contrast: most cells find nothing at the initial threshold and fall back
    lo = image("lowc", 97, 131, 3)
    c = R.level_candidates(lo, INI_TH, MIN_TH)
    assert (c[:, 2] < INI_TH).sum() >= 5 and c[:, 2].min() >= MIN_TH


_MODS = (0, 1, 15, 29)
SWEEP_W = [32 + 60 + m for m in _MODS] + [32 + 90 + m for m in _MODS]  # nCols 2 and 3
SWEEP_H = [32 + 60 + m for m in _MODS]


@pytest.mark.parametrize("lw", SWEEP_W)
def test_candidates_cell_grid_sweep(oracle, lw):
    """(lw - 32) mod 30 and (lh - 32) mod 30 in {0, 1, 15, 29}: cells of 30 and of 31 .. 45
    pixels, the clipped last cell, nCols 2 against 3.  The grid itself is checked against the
    closed form of the definition before the images are compared."""
    p = oracle.params(nfeatures=3000, nlevels=1, ini_th_fast=INI_TH, min_th_fast=MIN_TH)
    for lh in SWEEP_H:
        wins = R.cell_windows(lw, lh)
        ncols, nrows = (lw - 32) // 30, (lh - 32) // 30
        wcell = int(np.ceil((lw - 32) / ncols))
        assert len(wins) == ncols * nrows
        assert wins[0][:2] == (16, 16) and wins[-1][2:] == (lw - 16, lh - 16)
        assert wins[0][2] - wins[0][0] == min(wcell + 6, lw - 32)
        for kind in ("noise", "lowc"):
            img = image(kind, lh, lw, lw + lh)
            got = oracle_candidates(oracle, p, img, 0)
            ref = R.level_candidates(img, INI_TH, MIN_TH)
            assert got.shape == ref.shape and np.array_equal(got, ref), (kind, lw, lh)


# ------------------------------------------------------------------ blur
@pytest.mark.parametrize("k", [R.GAUSS_K, LEGACY_K])
def test_blur_exact(oracle, k):
    imgs = [image(kind, h, w, seed) for (kind, h, w, _, seed) in ALL_IMAGES]
    imgs += [image("noise", 8, 5, 1), image("noise", 7, 40, 2), np.full((9, 9), 255, np.uint8)]
    sat = 0
    for img in imgs:
        got = oracle.gauss7(img, k)
        ref = R.gauss7_exact(img, k)
        assert np.array_equal(got, ref), img.shape
        sat += int((ref == 255).sum())
    assert sat > 0  # 255-valued areas: 257 * 257 * 255 >> 16 saturates with the legacy table


# ------------------------------------------------------------------ resize
RESIZE_CASES = [(97, 131, 81, 109), (160, 200, 133, 167), (133, 167, 111, 139),
                (90, 257, 75, 214), (97, 131, 65, 87)]  # sh, sw, dh, dw (1.2 and 1.5)


@pytest.mark.parametrize("mode,simd", [(8, True), (4, True), (0, False)])
def test_resize_within_derived_bound(oracle, mode, simd):
    bound = R.resize_bound(simd)
    assert abs(bound - (1.2646 if simd else 0.7490)) < 1e-3
    worst = 0.0
    for sh, sw, dh, dw in RESIZE_CASES:
        for kind in ("frame", "noise", "blocks"):
            src = image(kind, sh, sw, sh + dw)
            err = np.abs(oracle.resize_linear(src, dw, dh, mode) - R.bilinear64(src, dw, dh))
            worst = max(worst, float(err.max()))
            assert err.max() <= bound, (mode, kind, sh, sw, np.argwhere(err > bound)[:3])
    print("resize mode %d: max |oracle - bilinear64| = %.4f (bound %.4f)" % (mode, worst, bound))


# ------------------------------------------------------------------ angle, descriptor
@pytest.mark.parametrize("kind,h,w,nlevels,seed", ALL_IMAGES[:6])
def test_angle_and_descriptor_bits(oracle, kind, h, w, nlevels, seed):
    r = extraction(oracle, kind, h, w, nlevels, seed)
    kps, desc = r["kps"], r["desc"]
    assert len(kps) > 10
    lx, ly = level_coords(kps, r["scale"])
    worst, nbits, namb = 0.0, 0, 0
    for l in range(nlevels):
        m = kps["octave"] == l
        if not m.any():
            continue
        lvl = r["pyramid"][l]
        d = R.circ_diff(kps["angle"][m], R.ic_angle64(lvl, lx[m], ly[m]))
        worst = max(worst, float(d.max()))
        assert d.max() < R.ANGLE_TOL_DEG, (l, d.max())
        bits, amb = R.brief_bits64(oracle.gauss7(lvl), lx[m], ly[m], kps["angle"][m])
        bad = (bits != R.unpack_bits(desc[m])) & ~amb
        assert not bad.any(), (l, np.argwhere(bad)[:5])
        nbits += bits.size
        namb += int(amb.sum())
    print("%s %dx%d: %d keypoints, max angle diff %.4f deg, ambiguous %d / %d bits (%.3f %%)"
          % (kind, w, h, len(kps), worst, namb, nbits, 100.0 * namb / nbits))
    assert namb <= R.AMBIGUOUS_CAP * nbits


# ------------------------------------------------------------------ full-survival inputs
FULL_SURVIVAL = [(k, 97, 131, 2, s) for k in KINDS for s in (1, 2, 3)]


@pytest.mark.parametrize("kind,h,w,nlevels,seed", FULL_SURVIVAL)
def test_full_survival_inputs(oracle, kind, h, w, nlevels, seed):
    """On these inputs (nfeatures 3000) the quadtree drops nothing: the extracted keypoints
    of a level, back in level coordinates, are exactly the level's candidates.  The GPU test
    relies on this list; an input belongs here only after passing this check."""
    r = extraction(oracle, kind, h, w, nlevels, seed)
    lx, ly = level_coords(r["kps"], r["scale"])
    assert len(r["kps"]) > 0
    for l in range(nlevels):
        m = r["kps"]["octave"] == l
        got = set(zip(lx[m].tolist(), ly[m].tolist(), r["kps"]["response"][m].astype(int).tolist()))
        ref = R.level_candidates(r["pyramid"][l], INI_TH, MIN_TH)
        assert m.sum() == len(ref)
        assert got == set(map(tuple, ref.tolist())), (kind, seed, l)
