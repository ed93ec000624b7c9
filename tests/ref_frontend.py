"""An independent NumPy statement of the ORB front end, stage by stage.

Every other extractor test compares the HIP kernels with oracle/orb_oracle.c, a C restatement
written next to the kernels.  This module states the same operations a second time, from
their definitions, in float64 or exact integers, without importing oracle/ or the package:

    bilinear64        real-valued bilinear resampling, half-pixel centres, clamped edges
    gauss7_exact      separable 7-tap integer convolution, REFLECT_101, round half up
    fast_score_map    FAST-9/16 score = largest threshold at which the pixel is a corner
    fast_window       cv::FAST(window, th, nonmax=true): corners that beat their 8 neighbours
    level_candidates  the 30-pixel cell grid of ComputeKeyPointsOctTree with its fallback
    ic_angle64        intensity-centroid angle over the umax disc
    brief_bits64      the 256 rotated-pattern comparisons, with the bits float32 may flip

tests/test_ref_frontend.py holds the oracle to it on the CPU, tests/test_gpu_frontend_ref.py
the kernels on the GPU.  Its only constants are bit_pattern_31 and umax of
tests/golden/ref_tables.json.

Rules this module had wrong at first (the kind of rule it exists to pin):
  * NMS row range.  A first draft emitted corners only on rows 4 .. h-5 of a window, as if a
    corner needed three scored rows.  cv::FAST scores rows 3 .. h-4 and compares against a
    zero-filled buffer, so rows 3 and h-4 (and columns 3 and w-4) do emit corners; an
    unscored neighbour counts as 0.  The draft lost 5-13 % of the candidates.

Measured maxima (the bounds the tests assert are derived, not these):
  CPU, oracle against this module (tests/test_ref_frontend.py)
    resize |oracle - bilinear64|, grey levels: 16+8 SIMD 0.7839, 16+4 SIMD 0.7839,
        scalar 0.5623 (bounds 1.2646 and 0.7490)
    angle |oracle - ic_angle64|: 0.0092 deg (bound 0.02)
    descriptor: 0 mismatching unambiguous bits; ambiguous share at most 0.112 % (cap 0.5 %)
  GPU (MI355X), kernels against this module (tests/test_gpu_frontend_ref.py)
    resize |level l - bilinear64(level l-1)|: k_pyramid 0.7672, k_resize chain 0.7672,
        scale factor 1.5 0.7932, 16+4 mode 0.7672 (bound 1.2646); scalar mode 0.5489 on
        both kernels (bound 0.7490)
    angle |k_orient_desc - ic_angle64|: 0.0096 deg (bound 0.02)
    descriptor: 0 mismatching unambiguous bits; ambiguous share at most 0.119 % (cap 0.5 %)
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(_HERE, "golden", "ref_tables.json")) as _f:
    _T = json.load(_f)
PATTERN = np.asarray(_T["bit_pattern_31"], np.int64).reshape(256, 2, 2)  # [bit][point][x, y]
UMAX = np.asarray(_T["umax"], np.int64)
HALF_PATCH = 15
EDGE_THRESHOLD = 19
CELL = 30
GAUSS_K = (18, 34, 48, 56, 48, 34, 18)


# ---------------------------------------------------------------- a. resize
def _axis(d, s):
    c = (np.arange(d, dtype=np.float64) + 0.5) * (s / d) - 0.5
    c = np.clip(c, 0.0, s - 1.0)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, s - 1), c - i0


def bilinear64(src, dw, dh):
    """src resampled to dh x dw: the bilinear interpolant of the pixel centres evaluated at
    (d + 0.5) * (s / dsize) - 0.5, coordinates clamped to the image.  float64, unrounded."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape
    x0, x1, fx = _axis(dw, sw)
    y0, y1, fy = _axis(dh, sh)
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


# ---------------------------------------------------------------- b. blur
def gauss7_exact(src, k=GAUSS_K):
    """7x7 separable convolution with integer weights k (8.8 fixed point, so the product of
    two passes carries 16 fraction bits), borders mirrored without repeating the edge pixel,
    result floor(acc / 65536 + 0.5) saturated to u8."""
    k = np.asarray(k, np.int64)
    a = np.pad(np.asarray(src, np.int64), 3, mode="reflect")
    h, w = a.shape
    hor = sum(k[t] * a[:, t:w - 6 + t] for t in range(7))
    acc = sum(k[t] * hor[t:h - 6 + t, :] for t in range(7))
    return np.clip((2 * acc + 65536) // 131072, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- c. FAST
def _ring():
    """The 16 pixels of the radius-3 Bresenham circle, in order around it."""
    q = [(0, 3), (1, 3), (2, 2), (3, 1)]  # one quadrant; the rest by quarter turns
    pts = []
    for _ in range(4):
        pts += q
        q = [(y, -x) for x, y in q]
    return pts


RING = _ring()


def fast_score_map(img):
    """score(p) = the largest t >= 0 such that 9 contiguous ring pixels are all > v + t or
    all < v - t, i.e. max over the 16 arcs and both signs of min(d) - 1; -1 when there is no
    such t.  Defined on rows and columns 3 .. n-4; -1 elsewhere."""
    img = np.asarray(img, np.int64)
    h, w = img.shape
    out = np.full((h, w), -1, np.int64)
    if h < 7 or w < 7:
        return out
    v = img[3:h - 3, 3:w - 3]
    d = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in RING])
    best = np.full(v.shape, -1, np.int64)
    for sign in (1, -1):
        dd = np.concatenate([sign * d, sign * d[:8]])
        for s in range(16):
            best = np.maximum(best, dd[s:s + 9].min(axis=0) - 1)
    out[3:h - 3, 3:w - 3] = best
    return out


def fast_window(img, th):
    """Corners of one window at threshold th after non-maximum suppression: score >= th and
    score strictly greater than each of the 8 neighbours, where a neighbour that is unscored
    or no corner at th counts as 0.  Returns an (n, 3) int64 array of (x, y, score) in
    row-major order."""
    s = fast_score_map(img)
    h, w = s.shape
    z = np.zeros((h + 2, w + 2), np.int64)
    z[1:-1, 1:-1] = np.where(s >= th, s, 0)
    c = z[1:-1, 1:-1]
    keep = s >= th
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                keep &= c > z[dy:dy + h, dx:dx + w]
    y, x = np.nonzero(keep)
    return np.stack([x, y, s[y, x]], 1).astype(np.int64).reshape(-1, 3)


# ---------------------------------------------------------------- d. cell grid
def cell_windows(lw, lh):
    """The FAST windows of a level of lw x lh pixels, in the order the cells are visited:
    (x0, y0, x1, y1) half-open in level coordinates.  The detection area leaves a border of
    EDGE_THRESHOLD - 3 on every side; it is cut into int(width / 30) columns of
    ceil(width / nCols) pixels (rows alike); each window is a cell plus 6, clipped to the far
    border; a row that starts within 3 of the far border, or a column within 6, is dropped."""
    b = EDGE_THRESHOLD - 3
    max_x, max_y = lw - b, lh - b
    width, height = max_x - b, max_y - b
    ncols, nrows = width // CELL, height // CELL
    if ncols <= 0 or nrows <= 0:
        raise ValueError("level %dx%d has no 30-pixel cell" % (lw, lh))
    wcell, hcell = -(-width // ncols), -(-height // nrows)
    out = []
    for i in range(nrows):
        y0 = b + i * hcell
        if y0 >= max_y - 3:
            continue
        for j in range(ncols):
            x0 = b + j * wcell
            if x0 >= max_x - 6:
                continue
            out.append((x0, y0, min(x0 + wcell + 6, max_x), min(y0 + hcell + 6, max_y)))
    return out


def level_candidates(level, ini_th, min_th):
    """Every FAST candidate of one pyramid level: per cell window, the corners at ini_th, or,
    only when there is none, the corners at min_th.  Returns an (n, 3) int64 array of
    (x, y, response) in LEVEL coordinates (the reference keeps them relative to the
    EDGE_THRESHOLD - 3 border until after the quadtree), cells in visiting order, row-major
    inside a cell."""
    level = np.asarray(level)
    lh, lw = level.shape
    out = []
    for x0, y0, x1, y1 in cell_windows(lw, lh):
        win = level[y0:y1, x0:x1]
        k = fast_window(win, ini_th)
        if len(k) == 0:
            k = fast_window(win, min_th)
        out.append(k + np.array([x0, y0, 0]))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


# ---------------------------------------------------------------- e. orientation, rBRIEF
def _disc():
    v = np.arange(-HALF_PATCH, HALF_PATCH + 1)
    vv, uu = np.meshgrid(v, v, indexing="ij")
    m = np.abs(uu) <= UMAX[np.abs(vv)]
    return uu[m], vv[m]


_DISC_U, _DISC_V = _disc()


def ic_angle64(level, x, y):
    """Direction of the intensity centroid of the disc |v| <= 15, |u| <= umax[|v|] around
    each integer (x, y): degrees(atan2(m01, m10)) mod 360 with exact integer moments."""
    level = np.asarray(level, np.int64)
    x = np.atleast_1d(np.asarray(x, np.int64))
    y = np.atleast_1d(np.asarray(y, np.int64))
    patch = level[y[:, None] + _DISC_V[None, :], x[:, None] + _DISC_U[None, :]]
    m10 = (patch * _DISC_U).sum(1)
    m01 = (patch * _DISC_V).sum(1)
    return np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0


def brief_bits64(blurred, x, y, angle_deg, eps=1e-4):
    """The 256 rBRIEF tests of each keypoint: pattern point (px, py) rotated by angle_deg to
    (px cos - py sin, px sin + py cos), each coordinate rounded half to even, bit = I(first) <
    I(second).  Returns (bits, ambiguous), both (n, 256) bool: a bit is ambiguous when any of
    its four rotated coordinates lies within eps of a half-integer, where a float32
    evaluation may round the other way."""
    blurred = np.asarray(blurred, np.int64)
    x = np.atleast_1d(np.asarray(x, np.int64))[:, None, None]
    y = np.atleast_1d(np.asarray(y, np.int64))[:, None, None]
    t = np.radians(np.atleast_1d(np.asarray(angle_deg, np.float64)))[:, None, None]
    px = PATTERN[None, :, :, 0].astype(np.float64)
    py = PATTERN[None, :, :, 1].astype(np.float64)
    rx = px * np.cos(t) - py * np.sin(t)
    ry = px * np.sin(t) + py * np.cos(t)
    val = blurred[y + np.rint(ry).astype(np.int64), x + np.rint(rx).astype(np.int64)]
    near = lambda r: np.abs(np.abs(r - np.floor(r)) - 0.5) < eps
    return val[:, :, 0] < val[:, :, 1], (near(rx) | near(ry)).any(axis=2)


def unpack_bits(desc):
    """(n, 32) u8 descriptors -> (n, 256) bool, bit i of the descriptor = bit i % 8 of byte
    i // 8 (the order the 256 tests are written in)."""
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little").astype(bool)


# ---------------------------------------------------------------- derived bounds, inputs
def resize_bound(simd):
    """Largest |u8 fixed-point resize - bilinear64| a correct implementation can show, in
    grey levels: final rounding 0.5; coefficient quantisation, four 11-bit coefficients each
    off by at most 0.5/2048 on a value of at most 255; and on the SIMD path the two
    high-multiply truncations, 0.25 each after the final >> 2, plus the >> 4 pre-shift of the
    horizontal sums, 2/128."""
    b = 0.5 + 4 * (0.5 / 2048) * 255
    if simd:
        b += 2 * 0.25 + 2.0 / 128
    return b


ANGLE_TOL_DEG = 0.02        # cv::fastAtan2's own accuracy (tests/test_oracle_kats.py)
AMBIGUOUS_CAP = 0.005       # share of descriptor bits per image that may be ambiguous


def circ_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def low_contrast(img):
    """frame * 0.15 + 100: nothing reaches the initial threshold, every cell falls back."""
    return np.rint(np.asarray(img, np.float64) * 0.15 + 100).astype(np.uint8)


def blocks_0_255(h, w, seed, block=4):
    """Random 0 / 255 blocks: corners of score 254 and saturating blur sums."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2, (h // block + 1, w // block + 1), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


def plateaus(h, w):
    """Equal-score neighbours: bright 2x2, 1x2, 2x1 and 3x3 blocks on a flat background (the
    ring of radius 3 misses the block's other pixels, so each of them is a corner with the
    same score and none survives), single dots that do survive, and a checkerboard."""
    img = np.full((h, w), 40, np.uint8)
    shapes = [(2, 2), (1, 2), (2, 1), (3, 3), (1, 1)]
    n = 0
    for y in range(18, h // 2 + 20, 9):
        for x in range(18, w - 20, 9):
            bh, bw = shapes[n % len(shapes)]
            img[y:y + bh, x:x + bw] = 200
            n += 1
    yy, xx = np.mgrid[h // 2 + 20:h, 0:w]
    img[h // 2 + 20:, :] = np.where(((yy // 6) + (xx // 6)) % 2 == 0, 60, 180)
    return img


def window_edge_dots(h, w):
    """Single bright pixels exactly on the first and last scored row and column of every cell
    window (rows 3 and h-4, columns 3 and w-4 of the window), nothing else.  A dot on the
    last scored column of one window is unscored in the next one and the other way round."""
    img = np.zeros((h, w), np.uint8)
    for x0, y0, x1, y1 in cell_windows(w, h):
        if y1 - y0 < 7:
            continue
        for yy in (y0 + 3, y1 - 4):
            for xx in (x0 + 3, x1 - 4):
                img[yy, xx] = 255
    return img
