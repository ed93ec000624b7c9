"""GPU: every stage of the extractor (k_pyramid / k_resize, k_blur2, k_fast2, the quadtree's
output fields, k_orient_desc) against tests/ref_frontend.py, the independent NumPy statement
of the operations.  No oracle here: tests/test_ref_frontend.py holds the oracle to the same
module on the CPU, and the other GPU tests hold the kernels to the oracle bit for bit.

Each image runs once through extract_batch_device (B = 1) per configuration; every stage is
checked on the GPU's own previous stage (level l from level l-1, blur and candidates from the
GPU's level, angle and descriptor from the GPU's level, blurred level and angle), so a failure
names the stage.  Shapes are small: a test takes a second or two, most of it NumPy.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_frontend as R  # noqa: E402
from test_ref_frontend import FULL_SURVIVAL, INI_TH, LEGACY_K, MIN_TH, image  # noqa: E402

from orb_slam2_test_amd import ORBextractor  # noqa: E402

pytestmark = pytest.mark.gpu

NFEATURES = 3000
# kind, h, w, levels, seed
SMALL = [("frame", 97, 131, 2, 1), ("noise", 97, 131, 2, 2), ("lowc", 97, 131, 2, 3)]
MEDIUM = [("frame", 160, 200, 3, 1), ("noise", 160, 200, 3, 2)]
CRAFTED = [("edges", 97, 131, 2, 0), ("plateaus", 97, 131, 2, 0), ("blocks", 97, 131, 2, 5)]
# level sizes with (lw - 32) mod 30 and (lh - 32) mod 30 over 0, 1, 15, 29, nCols 2 and 3
SWEEP = [("noise", 92, 93, 2, 11), ("noise", 107, 121, 2, 12), ("lowc", 121, 137, 2, 13),
         ("noise", 93, 151, 2, 14)]
IMAGES = SMALL + MEDIUM + CRAFTED + SWEEP
assert all(c in FULL_SURVIVAL for c in SMALL)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def run(case, factor=1.2, env=(), gauss_k=None, resize_mode=8):
    """One B = 1 batch extraction of `case`, every output downloaded: computed once per
    configuration and shared (read-only) among the tests."""
    key = (case, factor, tuple(env), gauss_k, resize_mode)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    kind, h, w, nlevels, seed = case
    img = image(kind, h, w, seed)

    def go():
        ext = ORBextractor(NFEATURES, factor, nlevels, INI_TH, MIN_TH, gauss_k=gauss_k,
                           resize_mode=resize_mode)
        d = torch.from_numpy(img).cuda()
        ext.extract_batch_device(d.data_ptr(), 1, w, h)
        ext.ctx.sync()
        ncand, nkp = ext.ctx.batch_stats()
        kps, desc = ext.download_frame(0)
        r = dict(img=img, kps=kps, desc=desc, ncand=ncand, nkp=nkp,
                 levels=[ext.get_level(0, l) for l in range(nlevels)],
                 blurred=[ext.get_blurred_level(0, l) for l in range(nlevels)],
                 scale=np.array(ext.GetScaleFactors(), np.float32), tiled=ext.ctx.blur_tiled())
        ext.close()
        return r

    r = _with_env(dict(env), go)
    assert np.array_equal(r["levels"][0], img)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _RUNS[key] = r
    return r


_CANDS = {}


def candidates(case):
    """ref_frontend.level_candidates of every level the GPU built for `case` (default run)."""
    if case not in _CANDS:
        _CANDS[case] = [R.level_candidates(lvl, INI_TH, MIN_TH) for lvl in run(case)["levels"]]
    return _CANDS[case]


def level_coords(r):
    """The keypoints' integer coordinates on their own level, and the proof that they are
    integers there: x, y = float32(level coordinate) * float32(scale[octave])."""
    kps = r["kps"]
    s = r["scale"][kps["octave"]]
    lx = np.rint(kps["x"].astype(np.float64) / s).astype(np.int64)
    ly = np.rint(kps["y"].astype(np.float64) / s).astype(np.int64)
    assert np.array_equal(kps["x"], lx.astype(np.float32) * s)
    assert np.array_equal(kps["y"], ly.astype(np.float32) * s)
    return lx, ly


def _id(c):
    return "%s-%dx%d-L%d" % (c[0], c[2], c[1], c[3]) if isinstance(c, tuple) else str(c)


# ------------------------------------------------------------------ pyramid
# scale factor, environment, resize_mode (8: 16+8 SIMD bulk, the default; 4: 16+4; 0: scalar)
PYR_CONFIGS = [(1.2, (), 8), (1.2, (("ORBG_PYR", "0"),), 8), (1.5, (), 8), (1.2, (), 4),
               (1.2, (), 0), (1.2, (("ORBG_PYR", "0"),), 0)]


@pytest.mark.parametrize("factor,env,mode", PYR_CONFIGS,
                         ids=["k_pyramid", "k_resize_chain", "factor1.5", "simd16+4", "scalar",
                              "scalar_chain"])
def test_pyramid_levels_are_bilinear(factor, env, mode):
    """Level l is the bilinear resampling of the GPU's level l-1 within the bound derived for
    the fixed-point path in use (ref_frontend.resize_bound): the default plan (k_pyramid), the
    k_resize chain (ORBG_PYR=0), scale factor 1.5 with 3 levels, and the 16+4 and scalar
    rounding modes (the scalar bound is the tighter one)."""
    bound = R.resize_bound(simd=mode != 0)
    worst = 0.0
    cases = [MEDIUM[0], MEDIUM[1], ("blocks", 160, 200, 3, 6)]
    if factor == 1.2:  # at 1.5 a third level of the smaller images has no 30-pixel cell left
        cases += [SMALL[1], SWEEP[2]]
    for case in cases:
        r = run(case, factor, env, resize_mode=mode)
        for l in range(1, case[3]):
            src, dst = r["levels"][l - 1], r["levels"][l]
            s = np.float32(1) / r["scale"][l]
            assert dst.shape == (int(np.rint(np.float32(case[1]) * s)),
                                 int(np.rint(np.float32(case[2]) * s)))
            err = np.abs(dst - R.bilinear64(src, dst.shape[1], dst.shape[0]))
            worst = max(worst, float(err.max()))
            assert err.max() <= bound, (case, l, np.argwhere(err > bound)[:3])
    print("pyramid %s %s mode %d: max |level - bilinear64| = %.4f (bound %.4f)"
          % (factor, dict(env), mode, worst, bound))


def test_pyramid_paths_agree():
    """k_pyramid and the k_resize chain are two kernels for one operation: the same bytes."""
    for case in MEDIUM:
        a, b = run(case), run(case, 1.2, PYR_CONFIGS[1][1])
        for l in range(case[3]):
            assert np.array_equal(a["levels"][l], b["levels"][l]), (case, l)


# ------------------------------------------------------------------ blur
@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "rows"])
def test_blur_is_the_exact_integer_kernel(tiled):
    env = (("ORBG_BLUR_TILED", "1" if tiled else "0"),)
    for case, k in [(c, None) for c in MEDIUM + CRAFTED + SWEEP[:2]] + [(CRAFTED[2], LEGACY_K)]:
        r = run(case, 1.2, env, k)
        assert r["tiled"] == tiled
        for l in range(case[3]):
            ref = R.gauss7_exact(r["levels"][l], R.GAUSS_K if k is None else k)
            bad = np.argwhere(r["blurred"][l] != ref)
            assert bad.size == 0, (case, l, bad[:5])


# ------------------------------------------------------------------ candidates, keypoint fields
@pytest.mark.parametrize("case", IMAGES, ids=_id)
def test_candidates_and_keypoint_fields(case):
    r = run(case)
    cands = candidates(case)
    kps = r["kps"]
    print("%s: %s candidates, %d keypoints" % (_id(case), [len(c) for c in cands], len(kps)))
    assert r["ncand"] == sum(len(c) for c in cands)
    assert r["nkp"] == len(kps) > 0
    assert np.all(np.diff(kps["octave"]) >= 0)
    assert kps["octave"].min() >= 0 and kps["octave"].max() < case[3]
    assert np.all(kps["class_id"] == -1)
    size = (np.float32(31) * r["scale"]).astype(np.int64).astype(np.float32)
    assert np.array_equal(kps["size"], size[kps["octave"]])
    lx, ly = level_coords(r)
    for l in range(case[3]):
        m = kps["octave"] == l
        got = list(zip(lx[m].tolist(), ly[m].tolist(), kps["response"][m].astype(int).tolist()))
        assert np.array_equal(kps["response"][m], np.array([g[2] for g in got], np.float32))
        ref = set(map(tuple, cands[l].tolist()))
        assert len(set(got)) == len(got), (l, "a candidate kept twice")
        assert set(got) <= ref, (l, sorted(set(got) - ref)[:5])
        if case in FULL_SURVIVAL:
            assert set(got) == ref, (l, sorted(ref - set(got))[:5])


# ------------------------------------------------------------------ angle, descriptor
@pytest.mark.parametrize("case", SMALL + MEDIUM + CRAFTED[1:], ids=_id)
def test_angle_and_descriptor_bits(case):
    r = run(case)
    kps = r["kps"]
    lx, ly = level_coords(r)
    worst, nbits, namb = 0.0, 0, 0
    for l in range(case[3]):
        m = kps["octave"] == l
        if not m.any():
            continue
        d = R.circ_diff(kps["angle"][m], R.ic_angle64(r["levels"][l], lx[m], ly[m]))
        worst = max(worst, float(d.max()))
        assert d.max() < R.ANGLE_TOL_DEG, (l, float(d.max()))
        assert np.all((kps["angle"][m] >= 0) & (kps["angle"][m] <= 360))
        bits, amb = R.brief_bits64(r["blurred"][l], lx[m], ly[m], kps["angle"][m])
        bad = (bits != R.unpack_bits(r["desc"][m])) & ~amb
        assert not bad.any(), (l, np.argwhere(bad)[:5])
        nbits += bits.size
        namb += int(amb.sum())
    print("%s: %d keypoints, max angle diff %.4f deg, ambiguous %d / %d bits (%.3f %%)"
          % (_id(case), len(kps), worst, namb, nbits, 100.0 * namb / nbits))
    assert namb <= R.AMBIGUOUS_CAP * nbits
