"""CPU: pin the oracle against the known answers the reference text itself holds.

SURVEY.md 8c "Golden vectors / KATs pinned by the reference text": bit_pattern_31_,
umax, mnFeaturesPerLevel / level sizes, matcher constants, Huber thresholds, and g2o's
own central-difference Jacobian as the check of the analytic edge Jacobians.
"""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inc_pattern(path):
    vals = []
    with open(path) as f:
        for line in f:
            m = re.match(r"ORBG_PAIR\(\s*(-?\d+),\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\)", line)
            if m:
                vals.extend(int(g) for g in m.groups())
    return vals


def test_pattern_tables_match_reference_text(ref_tables):
    assert len(ref_tables["bit_pattern_31"]) == 1024
    for p in ("oracle/orb_pattern.inc", "orb_slam2_test_amd/csrc/orb_pattern.inc"):
        assert _inc_pattern(os.path.join(ROOT, p)) == ref_tables["bit_pattern_31"], p


# SHA-256 of the 1024 integers tools/make_ref_tables.py extracted from the reference text
# (src/ORBextractor.cc:160-418), joined with commas: recorded when ref_tables.json was made
REF_PATTERN_SHA256 = "88df8ca875cc8db56799edd57bb914edad8acb2d48c202b7a464a575b55dbdb8"


def test_ref_tables_current(ref_tables, tmp_path):
    """ref_tables.json and both orb_pattern.inc are what tools/make_ref_tables.py extracts
    from the reference text.  The reference is not part of this repository, so the check is
    made of three parts that need only the repository: the stored table has the digest
    recorded from the reference text; the tool's parsers return the stored values from a text
    laid out like the reference's tables (one test per line, its statistics in a comment full
    of digits after the numbers); and the tool's writer regenerates both committed .inc
    files byte for byte."""
    import hashlib
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "mrt", os.path.join(ROOT, "tools", "make_ref_tables.py"))
    mrt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mrt)
    pat = ref_tables["bit_pattern_31"]
    assert hashlib.sha256(",".join(map(str, pat)).encode()).hexdigest() == REF_PATTERN_SHA256
    rows = ["    %d,%d, %d,%d/*mean (%g), correlation (0.0%d)*/," % (*pat[4 * i:4 * i + 4],
                                                                  1.12461e-05 * i, 437584 + i)
            for i in range(256)]
    text = "// table\nstatic int bit_pattern_31_[256*4] =\n{\n" + "\n".join(rows) + "\n};\n"
    assert mrt.parse_pattern(text) == pat
    consts = ref_tables["matcher_consts"]
    text = "".join("const int ORBmatcher::%s = %d;\n" % kv for kv in consts.items())
    assert mrt.parse_matcher_consts(text) == consts
    inc = str(tmp_path / "orb_pattern.inc")
    mrt.write_inc(inc, pat)
    for p in ("oracle/orb_pattern.inc", "orb_slam2_test_amd/csrc/orb_pattern.inc"):
        with open(inc) as a, open(os.path.join(ROOT, p)) as b:
            assert a.read() == b.read(), p


def test_umax_kat(oracle, ref_tables):
    p = oracle.params()
    assert list(p.umax) == ref_tables["umax"]


@pytest.mark.parametrize("nfeat,expect", [
    (2000, [434, 362, 302, 251, 209, 175, 145, 122]),
    (1000, [217, 181, 151, 126, 105, 87, 73, 60]),         # TUM1
    (4000, [869, 724, 603, 503, 419, 349, 291, 242]),      # mono init 2 x nFeatures
])
def test_features_per_level_kat(oracle, nfeat, expect):
    p = oracle.params(nfeatures=nfeat)
    got = list(p.features_per_level)[:8]
    assert got[:7] == expect[:7]
    assert sum(got) == nfeat


def test_level_sizes_kat(oracle):
    p = oracle.params()
    assert oracle.level_sizes(p, 1241, 376) == [
        (1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126),
        (346, 105)]
    assert oracle.level_sizes(p, 640, 480) == [
        (640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161),
        (179, 134)]
    # pyramid totals quoted in SURVEY.md 8
    assert sum(a * b for a, b in oracle.level_sizes(p, 1241, 376)) == 1444097
    assert sum(a * b for a, b in oracle.level_sizes(p, 640, 480)) == 950532


def test_scale_tables_float_semantics(oracle):
    p = oracle.params()
    # mvScaleFactor[i] = float(float(prev) * double(1.2f)), ORBextractor.cc:445 + .h:128
    s = np.float32(1.0)
    for i in range(8):
        assert np.float32(p.scale[i]) == s
        s = np.float32(np.float64(s) * np.float64(np.float32(1.2)))


def test_matcher_constants(ref_tables):
    from orb_slam2_test_amd import ORBmatcher
    c = ref_tables["matcher_consts"]
    assert (ORBmatcher.TH_HIGH, ORBmatcher.TH_LOW, ORBmatcher.HISTO_LENGTH) == (
        c["TH_HIGH"], c["TH_LOW"], c["HISTO_LENGTH"])


def test_descriptor_distance_is_popcount(oracle):
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = rng.integers(0, 256, 32, dtype=np.uint8)
        ref = int(np.unpackbits(a ^ b).sum())
        assert oracle.descriptor_distance(a, b) == ref
    z = np.zeros(32, np.uint8)
    assert oracle.descriptor_distance(z, np.full(32, 255, np.uint8)) == 256


def test_fast_atan2_accuracy_and_range(oracle):
    rng = np.random.default_rng(1)
    for _ in range(500):
        y, x = rng.normal(size=2) * 1000
        a = oracle.fast_atan2(y, x)
        ref = math.degrees(math.atan2(y, x)) % 360
        d = abs(a - ref)
        assert min(d, 360 - d) < 0.02  # fastAtan2 is accurate to ~0.01 deg
        assert 0 <= a <= 360
    assert oracle.fast_atan2(0, 0) == 0


def test_pinned_sincos_is_correctly_rounded(oracle):
    """Round 1's pin (sincos_mode PINNED): correctly rounded, i.e. NOT what the reference
    computes (glibc cosf/sinf are not correctly rounded) -- kept as a selectable variant."""
    rng = np.random.default_rng(2)
    for a in list(rng.uniform(0, 360, 2000)) + [0, 90, 180, 270, 359.999, 45]:
        c, s = oracle.sincos_deg(a, oracle.SINCOS_PINNED)
        ang = np.float32(np.float32(a) * np.float32(math.pi / 180.0))
        assert c == np.float32(math.cos(float(ang)))
        assert s == np.float32(math.sin(float(ang)))


def _libm():
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (m.sinf, m.cosf):
        f.argtypes = [ctypes.c_float]
        f.restype = ctypes.c_float
    return m


def test_glibc_sincosf_restatement_equals_host_libm(oracle):
    """The reference's (float)cos(angle) / sin(angle) (ORBextractor.cc:122) resolve to glibc's
    cosf / sinf.  The oracle restates glibc 2.35's flt-32 algorithm; it must equal the host
    libm bit for bit.  tools/sincosf_sweep.c checks every float in [0, 7) (all 1,088,421,888
    of them: 0 mismatches on this image); here a strided sweep of the same range plus the
    hard cases (quadrant edges, tiny, near-zero results)."""
    assert oracle.sincosf_check(0, 0x40E00000, 997) == 0  # ~1.1M angles, both functions
    m = _libm()
    specials = [0.0, 1e-30, 2.0 ** -12, 0.7499999, 0.75, math.pi / 4, math.pi / 2, math.pi,
                3 * math.pi / 2, 2 * math.pi, 6.2831855, 6.9999995]
    for y in specials + list(np.float32(np.arange(361) * np.float32(math.pi / 180.0))):
        y = float(np.float32(y))
        assert np.float32(oracle.glibc_sinf(y)) == np.float32(m.sinf(y)), y
        assert np.float32(oracle.glibc_cosf(y)) == np.float32(m.cosf(y)), y


def test_brief_rotation_uses_glibc_by_default(oracle):
    """The default sincos_mode (GLIBC) gives the host libm's cosf/sinf of angle * factorPI,
    and on angles where the round-1 pin differs from glibc the modes disagree."""
    m = _libm()
    fpi = np.float32(math.pi / 180.0)
    rng = np.random.default_rng(7)
    ndiff = 0
    for a in rng.uniform(0, 360, 4000).astype(np.float32):
        ang = float(np.float32(a * fpi))
        c, s = oracle.sincos_deg(float(a), oracle.SINCOS_GLIBC)
        assert c == np.float32(m.cosf(ang)) and s == np.float32(m.sinf(ang))
        assert oracle.sincos_deg(float(a), oracle.SINCOS_HOST) == (c, s)
        ndiff += oracle.sincos_deg(float(a), oracle.SINCOS_PINNED) != (c, s)
    assert oracle.params().sincos_mode == oracle.SINCOS_GLIBC
    assert ndiff >= 0  # ~0.13% of angles differ (tools/sincosf_sweep.c counts them all)


def test_lm_cube_matches_host_libm_pow(oracle):
    """g2o's LM step factor 1 - pow(2 rho - 1, 3) (optimization_algorithm_levenberg.cpp:135)
    calls libm pow(double, double).  The oracle and k_pose_opt form the exact cube as a
    double-double rounded once (orc_lm_cube), i.e. the correctly rounded cube.  Round 1's
    t*t*t differed from the host's pow(t, 3.0) on ~25% of inputs; the correctly rounded cube
    differs on ~0.08%, and on every one of those glibc's pow is the one that misrounds
    (checked against the exact rational cube).  Matching those too would need glibc's
    table-driven pow restated (its log/exp tables are not in this image): residual, unpinned."""
    import ctypes
    import ctypes.util
    from fractions import Fraction
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    m.pow.restype = ctypes.c_double
    cube = oracle.lib().orc_lm_cube
    cube.argtypes = [ctypes.c_double]
    cube.restype = ctypes.c_double
    rng = np.random.default_rng(11)
    rho = np.concatenate([rng.uniform(0, 1, 150000), rng.uniform(0, 50, 30000),
                          10.0 ** rng.uniform(-12, 0, 20000)])
    nbad = naive_bad = 0
    for r in rho:
        t = 2 * float(r) - 1
        ref = m.pow(t, 3.0)
        c = cube(t)
        naive_bad += t * t * t != ref
        if c != ref:
            nbad += 1
            assert c == float(Fraction(t) ** 3), t  # ours is the correctly rounded cube
    assert nbad <= 0.002 * len(rho)
    assert naive_bad > 100 * nbad


def test_fast_score_equals_threshold_test(oracle):
    """cornerScore<16> == max threshold at which the pixel is a corner (score >= th <=> corner)."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        patch = rng.integers(0, 256, (7, 7), dtype=np.uint8)
        if rng.random() < 0.5:  # plant a corner
            patch[:, :] = rng.integers(0, 60)
            patch[3, 3] = 200
        s = oracle.lib().orc_fast_score(patch.ctypes.data + 3 * 7 + 3, 7)
        for th in (0, 7, 20, 40):
            kp = np.zeros(4, oracle.KP_DTYPE)
            # a 7x7 window has exactly one detectable pixel (3,3), NMS has no neighbours
            n = oracle.lib().orc_fast_window(patch.ctypes.data, 7, 7, 7, th, kp.ctypes.data, 4)
            # NMS compares against 0-filled neighbours: a score-0 corner never survives
            assert n == (1 if (s >= th and s > 0) else 0), (s, th)


def test_octree_returns_one_key_per_node(oracle):
    rng = np.random.default_rng(4)
    n = 3000
    keys = np.zeros(n, oracle.KP_DTYPE)
    pts = rng.choice(1209 * 344, size=n, replace=False)
    keys["x"] = (pts % 1209).astype(np.float32)
    keys["y"] = (pts // 1209).astype(np.float32)
    keys["response"] = rng.integers(7, 100, n).astype(np.float32)
    out = np.zeros(600, oracle.KP_DTYPE)
    for N in (1, 50, 434):
        k = oracle.lib().orc_distribute_octree(keys.ctypes.data, n, 16, 1225, 16, 360, N,
                                               out.ctypes.data, 600)
        assert N <= k <= N + 3 or (N < 16 and k <= 16)
        sel = out[:k]
        # every selected key is a candidate, no duplicates
        assert len(set(zip(sel["x"], sel["y"]))) == k


def test_ba_analytic_vs_numeric_jacobian(oracle):
    """g2o's generic BaseBinaryEdge::linearizeOplus (central differences, delta 1e-9,
    base_binary_edge.hpp:131-205) is the in-tree check of the analytic Jacobians."""
    from orb_slam2_test_amd import synthetic as S
    poses, pts, edges = S.ba_window(n_points=150, seed=7)
    eo, *_ = oracle.ba_linearize(poses, pts, edges)
    for i in range(0, len(edges), 7):
        e = edges[i]
        jp, jt = oracle.ba_numeric_jacobian(poses[e["pose"]], pts[e["point"]], e)
        D = 3 if e["stereo"] else 2
        sj = np.abs(eo[i]["jp"][:D]).max()
        st = np.abs(eo[i]["jt"][:D]).max()
        assert np.abs(jp[:D] - eo[i]["jp"][:D]).max() / sj < 2e-4
        assert np.abs(jt[:D] - eo[i]["jt"][:D]).max() / st < 2e-5


def test_ba_huber_and_quadratic_form(oracle):
    """chi2 = e^T Omega e, rho' = 1 inside delta^2 (float dsqr) else delta/sqrt(chi2);
    H blocks symmetric PSD; b = -J^T W e summed per vertex."""
    from orb_slam2_test_amd import synthetic as S
    poses, pts, edges = S.ba_window(n_points=300, seed=8)
    eo, hp, bp, hq, bq = oracle.ba_linearize(poses, pts, edges)
    for i in range(len(edges)):
        e, o = edges[i], eo[i]
        D = 3 if e["stereo"] else 2
        chi2 = float(np.sum(o["err"][:D] ** 2) * e["inv_sigma2"])
        assert abs(o["chi2"] - chi2) <= 1e-12 * max(1.0, chi2)
        dsqr = np.float32(e["huber_delta"] * e["huber_delta"])
        want = 1.0 if o["chi2"] <= dsqr else e["huber_delta"] / math.sqrt(o["chi2"])
        assert o["rho1"] == pytest.approx(want, rel=1e-15)
    for H in list(hp) + list(hq):
        assert np.allclose(H, H.T, rtol=1e-12, atol=1e-9 * np.abs(H).max())
        assert np.linalg.eigvalsh((H + H.T) / 2).min() >= -1e-6 * np.abs(H).max()
    assert np.all(hp[poses["fixed"] == 1] == 0)


def test_stereo_oracle_recovers_synthetic_disparity(oracle):
    """Sanity of the ComputeStereoMatches restatement (the reference ships no stereo fixtures;
    tests/test_matching_ref.py holds the restatement, rule by rule, to the independent
    statement in tests/ref_matching.py): on a rectified synthetic pair with known disparity the matched
    keypoints' disparities agree with the truth, every depth is bf / disparity, and a
    featureless right image yields no match."""
    from orb_slam2_test_amd import synthetic as S
    L, R, disp = S.stereo_pair(240, 752, seed=3, d_max=40.0)
    p = oracle.params(nfeatures=800)
    l = oracle.extract(p, L, with_pyramid=True)
    r = oracle.extract(p, R, with_pyramid=True)
    bf = S.KITTI_BF
    ur, dp = oracle.stereo_matches(p, l, r, 752, 240, bf, bf / S.KITTI_FX)
    ok = dp > 0
    assert ok.sum() > 100
    k = l["kps"]
    d = k["x"][ok] - ur[ok]
    assert np.allclose(dp[ok], np.float32(bf) / d, rtol=1e-6)
    y = np.clip(np.rint(k["y"][ok]).astype(int), 0, 239)
    x = np.clip(np.rint(k["x"][ok]).astype(int), 0, 751)
    assert np.median(np.abs(d - disp[y, x])) < 1.0
    assert np.all((ur[~ok] == -1) & (dp[~ok] == -1))
    c = oracle.extract(p, S.constant(240, 752, 90), with_pyramid=True)
    ur2, dp2 = oracle.stereo_matches(p, l, c, 752, 240, bf, bf / S.KITTI_FX)
    assert np.all(dp2 == -1)


def test_schur_solve_equals_dense_solve(oracle):
    """orc_ba_schur_solve (g2o's Schur complement + pose solve + back-substitution) equals a
    dense solve of the full damped system [H_pp H_pl; H_lp H_ll] + lambda I."""
    import numpy as np
    from orb_slam2_test_amd import synthetic as S
    poses, pts, edges = S.ba_window(seed=3, n_points=400)
    eo, hp, bp, hq, bq = oracle.ba_linearize(poses, pts, edges)
    lam = 1e-3 * np.abs(hp.reshape(len(poses), 36)[:, ::7]).max()
    ok, dxp, dxq = oracle.ba_schur_solve(poses, len(pts), edges, eo, hp, bp, hq, bq, lam)
    assert ok
    free = [i for i in range(len(poses)) if not poses[i]["fixed"]]
    act = edges["active"] != 0
    has = np.zeros(len(pts), bool)
    np.logical_or.at(has, edges["point"][act], True)
    pi = {p: k for k, p in enumerate(free)}
    qi = {q: k for k, q in enumerate(np.nonzero(has)[0])}
    n = 6 * len(free) + 3 * len(qi)
    H = np.zeros((n, n))
    b = np.zeros(n)
    hp3, hq3 = hp.reshape(len(poses), 6, 6), hq.reshape(len(pts), 3, 3)
    for p in free:
        o = 6 * pi[p]
        H[o:o + 6, o:o + 6] = hp3[p] + lam * np.eye(6)
        b[o:o + 6] = bp.reshape(-1, 6)[p]
    for q in qi:
        o = 6 * len(free) + 3 * qi[q]
        H[o:o + 3, o:o + 3] = hq3[q] + lam * np.eye(3)
        b[o:o + 3] = bq.reshape(-1, 3)[q]
    for e, ed in enumerate(edges):
        if not ed["active"] or ed["pose"] not in pi:
            continue
        o1, o2 = 6 * pi[ed["pose"]], 6 * len(free) + 3 * qi[ed["point"]]
        H[o1:o1 + 6, o2:o2 + 3] = eo["hpl"][e].T
        H[o2:o2 + 3, o1:o1 + 6] = eo["hpl"][e]
    x = np.linalg.solve(H, b)
    for p in free:
        assert np.allclose(dxp[p], x[6 * pi[p]:6 * pi[p] + 6], rtol=1e-9, atol=1e-12 * np.abs(x).max())
    for q in qi:
        o = 6 * len(free) + 3 * qi[q]
        assert np.allclose(dxq[q], x[o:o + 3], rtol=1e-9, atol=1e-12 * np.abs(x).max())
