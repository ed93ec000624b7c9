"""The rules an implementation of Initializer has to meet on the cases of ref_initializer.py,
shared by tests/test_gpu_initializer.py (the device) and tests/test_initializer_ref.py (the
one-core host program lib/init_host, which runs the kernels' arithmetic without a GPU).

A run is the dict initializer.initialize returns: result, p3d [n1][3], triangulated [n1],
scores_h / scores_f [its], H21 / F21 [its][9], masks_h / masks_f [its][ceil(N / 64)].
"""
import os
import subprocess
import tempfile

import numpy as np

import ref_initializer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT_HOST = os.path.join(ROOT, "orb_slam2_test_amd", "lib", "init_host")

# cases whose hypotheses are compared with the reference, and the models compared there (on the
# exactly planar scene F is degenerate: its 8 x 9 system has a two-dimensional null space)
HYP_CASES = {"plane": (0, 1), "general": (0, 1), "n64": (0, 1), "n65": (0, 1), "some": (0, 1),
             "few": (0, 1), "far": (0, 1), "rotation": (0, 1), "planar_exact": (0,)}
# cases whose results are compared with the reference (test_initializer_ref.py asserts that
# they are determined)
RESULT_CASES = ("plane", "general", "some", "far")
# cases whose CheckRT counts and parallaxes are compared with the reference: "few" takes the
# order statistic at size - 1, the others at index 50
PARALLAX_CASES = ("plane", "general", "some", "few", "far")
ALL_CASES = tuple(R.SCENES)


def problem_of(I, sc, its):
    return I.make_problem(sc["K"], sc["sigma"], its, sc["min_parallax"], sc["min_triangulated"])


def batch_arrays(I, L, cases, cap):
    """Host arrays of a batch of (scene, sets, iterations) cases: two frames per pair."""
    np_, max_its = len(cases), max(c[2] for c in cases)
    stride = max([cap] + [len(c[0]["keys2"]) for c in cases])
    kps = np.zeros((2 * np_, stride), L.KP_DTYPE)
    counts = np.zeros(2 * np_, np.int32)
    m12 = np.full((np_, cap), -1, np.int32)
    sets = np.zeros((np_, max_its, 8), np.int32)
    probs = np.zeros(np_, L.INIT_PROBLEM_DTYPE)
    for p, (sc, s, its) in enumerate(cases):
        k1, k2 = I.as_keys(sc["keys1"]), I.as_keys(sc["keys2"])
        kps[2 * p, :len(k1)], kps[2 * p + 1, :len(k2)] = k1, k2
        counts[2 * p], counts[2 * p + 1] = len(k1), len(k2)
        m12[p, :len(k1)] = sc["matches12"]
        sets[p, :its] = s[:its]
        probs[p] = problem_of(I, sc, its)[0]
    f1 = np.arange(np_, dtype=np.int32) * 2
    return probs, kps, counts, f1, f1 + 1, m12, sets


def single_of(batch, p, sc, its):
    """Pair p of a batch's outputs (NumPy arrays) in the shape of a single run."""
    n1 = len(sc["keys1"])
    N = int(batch["results"][p]["n"])
    w = (N + 63) // 64
    return {"result": batch["results"][p], "p3d": batch["p3d"][p, :n1],
            "triangulated": batch["triangulated"][p, :n1],
            "scores_h": batch["scores_h"][p, :its], "scores_f": batch["scores_f"][p, :its],
            "H21": batch["H21"][p, :its], "F21": batch["F21"][p, :its],
            "masks_h": batch["masks_h"][p, :its, :w].astype(np.uint64),
            "masks_f": batch["masks_f"][p, :its, :w].astype(np.uint64)}


def run_host(I, L, cases, cap):
    """lib/init_host on a batch of cases: (the batch outputs, seconds)."""
    buf, dims = I.pack_host_batch(*batch_arrays(I, L, cases, cap))
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(buf)
        t = subprocess.check_output([INIT_HOST, os.path.join(d, "in"), os.path.join(d, "out")])
        with open(os.path.join(d, "out"), "rb") as f:
            out = I.unpack_host_output(f.read(), *dims)
    return out, float(t)


def host_single(I, L, sc, sets, its):
    n1 = len(sc["keys1"])
    cap = max(64, (n1 + 63) // 64 * 64)
    out, _ = run_host(I, L, [(sc, sets, its)], cap)
    return single_of(out, 0, sc, its)


def bits(I, words, n):
    return I.mask_bits(words, n) if n else np.zeros(words.shape[:-1] + (0,), bool)


# ---------------------------------------------------------------------------
# own outputs, exact
# ---------------------------------------------------------------------------
def check_own_outputs(I, sc, its, d):
    r = d["result"]
    n1 = len(sc["keys1"])
    first, _ = R.compact(sc)
    N = len(first)
    assert r["n"] == N
    run = its if N >= 8 else 0
    bh, SH = R.first_strict_max(d["scores_h"][:run])
    bf, SF = R.first_strict_max(d["scores_f"][:run])
    assert (r["best_h"], r["best_f"]) == (bh, bf)
    assert r["SH"] == np.float32(SH) and r["SF"] == np.float32(SF)
    RH, model = R.model_of(r["SH"], r["SF"])
    assert r["model"] == model
    assert r["RH"] == RH or (np.isnan(r["RH"]) and np.isnan(RH))
    # a matrix that cannot score: zero matrix, zero score, empty mask
    mh, mf = bits(I, d["masks_h"], N), bits(I, d["masks_f"], N)
    for M, s, m in ((d["H21"], d["scores_h"], mh), (d["F21"], d["scores_f"], mf)):
        dead = ~M.reshape(len(M), 9).any(1)
        assert not s[dead].any() and not m[dead].any()
        assert dead[run:].all()
        assert np.isfinite(M).all()
    if N % 64:
        for w in (d["masks_h"], d["masks_f"]):
            assert not (w[:, -1] >> np.uint64(N % 64)).any()   # bits past N
    if model == 0:
        assert r["success"] == 0 and r["nhyp"] == 0 and r["hyp"] == -1 and r["ninliers"] == 0
    inl = np.zeros(N, bool)
    if model:
        inl = mh[bh] if model == 1 else mf[bf]
        assert r["ninliers"] == int(inl.sum())
        assert r["nhyp"] in ((0, 8) if model == 1 else (4,))
    # the decision rules on the device's own counts and parallaxes
    want = (0, -1)
    if r["nhyp"]:
        want = (R.decide_H if model == 1 else R.decide_F)(
            r["ngood"], r["parallax"], r["ninliers"], np.float32(sc["min_parallax"]),
            sc["min_triangulated"])
    assert (r["success"], r["hyp"]) == want
    assert not r["ngood"][r["nhyp"]:].any() and not r["parallax"][r["nhyp"]:].any()
    assert (r["ngood"] <= r["ninliers"]).all()
    for h in range(r["nhyp"]):
        Rm, t = r["hyp_R"][h].reshape(3, 3).astype(np.float64), r["hyp_t"][h].astype(np.float64)
        if not np.isfinite(Rm).all():
            assert r["ngood"][h] == 0
            continue
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-6 and np.linalg.det(Rm) > 0
        assert abs(np.linalg.norm(t) - 1) <= 1e-6
    assert not r["hyp_R"][r["nhyp"]:].any() and not r["hyp_t"][r["nhyp"]:].any()
    tri = d["triangulated"].astype(bool)
    assert d["triangulated"].max(initial=0) <= 1
    if r["success"]:
        h = r["hyp"]
        assert np.array_equal(r["R21"], r["hyp_R"][h]) and np.array_equal(r["t21"], r["hyp_t"][h])
        assert int(tri.sum()) == r["ntriangulated"] <= r["ngood"][h]
        outside = np.ones(n1, bool)
        outside[first[inl]] = False
        assert not tri[outside].any() and not d["p3d"][outside].any()
        assert int(d["p3d"].any(1).sum()) == r["ngood"][h]     # vP3D of every counted match
        assert d["p3d"][tri].any(1).all() and np.isfinite(d["p3d"]).all()
    else:
        assert not r["R21"].any() and not r["t21"].any() and r["ntriangulated"] == 0
        assert not d["p3d"].any() and not tri.any()


# ---------------------------------------------------------------------------
# masks and scores from the device's own matrices
# ---------------------------------------------------------------------------
MAX_SKIP_H12 = 0.01   # share of H iterations whose H12i may round either way


def _rounds_either_way(x64):
    """An entry of x64 lies so close to the middle of two floats that two float64 routes to it
    (NumPy's LU inverse, the device's adjugate) may round it to different floats."""
    f = x64.astype(np.float32).astype(np.float64)
    gap = np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)
    return bool((np.abs(np.abs(x64 - f) / gap - 0.5) < 1e-6).any())


def check_masks_and_scores(I, sc, its, d):
    """NumPy's CheckHomography / CheckFundamental in the reference's float types
    (ref_initializer.check_*_f32) on the device's own float matrices: the decisions agree
    outside the threshold band and the scores to the float running-sum bound, with a full term
    per decision in the band.  H12i is not an output: it is the float64 inverse of the float
    H21i rounded once, and an iteration where that rounding could go either way is skipped.
    Returns (share of decisions in the band, share of H iterations skipped)."""
    first, second = R.compact(sc)
    N = len(first)
    if N < 8:
        return 0.0, 0.0
    m = np.concatenate([sc["keys1"][first], sc["keys2"][second]], 1)
    mh, mf = bits(I, d["masks_h"], N), bits(I, d["masks_f"], N)
    nband = ndec = nskip = nh = 0
    for it in range(its):
        for model, M, got, s in ((0, d["H21"][it], mh[it], d["scores_h"][it]),
                                 (1, d["F21"][it], mf[it], d["scores_f"][it])):
            if not M.any():
                continue
            if model == 0:
                nh += 1
                inv = np.linalg.inv(M.reshape(3, 3).astype(np.float64))
                if _rounds_either_way(inv):
                    nskip += 1
                    continue
                score, inl, chi = R.check_homography_f32(M, inv.astype(np.float32), m, sc["sigma"])
                band = R.in_band(chi.astype(np.float64), R.TH_H)
            else:
                score, inl, chi = R.check_fundamental_f32(M, m, sc["sigma"])
                band = R.in_band(chi.astype(np.float64), R.TH_F)
            sure = ~band.any(1)
            assert np.array_equal(got[sure], inl[sure]), (it, model)
            nband += int(band.sum())
            ndec += band.size
            # the float running-sum bound, and a full term per decision in the band
            tol = abs(score) * N * 2.0 ** -24 + R.TH_SCORE * band.sum()
            assert abs(float(s) - score) <= tol, (it, model, float(s), score, tol)
    return nband / max(ndec, 1), nskip / max(nh, 1)


def check_parallax(name, d):
    """CheckRT's counts and parallaxes (the order statistic sorted(vCosParallax)[min(50, size -
    1)]) of all hypotheses against the reference's, as multisets: which index holds which
    hypothesis is the SVD routines' choice.  A count may differ by the matches the reference
    finds within a band of one of CheckRT's thresholds.  A parallax is acos of a float cosine
    that comes out of eight float roundings (the three coordinates of x3D, two norms, their
    product, the dot product, the quotient) of 2^-24 relative each, and d acos(c) / dc = -1 /
    sin: 8 * 2^-24 / sin(parallax) rad, and the same again for the float x3D the cosine is
    formed from."""
    ref, _ = R.reference(name)
    r, rec = d["result"], ref["rec"]
    assert r["nhyp"] == len(rec["hyps"]) and r["ninliers"] == rec["ninliers"]
    near = max((int(c["near"].sum()) for c in rec["checks"]), default=0)
    got = sorted(zip(r["ngood"].tolist(), r["parallax"].tolist()))
    want = sorted(zip(rec["ngood"], rec["parallax"]))
    worst = 0.0
    for (g, pg), (w, pw) in zip(got, want):
        assert abs(g - w) <= near, (name, got, want)
        if near == 0 or g == w:
            tol = np.degrees(2 * 8 * 2.0 ** -24 / max(np.sin(np.radians(pw)), 2.0 ** -12)) if w else 0.0
            assert abs(pg - pw) <= tol, (name, g, pg, pw, tol)
            worst = max(worst, abs(pg - pw) / tol if tol else 0.0)
    return worst


# ---------------------------------------------------------------------------
# against the reference
# ---------------------------------------------------------------------------
def check_hypotheses(name, d, models=(0, 1)):
    ref, again = R.reference(name)
    ill = R.ill_conditioned(ref, again)
    its = len(ill)
    worst = 0.0
    for model in models:
        got = d["H21" if model == 0 else "F21"]
        want = ref["hy"]["H21" if model == 0 else "F21"]
        for it in range(its):
            if ill[it, model]:
                continue
            assert bool(got[it].any()) == bool(want[it].any()), (name, it, model)
            e = np.abs(R.unit(got[it]) - R.unit(want[it])).max()
            worst = max(worst, e)
            assert e <= R.DEVICE_TOL, (name, it, model, e)
    return worst, ill[:, list(models)].mean()


def check_results(name, d):
    sc, sets, its = R.case(name)
    ref, again = R.reference(name)
    r = d["result"]
    assert r["model"] == ref["model"] and r["success"] == ref["success"]
    assert (r["best_h"], r["best_f"])[ref["model"] - 1] == (ref["best_h"], ref["best_f"])[ref["model"] - 1]
    det = R.determined(sc, ref, again)
    if det["gap_scores_h"] > 100 * ref["n"] * 2.0 ** -24:
        assert r["best_h"] == ref["best_h"]
    if det["gap_scores_f"] > 100 * ref["n"] * 2.0 ** -24:
        assert r["best_f"] == ref["best_f"]
    assert abs(float(r["RH"]) - float(ref["RH"])) <= 1e-4
    if not ref["success"]:
        return None
    sens = R.pose_sensitivity(sc, ref)
    tol = 10 * sens + 2.0 ** -20
    eR = R.rotation_angle(r["R21"], ref["R21"])
    et = R.direction_angle(r["t21"], ref["t21"])
    assert eR <= tol[0] and et <= tol[1], (eR, et, tol)
    c = ref["rec"]["checks"][ref["hyp"]]
    first = ref["hy"]["first"]
    sure = np.ones(len(sc["keys1"]), bool)
    sure[first[c["near"]]] = False
    assert np.array_equal(d["triangulated"].astype(bool)[sure], ref["triangulated"][sure])
    both = d["p3d"].any(1) & ref["p3d"].any(1)
    assert both.sum() >= 0.9 * ref["p3d"].any(1).sum()
    rel = np.linalg.norm(d["p3d"][both] - ref["p3d"][both], axis=1) / np.linalg.norm(ref["p3d"][both], axis=1)
    assert rel.max() <= tol[2], (rel.max(), tol[2])
    return eR, et, float(rel.max()), tol
