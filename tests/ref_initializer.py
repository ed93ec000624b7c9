"""An independent float64 NumPy restatement of ORB-SLAM2's Initializer (src/Initializer.cc:
Initialize, Normalize, FindHomography / FindFundamental, ComputeH21 / ComputeF21,
CheckHomography / CheckFundamental, ReconstructF / ReconstructH, DecomposeE, CheckRT,
Triangulate), the synthetic scenes of the Initializer tests and the premises those tests rest
on.  It shares no code with the kernels: the linear algebra is numpy.linalg in float64.

What is kept of the reference's types: the keypoints are float32, Normalize's mean, scale and
normalised points are float32, the entries of ComputeH21's / ComputeF21's A are float32
products (CV_32F).  Everything after that is float64.  The 3x3 SVDs of the reconstruction use
the sign convention include/orbg.h states (a right singular vector's component of largest
magnitude is positive; DecomposeE's third vectors are cross products).  Hypothesis indices are
still not comparable between two implementations (the null vector's sign reverses the Faugeras
groups, E21's nearly equal singular values pair (R1, R2) either way): the tests compare
motions, points and the chosen hypothesis' counts.
"""
import numpy as np

K0 = (517.3, 516.5, 318.6, 255.3)
W_IMG, H_IMG = 640, 480
TH_H, TH_F, TH_SCORE = 5.991, 3.841, 5.991

# ---- the premises' constants (tests/test_initializer_ref.py asserts them on the scenes) ----
# How far the reference's own H21i / F21i (unit Frobenius norm, fixed sign) move under a 2^-40
# relative perturbation of A's entries and a flipped null vector, on an iteration that counts
# as well-conditioned; an iteration that moves further is skipped (at most MAX_ILL of them).
SENSITIVITY = 1e-7
# The device rounds its matrices to float once: 2^-24 relative per entry, 9 entries.
FLOAT_ROUND = 3 * 2.0 ** -24
DEVICE_TOL = 10 * SENSITIVITY + FLOAT_ROUND
MAX_ILL = 0.05
BAND = 1e-4          # relative distance of a chi-square from its threshold
MAX_BAND = 1e-3      # share of decisions in the band
# R21 / t21 / p3d of the float device against the float64 reference: the float H21 / F21 carry
# 2^-24 relative error; DecomposeE / Faugeras and the triangulation amplify it by the
# conditioning pose_sensitivity() measures (the reference's move under a 2^-24 perturbation of
# its own chosen matrix and under float-formed E21 / A); init_checks.check_results allows ten
# times that plus 2^-20 for the float R21, t21 and points themselves.
POSE_PERTURB = 2.0 ** -24


def intrinsics(K=K0):
    fx, fy, cx, cy = K
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def make_scene(seed, nmatch, nkeys, depth, noise=0.5, outliers=0.2, angle=0.05,
               baseline=(0.4, 0.05, 0.02), plane=None, K=K0, far=None):
    """keys1 / keys2 float32 [nkeys][2], matches12 int32 [nkeys], the planted R21 / t21 (t of
    unit length, or zero for a pure rotation) and `outlier` per match (in keys1 index order).
    depth: (lo, hi) uniform, or a plane z = d + a x + b y given as `plane` = (d, a, b); far =
    (count, lo, hi) puts the first `count` points at depths lo .. hi instead (points CheckRT
    counts but, for want of parallax, does not mark triangulated)."""
    rng = np.random.default_rng(seed)
    Km = intrinsics(K)
    R = rot_y(angle)
    C = np.asarray(baseline, np.float64)
    t = -R @ C
    pts1, pts2 = [], []
    while len(pts1) < nmatch:
        u = rng.uniform(20, W_IMG - 20)
        v = rng.uniform(20, H_IMG - 20)
        ray = np.linalg.inv(Km) @ np.array([u, v, 1.0])
        if plane is not None:
            d, a, b = plane
            z = d / (1.0 - a * ray[0] - b * ray[1])
        elif far is not None and len(pts1) < far[0]:
            z = rng.uniform(far[1], far[2])
        else:
            z = rng.uniform(*depth)
        X = ray * z
        x2 = Km @ (R @ X + t)
        if x2[2] <= 0.1:
            continue
        p2 = x2[:2] / x2[2]
        if not (5 < p2[0] < W_IMG - 5 and 5 < p2[1] < H_IMG - 5):
            continue
        pts1.append([u, v])
        pts2.append(p2)
    pts1, pts2 = np.array(pts1).reshape(-1, 2), np.array(pts2).reshape(-1, 2)
    pts1 = pts1 + rng.normal(0, noise, pts1.shape) if noise else pts1
    pts2 = pts2 + rng.normal(0, noise, pts2.shape) if noise else pts2
    out = rng.uniform(size=nmatch) < outliers
    pts2[out] = np.stack([rng.uniform(5, W_IMG - 5, out.sum()), rng.uniform(5, H_IMG - 5, out.sum())], 1)
    extra = nkeys - nmatch
    k1 = np.concatenate([pts1, np.stack([rng.uniform(5, W_IMG - 5, extra), rng.uniform(5, H_IMG - 5, extra)], 1)])
    k2 = np.concatenate([pts2, np.stack([rng.uniform(5, W_IMG - 5, extra), rng.uniform(5, H_IMG - 5, extra)], 1)])
    o1, o2 = rng.permutation(nkeys), rng.permutation(nkeys)   # slot of point k in each frame
    keys1 = np.zeros((nkeys, 2), np.float32)
    keys2 = np.zeros((nkeys, 2), np.float32)
    keys1[o1] = k1
    keys2[o2] = k2
    m12 = np.full(nkeys, -1, np.int32)
    m12[o1[:nmatch]] = o2[:nmatch]
    outlier = np.zeros(nkeys, bool)
    outlier[o1[:nmatch]] = out
    nt = np.linalg.norm(t)
    return {"keys1": keys1, "keys2": keys2, "matches12": m12, "K": tuple(K), "R": R,
            "t": t / nt if nt > 0 else t, "outlier": outlier[m12 >= 0], "sigma": 1.0,
            "min_parallax": 1.0, "min_triangulated": 50}


# name: (builder kwargs, iterations, stream seed)
SCENES = {
    "plane": (dict(seed=30, nmatch=300, nkeys=400, depth=None, plane=(5.0, 0.8, 0.3)), 200, 1),
    "general": (dict(seed=37, nmatch=300, nkeys=400, depth=(3.0, 8.0)), 200, 2),
    "n8": (dict(seed=13, nmatch=8, nkeys=12, depth=(3.0, 8.0), outliers=0.0), 32, 3),
    "n64": (dict(seed=14, nmatch=64, nkeys=70, depth=(3.0, 8.0)), 32, 4),
    "n65": (dict(seed=15, nmatch=65, nkeys=65, depth=(3.0, 8.0)), 32, 5),
    "n7": (dict(seed=16, nmatch=7, nkeys=20, depth=(3.0, 8.0)), 32, 6),
    "n0": (dict(seed=17, nmatch=0, nkeys=10, depth=(3.0, 8.0)), 32, 7),
    "rotation": (dict(seed=18, nmatch=200, nkeys=220, depth=(3.0, 8.0), baseline=(0.0, 0.0, 0.0),
                      outliers=0.1), 32, 8),
    "planar_exact": (dict(seed=19, nmatch=120, nkeys=130, depth=None, plane=(5.0, 0.8, 0.3),
                          noise=0.0, outliers=0.0), 32, 9),
    "few": (dict(seed=20, nmatch=45, nkeys=60, depth=(3.0, 8.0), outliers=0.0, noise=0.2), 32, 10),
    "some": (dict(seed=21, nmatch=70, nkeys=80, depth=(3.0, 8.0), outliers=0.0, noise=0.2), 32, 11),
    "far": (dict(seed=22, nmatch=120, nkeys=128, depth=(3.0, 8.0), outliers=0.0, noise=0.2,
                 far=(8, 400.0, 800.0)), 32, 12),
}
MAIN = ("plane", "general")


def rand_stream(seed, count):
    """`count` values of rand(): integers in [0, 2^31)."""
    return np.random.default_rng(1000 + seed).integers(0, 2 ** 31, size=count).tolist()


def draw_sets_literal(n, iterations, stream):
    """Initializer.cc:135-150, line by line, on a stream of rand() values
    (DUtils::Random::RandomInt(min, max) = min + int(rand() / (RAND_MAX + 1.0) * (max - min + 1)))."""
    sets = np.zeros((iterations, 8), np.int32)
    if n < 8:
        return sets
    it = iter(stream)
    vAllIndices = list(range(n))
    for k in range(iterations):
        vAvailableIndices = list(vAllIndices)
        for j in range(8):
            d = (len(vAvailableIndices) - 1) - 0 + 1
            randi = 0 + int(next(it) / 2147483648.0 * d)
            idx = vAvailableIndices[randi]
            sets[k, j] = idx
            vAvailableIndices[randi] = vAvailableIndices[-1]
            vAvailableIndices.pop()
    return sets


_cache = {}


def case(name):
    """(scene, sets, iterations) of a named case; the scene's arrays must not be changed."""
    if name not in _cache:
        kw, its, seed = SCENES[name]
        sc = make_scene(**kw)
        n = int((sc["matches12"] >= 0).sum())
        sets = draw_sets_literal(n, its, rand_stream(seed, its * 8))
        _cache[name] = (sc, sets, its)
    return _cache[name]


def bad_sets_case():
    """The "n64" scene with a repeated index in iteration 3 and an index out of range in
    iterations 5 (== N) and 6 (negative)."""
    sc, sets, its = case("n64")
    s = sets.copy()
    s[3, 4] = s[3, 1]
    s[5, 0] = 64
    s[6, 7] = -1
    return sc, s, its


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def compact(sc):
    """mvMatches12 (:94-109): (first, second) index arrays in i order."""
    m = sc["matches12"]
    n2 = len(sc["keys2"])
    first = np.flatnonzero((m >= 0) & (m < n2))
    return first, m[first]


def normalize(keys):
    """:984-1037 with the sums in float64 rounded once: float32 normalised points and T."""
    n = len(keys)
    mean = (keys.astype(np.float64).sum(0) / n).astype(np.float32)
    d = keys - mean
    dev = (np.abs(d).astype(np.float64).sum(0) / n).astype(np.float32)
    s = (1.0 / dev.astype(np.float64)).astype(np.float32)
    T = np.eye(3)
    T[0, 0], T[1, 1] = s[0], s[1]
    T[0, 2], T[1, 2] = np.float32(-mean[0]) * s[0], np.float32(-mean[1]) * s[1]
    return (d * s).astype(np.float32), T


def _A_h(p1, p2):
    A = np.zeros((16, 9), np.float32)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -u1, -v1, -1
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = v2 * u1, v2 * v1, v2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = u1, v1, 1
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -u2 * u1, -u2 * v1, -u2
    return A


def _A_f(p1, p2):
    A = np.zeros((8, 9), np.float32)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[:, 0], A[:, 1], A[:, 2] = u2 * u1, u2 * v1, u2
    A[:, 3], A[:, 4], A[:, 5] = v2 * u1, v2 * v1, v2
    A[:, 6], A[:, 7], A[:, 8] = u1, v1, 1
    return A


def _null(A, noise, flip):
    A = A.astype(np.float64)
    if noise is not None:
        A = A * (1.0 + 2.0 ** -40 * noise.uniform(-1, 1, A.shape))
    return np.linalg.svd(A)[2][8] * (-1.0 if flip else 1.0)


def compute_H21(p1, p2, noise=None, flip=False):
    return _null(_A_h(p1, p2), noise, flip).reshape(3, 3)


def compute_F21(p1, p2, noise=None, flip=False):
    Fpre = _null(_A_f(p1, p2), noise, flip).reshape(3, 3)
    u, w, vt = np.linalg.svd(Fpre)
    w[2] = 0
    return u @ np.diag(w) @ vt


def check_homography(H21, H12, m, sigma):
    """(score, inliers [N], chi [N][2]) on matches m = (u1, v1, u2, v2) [N][4]."""
    H21, H12 = np.asarray(H21, np.float64).reshape(3, 3), np.asarray(H12, np.float64).reshape(3, 3)
    u1, v1, u2, v2 = (m[:, k].astype(np.float64) for k in range(4))
    inv = 1.0 / (sigma * sigma)
    with np.errstate(all="ignore"):
        w = 1.0 / (H12[2, 0] * u2 + H12[2, 1] * v2 + H12[2, 2])
        a = (H12[0, 0] * u2 + H12[0, 1] * v2 + H12[0, 2]) * w
        b = (H12[1, 0] * u2 + H12[1, 1] * v2 + H12[1, 2]) * w
        chi1 = ((u1 - a) ** 2 + (v1 - b) ** 2) * inv
        w = 1.0 / (H21[2, 0] * u1 + H21[2, 1] * v1 + H21[2, 2])
        a = (H21[0, 0] * u1 + H21[0, 1] * v1 + H21[0, 2]) * w
        b = (H21[1, 0] * u1 + H21[1, 1] * v1 + H21[1, 2]) * w
        chi2 = ((u2 - a) ** 2 + (v2 - b) ** 2) * inv
        chi = np.stack([chi1, chi2], 1)
        rej = chi > TH_H
        score = np.where(rej, 0.0, TH_H - chi).sum()
    return score, ~rej.any(1), chi


def check_fundamental(F21, m, sigma):
    F = np.asarray(F21, np.float64).reshape(3, 3)
    u1, v1, u2, v2 = (m[:, k].astype(np.float64) for k in range(4))
    inv = 1.0 / (sigma * sigma)
    with np.errstate(all="ignore"):
        a2 = F[0, 0] * u1 + F[0, 1] * v1 + F[0, 2]
        b2 = F[1, 0] * u1 + F[1, 1] * v1 + F[1, 2]
        c2 = F[2, 0] * u1 + F[2, 1] * v1 + F[2, 2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
        a1 = F[0, 0] * u2 + F[1, 0] * v2 + F[2, 0]
        b1 = F[0, 1] * u2 + F[1, 1] * v2 + F[2, 1]
        c1 = F[0, 2] * u2 + F[1, 2] * v2 + F[2, 2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
        chi = np.stack([chi1, chi2], 1)
        rej = chi > TH_F
        score = np.where(rej, 0.0, TH_SCORE - chi).sum()
    return score, ~rej.any(1), chi


def _inv32(x):
    """(float)(1.0 / x): the division in double, rounded once."""
    with np.errstate(all="ignore"):
        return (1.0 / x.astype(np.float64)).astype(np.float32)


def check_homography_f32(H21, H12, m, sigma):
    """CheckHomography (:424-511) in the reference's float types and operation order, on float
    matrices: (score as the float64 sum of the float terms, inliers [N], chi float32 [N][2])."""
    f = np.float32
    h, g = np.asarray(H21, f).reshape(9), np.asarray(H12, f).reshape(9)
    u1, v1, u2, v2 = (m[:, k].astype(f) for k in range(4))
    th = f(TH_H)
    inv = _inv32(np.array(f(sigma) * f(sigma)))
    with np.errstate(all="ignore"):
        w = _inv32(g[6] * u2 + g[7] * v2 + g[8])
        a = (g[0] * u2 + g[1] * v2 + g[2]) * w
        b = (g[3] * u2 + g[4] * v2 + g[5]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w = _inv32(h[6] * u1 + h[7] * v1 + h[8])
        a = (h[0] * u1 + h[1] * v1 + h[2]) * w
        b = (h[3] * u1 + h[4] * v1 + h[5]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        chi = np.stack([chi1, chi2], 1)
        rej = chi > th
        terms = np.where(rej, f(0), th - chi)
    assert chi.dtype == np.float32 and terms.dtype == np.float32
    return float(terms.astype(np.float64).sum()), ~rej.any(1), chi


def check_fundamental_f32(F21, m, sigma):
    """CheckFundamental (:523-597), as check_homography_f32."""
    f = np.float32
    F = np.asarray(F21, f).reshape(9)
    u1, v1, u2, v2 = (m[:, k].astype(f) for k in range(4))
    th, ths = f(TH_F), f(TH_SCORE)
    inv = _inv32(np.array(f(sigma) * f(sigma)))
    with np.errstate(all="ignore"):
        a2 = F[0] * u1 + F[1] * v1 + F[2]
        b2 = F[3] * u1 + F[4] * v1 + F[5]
        c2 = F[6] * u1 + F[7] * v1 + F[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
        a1 = F[0] * u2 + F[3] * v2 + F[6]
        b1 = F[1] * u2 + F[4] * v2 + F[7]
        c1 = F[2] * u2 + F[5] * v2 + F[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
        chi = np.stack([chi1, chi2], 1)
        rej = chi > th
        terms = np.where(rej, f(0), ths - chi)
    assert chi.dtype == np.float32 and terms.dtype == np.float32
    return float(terms.astype(np.float64).sum()), ~rej.any(1), chi


def in_band(chi, th, band=BAND):
    return np.abs(chi - th) <= band * th


def first_strict_max(scores):
    """FindHomography's `currentScore > score` from 0: (best iteration or -1, score)."""
    best, s = -1, 0.0
    for i, v in enumerate(scores):
        if v > s:
            best, s = i, v
    return best, s


def unit(M):
    """A matrix up to scale: unit Frobenius norm, the entry of largest magnitude positive."""
    M = np.asarray(M, np.float64).reshape(-1)
    n = np.linalg.norm(M)
    if not np.isfinite(n) or n == 0:
        return np.zeros_like(M)
    M = M / n
    return M if M[np.argmax(np.abs(M))] > 0 else -M


def hypotheses(sc, sets, iterations, noise_seed=None, flip=False):
    """Every iteration's H21i, H12i, F21i (float64), scores, masks and chi-squares.  An
    iteration with a bad set, a matrix that is not finite or a singular H21i scores 0 with zero
    matrices."""
    first, second = compact(sc)
    N = len(first)
    pn1, T1 = normalize(sc["keys1"])
    pn2, T2 = normalize(sc["keys2"])
    m = np.concatenate([sc["keys1"][first], sc["keys2"][second]], 1).astype(np.float64)
    out = {"N": N, "first": first, "m": m, "H21": np.zeros((iterations, 3, 3)),
           "H12": np.zeros((iterations, 3, 3)), "F21": np.zeros((iterations, 3, 3)),
           "scores_h": np.zeros(iterations), "scores_f": np.zeros(iterations),
           "inl_h": np.zeros((iterations, N), bool), "inl_f": np.zeros((iterations, N), bool),
           "chi_h": np.full((iterations, N, 2), np.inf), "chi_f": np.full((iterations, N, 2), np.inf)}
    if N < 8:
        return out
    noise = np.random.default_rng(noise_seed) if noise_seed is not None else None
    for it in range(iterations):
        s = sets[it]
        if s.min() < 0 or s.max() >= N or len(set(s.tolist())) < 8:
            continue
        p1, p2 = pn1[first[s]], pn2[second[s]]
        with np.errstate(all="ignore"):
            H21 = np.linalg.inv(T2) @ compute_H21(p1, p2, noise, flip) @ T1
            ok = np.isfinite(H21).all() and np.linalg.matrix_rank(H21) == 3
            H12 = np.linalg.inv(H21) if ok else np.zeros((3, 3))
            if ok and np.isfinite(H12).all():
                out["H21"][it], out["H12"][it] = H21, H12
                out["scores_h"][it], out["inl_h"][it], out["chi_h"][it] = check_homography(
                    H21, H12, m, sc["sigma"])
            F21 = T2.T @ compute_F21(p1, p2, noise, flip) @ T1
            if np.isfinite(F21).all():
                out["F21"][it] = F21
                out["scores_f"][it], out["inl_f"][it], out["chi_f"][it] = check_fundamental(
                    F21, m, sc["sigma"])
    return out


def svd3(A, rank2=False):
    U, w, Vt = np.linalg.svd(A)
    U, V = U.copy(), Vt.T.copy()
    for k in range(3):
        j = int(np.argmax(np.abs(V[:, k])))
        if V[j, k] < 0:
            V[:, k] *= -1
            U[:, k] *= -1
    if rank2:
        U[:, 2] = np.cross(U[:, 0], U[:, 1])
        V[:, 2] = np.cross(V[:, 0], V[:, 1])
    return U, w, V


def decompose_E(E):
    """:1245-1270: R1, R2, t."""
    u, w, v = svd3(E, rank2=True)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1 = u @ W @ v.T
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = u @ W.T @ v.T
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return R1, R2, t


def triangulate(P1, P2, u1, v1, u2, v2):
    A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
    x = np.linalg.svd(A)[2][3]
    with np.errstate(all="ignore"):
        return x[:3] / x[3]


def check_RT(R, t, m, inl, K, th2):
    """:1056-1233.  Returns a dict: ngood, parallax (degrees), p3d [N][3], counted [N], good
    [N], cos [N] and near [N] (a test of that match lies within BAND of its threshold)."""
    N = len(m)
    Km = intrinsics(K)
    fx, fy, cx, cy = K
    P1 = np.hstack([Km, np.zeros((3, 1))])
    P2 = Km @ np.hstack([R, t.reshape(3, 1)])
    O2 = -R.T @ t
    p3d, counted, good = np.zeros((N, 3)), np.zeros(N, bool), np.zeros(N, bool)
    cos, near = np.zeros(N), np.zeros(N, bool)
    for i in np.flatnonzero(inl):
        u1, v1, u2, v2 = m[i]
        X = triangulate(P1, P2, u1, v1, u2, v2)
        if not np.isfinite(X).all():
            continue
        n1, n2 = X, X - O2
        c = n1.dot(n2) / (np.linalg.norm(n1) * np.linalg.norm(n2))
        cos[i] = c
        lowpar = c < 0.99998
        nr = abs(c - 0.99998) < 1e-6
        X2 = R @ X + t
        nr = nr or abs(X[2]) < 1e-4 * np.linalg.norm(X) or abs(X2[2]) < 1e-4 * np.linalg.norm(X2)
        if X[2] <= 0 and lowpar:
            near[i] = nr
            continue
        if X2[2] <= 0 and lowpar:
            near[i] = nr
            continue
        e1 = (fx * X[0] / X[2] + cx - u1) ** 2 + (fy * X[1] / X[2] + cy - v1) ** 2
        e2 = (fx * X2[0] / X2[2] + cx - u2) ** 2 + (fy * X2[1] / X2[2] + cy - v2) ** 2
        near[i] = nr or abs(e1 - th2) <= 1e-3 * th2 or abs(e2 - th2) <= 1e-3 * th2
        if e1 > th2 or e2 > th2:
            continue
        p3d[i] = X
        counted[i] = True
        good[i] = lowpar
    ngood = int(counted.sum())
    par = 0.0
    if ngood > 0:
        c = np.sort(cos[counted])[min(50, ngood - 1)]
        with np.errstate(all="ignore"):
            par = float(np.degrees(np.arccos(c)))
    return {"ngood": ngood, "parallax": par, "p3d": p3d, "counted": counted, "good": good,
            "cos": cos, "near": near}


def _f32(M):
    return M.astype(np.float32).astype(np.float64)


def hypotheses_F(F21, K, f32=False):
    """f32: the products K^T F21 and (K^T F21) K rounded to float, as the reference's CV_32F
    matrices are (pose_sensitivity's measure of what that costs)."""
    Km = intrinsics(K)
    E = _f32(_f32(_f32(Km).T @ _f32(F21)) @ _f32(Km)) if f32 else Km.T @ F21 @ Km
    R1, R2, t = decompose_E(E)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def hypotheses_H(H21, K, f32=False):
    """:760-864: the eight (R, t), or [] at the early return."""
    Km = intrinsics(K)
    A = np.linalg.inv(Km) @ H21 @ Km
    if f32:
        A = _f32(_f32(_f32(np.linalg.inv(Km)) @ _f32(H21)) @ _f32(Km))
    U, w, V = svd3(A)
    s = np.linalg.det(U) * np.linalg.det(V.T)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return []
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    out = []
    for i in range(4):
        Rp = np.eye(3)
        Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
        tp = np.array([x1[i], 0, -x3[i]]) * (d1 - d3)
        tt = U @ tp
        out.append((s * U @ Rp @ V.T, tt / np.linalg.norm(tt)))
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    for i in range(4):
        Rp = np.eye(3)
        Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
        tp = np.array([x1[i], 0, x3[i]]) * (d1 + d3)
        tt = U @ tp
        out.append((s * U @ Rp @ V.T, tt / np.linalg.norm(tt)))
    return out


def decide_F(ngood, parallax, N, min_parallax, min_triangulated):
    """:646-721 from the four counts and parallaxes: (success, hypothesis looked at or -1)."""
    ng = [int(x) for x in ngood[:4]]
    maxGood = max(ng)
    nMinGood = max(int(0.9 * N), int(min_triangulated))
    nsimilar = sum(1 for g in ng if g > 0.7 * maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return 0, -1
    k = ng.index(maxGood)
    return (1 if parallax[k] > min_parallax else 0), k


def decide_H(ngood, parallax, N, min_parallax, min_triangulated):
    """:867-923 from the eight counts and parallaxes."""
    bestGood, secondBestGood, idx, bestParallax = 0, 0, -1, -1.0
    for i in range(8):
        g = int(ngood[i])
        if g > bestGood:
            secondBestGood, bestGood, idx, bestParallax = bestGood, g, i, parallax[i]
        elif g > secondBestGood:
            secondBestGood = g
    ok = (secondBestGood < 0.75 * bestGood and bestParallax >= min_parallax
          and bestGood > min_triangulated and bestGood > 0.9 * N)
    return (1 if ok else 0), idx


def model_of(SH, SF):
    """(RH in float32, model): 0 none, 1 H, 2 F."""
    with np.errstate(all="ignore"):
        RH = np.float32(SH) / (np.float32(SH) + np.float32(SF))
    if not SH > 0 and not SF > 0:
        return RH, 0
    return RH, (1 if RH > 0.40 else 2)


def reconstruct(sc, hy, model, M, inl, f32=False):
    """ReconstructH (model 1) / ReconstructF (model 2) on the matrix M and its inlier mask."""
    K = sc["K"]
    th2 = 4.0 * sc["sigma"] ** 2
    hyps = hypotheses_H(M, K, f32) if model == 1 else hypotheses_F(M, K, f32)
    N = int(inl.sum())
    checks = [check_RT(R, t, hy["m"], inl, K, th2) for R, t in hyps]
    ng = [c["ngood"] for c in checks] + [0] * (8 - len(checks))
    par = [c["parallax"] for c in checks] + [0.0] * (8 - len(checks))
    success, which = 0, -1
    if hyps:
        success, which = (decide_H if model == 1 else decide_F)(
            ng, par, N, sc["min_parallax"], sc["min_triangulated"])
    return {"hyps": hyps, "checks": checks, "ngood": ng, "parallax": par, "success": success,
            "hyp": which, "ninliers": N}


def initialize(sc, sets, iterations, noise_seed=None, flip=False):
    """Initialize(): the hypotheses, the model, the reconstruction and the outputs."""
    hy = hypotheses(sc, sets, iterations, noise_seed, flip)
    bh, SH = first_strict_max(hy["scores_h"])
    bf, SF = first_strict_max(hy["scores_f"])
    RH, model = model_of(SH, SF)
    n1 = len(sc["keys1"])
    res = {"hy": hy, "n": hy["N"], "best_h": bh, "best_f": bf, "SH": SH, "SF": SF, "RH": RH,
           "model": model, "success": 0, "R21": np.zeros((3, 3)), "t21": np.zeros(3), "hyp": -1,
           "p3d": np.zeros((n1, 3)), "triangulated": np.zeros(n1, bool), "rec": None}
    if model == 0:
        return res
    M = hy["H21"][bh] if model == 1 else hy["F21"][bf]
    inl = hy["inl_h"][bh] if model == 1 else hy["inl_f"][bf]
    rec = reconstruct(sc, hy, model, M, inl)
    res["rec"], res["success"], res["hyp"] = rec, rec["success"], rec["hyp"]
    if rec["success"]:
        R, t = rec["hyps"][rec["hyp"]]
        c = rec["checks"][rec["hyp"]]
        res["R21"], res["t21"] = R, t
        res["p3d"][hy["first"][c["counted"]]] = c["p3d"][c["counted"]]
        res["triangulated"][hy["first"][c["good"]]] = True
    return res


_ref_cache = {}


def reference(name):
    """(the reference run of a case, the same run with A perturbed by 2^-40 and the null
    vectors flipped)."""
    if name not in _ref_cache:
        sc, sets, its = case(name)
        _ref_cache[name] = (initialize(sc, sets, its), initialize(sc, sets, its, noise_seed=5, flip=True))
    return _ref_cache[name]


def moves(ref, again):
    """Per iteration, how far unit(H21i) and unit(F21i) moved: [iterations][2]."""
    a, b = ref["hy"], again["hy"]
    its = len(a["scores_h"])
    out = np.zeros((its, 2))
    for i in range(its):
        out[i, 0] = np.abs(unit(a["H21"][i]) - unit(b["H21"][i])).max()
        out[i, 1] = np.abs(unit(a["F21"][i]) - unit(b["F21"][i])).max()
    return out


def ill_conditioned(ref, again):
    """[iterations][2] bool: the iterations compared with no other run of the same arithmetic."""
    return moves(ref, again) > SENSITIVITY


def rotation_angle(Ra, Rb):
    """The angle of Ra^T Rb, from the chord (accurate near zero, unlike the trace's arc cosine)."""
    D = np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3) - np.eye(3)
    return float(2 * np.arcsin(min(1.0, np.linalg.norm(D) / (2 * np.sqrt(2)))))


def direction_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a.dot(b)))


def pose_sensitivity(sc, ref):
    """How far the reference's own R21 (rad), t21 (rad) and p3d (relative) move when its
    chosen matrix is perturbed by 2^-24 relative, the error a float matrix carries, and when
    E21 = K^T F21 K / A = K^-1 H21 K are formed in float as the reference forms them (their
    entries cancel, so this is the larger of the two)."""
    hy = ref["hy"]
    model = ref["model"]
    M = hy["H21"][ref["best_h"]] if model == 1 else hy["F21"][ref["best_f"]]
    inl = hy["inl_h"][ref["best_h"]] if model == 1 else hy["inl_f"][ref["best_f"]]
    rng = np.random.default_rng(9)
    worst = np.zeros(3)
    for trial in range(5):
        Mp = M * (1 + POSE_PERTURB * rng.uniform(-1, 1, (3, 3))) if trial else M
        rec = reconstruct(sc, hy, model, Mp, inl, f32=(trial == 0))
        if not rec["success"]:
            return np.full(3, np.inf)
        R, t = rec["hyps"][rec["hyp"]]
        c, c0 = rec["checks"][rec["hyp"]], ref["rec"]["checks"][ref["hyp"]]
        both = c["counted"] & c0["counted"]
        dp = np.linalg.norm(c["p3d"][both] - c0["p3d"][both], axis=1) / np.linalg.norm(c0["p3d"][both], axis=1)
        worst = np.maximum(worst, [rotation_angle(R, ref["R21"]), direction_angle(t, ref["t21"]),
                                   dp.max() if len(dp) else 0.0])
    return worst


def determined(sc, ref, again):
    """The premises under which best iterations, the model and the reconstruction's decisions
    are compared between two implementations: a dict of booleans and the figures behind them."""
    hy = ref["hy"]
    N = hy["N"]
    run_bound = N * 2.0 ** -24
    out = {}
    for key, best in (("scores_h", ref["best_h"]), ("scores_f", ref["best_f"])):
        s = np.sort(hy[key])[::-1]
        out["gap_" + key] = float((s[0] - s[1]) / s[0]) if s[0] > 0 else 0.0
    chosen = "gap_scores_h" if ref["model"] == 1 else "gap_scores_f"
    out["scores"] = out[chosen] > 100 * run_bound
    out["same_best"] = (ref["best_h"], ref["best_f"], ref["model"]) == (
        again["best_h"], again["best_f"], again["model"])
    out["RH"] = abs(float(ref["RH"]) - 0.40) > 0.01
    rec = ref["rec"]
    ok = rec is not None
    if ok:
        near = max((int(c["near"].sum()) for c in rec["checks"]), default=0)
        out["near"] = near
        ng = np.array(rec["ngood"])
        lo, hi = ng - near, ng + near
        ninl = rec["ninliers"]
        # every integer comparison keeps its outcome when each count moves by `near`
        if ref["model"] == 2:
            mx = ng[:4].max()
            ok = ok and (ng[:4] == mx).sum() == 1 and near < 0.05 * mx
            ok = ok and all(not (lo[k] <= 0.7 * (mx + near) and hi[k] >= 0.7 * (mx - near))
                            for k in range(4) if ng[k] != mx)
            ok = ok and abs(mx - max(int(0.9 * ninl), sc["min_triangulated"])) > near
        else:
            srt = np.sort(ng)[::-1]
            ok = ok and srt[0] - srt[1] > 2 * near and abs(srt[1] - 0.75 * srt[0]) > 2 * near
            ok = ok and abs(srt[0] - 0.9 * ninl) > near and abs(srt[0] - sc["min_triangulated"]) > near
        k = ref["hyp"]
        if k >= 0:
            ok = ok and abs(rec["parallax"][k] - sc["min_parallax"]) > 0.01 * sc["min_parallax"]
    out["reconstruction"] = bool(ok)
    return out
