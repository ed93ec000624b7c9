"""An independent statement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1366-1578) in NumPy
float64, written from g2o's definitions (Thirdparty/g2o/g2o/types/sim3.h,
types_seven_dof_expmap.h, core/base_binary_edge.hpp, core/robust_kernel_impl.cpp,
core/optimization_algorithm_levenberg.cpp) and not from the kernel: nothing here is imported
from the package's csrc or from oracle/.

  - one free VertexSim3Expmap, estimate (q, t, s) with q = (x, y, z, w) kept as g2o::Sim3 keeps
    it (never re-normalised); oplus is Sim3(update) * estimate, update[6] = 0 under fix_scale;
  - per correspondence two fixed camera-frame points (float, widened) and two edges,
    e12 = obs1 - cam_map1(project(S.map(P2c))), e21 = obs2 - cam_map2(project(S^-1.map(P1c))),
    information inv_sigma2 * I, Huber of delta = float(sqrt(th2)) with delta^2 kept in a float;
  - jacobian="numeric": g2o's central differences (delta 1e-9, 1 / (2 delta)) through oplus,
    which is what ORB-SLAM2 runs; jacobian="analytic": the closed form of the same derivative;
  - g2o's Levenberg-Marquardt; the solve is np.linalg.solve on the damped system (no LDLT);
    sums are plain NumPy sums;
  - optimize(5); drop pairs with chi2 > th2 on either edge, read at the last trial g2o
    evaluated (accepted or not); fewer than 10 left: return 0 and leave the Sim3 alone;
    optimize(nBad > 0 ? 10 : 5); the same test again; nIn.

err_dtype=np.longdouble evaluates computeError (map, project, cam_map, the subtraction) in
extended precision and rounds the residual to float64: a variant used only to measure how far
rounding inside the difference quotients moves the result (SIM3_TOL below).
"""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
DELTA = 1e-9                      # base_binary_edge.hpp:147
TH2 = 10.0                        # LoopClosing.cc:601


# --------------------------------------------------------------------------- Sim3
def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def quat_of_rot(R):
    """Eigen's Quaterniond(Matrix3d) (x, y, z, w): the branch on the trace, no normalisation."""
    R = np.asarray(R, np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        s = np.sqrt(t + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[2, 1] - R[1, 2]) * s
        q[1] = (R[0, 2] - R[2, 0]) * s
        q[2] = (R[1, 0] - R[0, 1]) * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    return q


def rot_of_quat(q):
    """Quaterniond::toRotationMatrix of q as it is (no normalisation), in Eigen's order of
    operations, so that rounding it once to float reproduces Converter::toCvMat's matrix."""
    x, y, z, w = [float(v) for v in q]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def q_rotate(q, v):
    """q * v for q = (u, w): v + 2 w (u x v) + 2 u x (u x v); v (..., 3), any float dtype."""
    u, w = q[:3], q[3]
    uv = np.cross(u, v)
    return v + 2 * (w * uv + np.cross(u, uv))


def q_mul(a, b):
    ua, wa, ub, wb = a[:3], a[3], b[:3], b[3]
    return np.concatenate([wa * ub + wb * ua + np.cross(ua, ub), [wa * wb - ua @ ub]])


def sim3_exp(u):
    """Sim3(const Vector7d&), sim3.h:70-142: u = (omega, upsilon, sigma).  R = exp(Omega)
    (below 1e-5 rad: I + Omega + Omega^2), s = exp(sigma), t = W upsilon with
    W = A Omega + B Omega^2 + C I in the four branches on |sigma| < 1e-5, theta < 1e-5."""
    u = np.asarray(u, np.float64)
    w, ups, sigma = u[:3], u[3:6], u[6]
    theta = np.linalg.norm(w)
    Om = skew(w)
    Om2 = Om @ Om
    s = np.exp(sigma)
    eps = 1e-5
    I = np.eye(3)
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 0.5, 1.0 / 6.0
            R = I + Om + Om2
        else:
            A = (1 - np.cos(theta)) / theta ** 2
            B = (theta - np.sin(theta)) / theta ** 3
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / theta ** 2 * Om2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            A = ((sigma - 1) * s + 1) / sigma ** 2
            B = ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3
            R = I + Om + Om2
        else:
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / theta ** 2 * Om2
            a, b = s * np.sin(theta), s * np.cos(theta)
            c = theta ** 2 + sigma ** 2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    W = A * Om + B * Om2 + C * I
    return quat_of_rot(R), W @ ups, float(s)


def sim3_exp_series(u, terms=40):
    """The same group element from the definition: exp of the 4x4 generator
    [[sigma I + Omega, upsilon], [0, 0]] = [[s R, W upsilon], [0, 1]], by the power series
    (W = sum_k (sigma I + Omega)^k / (k + 1)!).  Returns (R, t, s)."""
    u = np.asarray(u, np.float64)
    M = u[6] * np.eye(3) + skew(u[:3])
    E, W, P = np.eye(3), np.eye(3), np.eye(3)
    for k in range(1, terms):
        P = P @ M / k
        E = E + P
        W = W + P / (k + 1)
    s = float(np.exp(u[6]))
    return E / s, W @ u[3:6], s


def sim3_mul(a, b):
    """Sim3::operator*: (qa qb, sa (qa * tb) + ta, sa sb)."""
    return q_mul(a[0], b[0]), a[2] * q_rotate(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inv(a):
    """Sim3::inverse: (conj q, conj q * ((-1 / s) t), 1 / s)."""
    qc = np.concatenate([-a[0][:3], a[0][3:]])
    return qc, q_rotate(qc, (-1.0 / a[2]) * a[1]), 1.0 / a[2]


def sim3_map(a, x):
    return a[2] * q_rotate(a[0], x) + a[1]


def sim3_oplus(S, u, fix_scale):
    u = np.array(u, np.float64)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def sim3_from_float(R, t, s):
    """g2o::Sim3(Converter::toMatrix3d(R), toVector3d(t), s): floats widened, Quaterniond(R)."""
    return (quat_of_rot(np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)),
            np.asarray(t, np.float32).astype(np.float64).reshape(3), float(np.float32(s)))


# Quaterniond(R) from another implementation of the same formula: the inputs are exact (floats
# widened), |R_ij| <= 1 + 1e-6 and |q_i| <= 1.  The trace and t + 1 round 3 times (any
# association), the square root once and halves the relative error carried in, 0.5 / s once
# more, each off-diagonal difference once and its product once: at most 6 roundings of eps64 / 2
# relative on magnitudes <= 1 per component, 3 eps64; doubled for the branch on the largest
# diagonal entry, whose 4-term sum rounds once more: 8 eps64, absolute.  t and s are exact.
INIT_Q_BOUND = 8 * EPS64


# --------------------------------------------------------------------------- edges
def camera_points(T, Xw):
    """R Xw + t in float32, ((r0 x + r1 y) + r2 z) + t per row, widened to float64."""
    T = np.asarray(T, np.float32)[:3, :4]
    X = np.asarray(Xw, np.float32).reshape(-1, 3)
    out = np.empty((len(X), 3), np.float32)
    for r in range(3):
        out[:, r] = ((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3]
    return out.astype(np.float64)


class Problem:
    """The fixed data of one call: camera-frame points, measurements, informations."""

    def __init__(self, sc):
        f64 = np.float64
        self.P1c = camera_points(sc["T1w"], sc["Xw1"])
        self.P2c = camera_points(sc["T2w"], sc["Xw2"])
        self.obs1 = np.asarray(sc["obs1"], np.float32).astype(f64).reshape(-1, 2)
        self.obs2 = np.asarray(sc["obs2"], np.float32).astype(f64).reshape(-1, 2)
        self.w1 = np.asarray(sc["inv_sigma2_1"], np.float32).astype(f64).reshape(-1)
        self.w2 = np.asarray(sc["inv_sigma2_2"], np.float32).astype(f64).reshape(-1)
        self.K1 = np.asarray(sc["K1"], np.float32).astype(f64)   # fx, fy, cx, cy
        self.K2 = np.asarray(sc["K2"], np.float32).astype(f64)
        self.n = len(self.P1c)
        self.fix_scale = bool(sc["fix_scale"])
        self.th2 = float(np.float32(sc.get("th2", TH2)))
        self.delta = float(np.float32(np.sqrt(np.float32(self.th2))))   # const float deltaHuber
        self.dsqr = float(np.float32(self.delta * self.delta))           # float dsqr


def _project(y, K):
    return np.stack([y[:, 0] / y[:, 2] * K[0] + K[2], y[:, 1] / y[:, 2] * K[1] + K[3]], 1)


def errors(pb, S, dtype=np.float64):
    """(e12, e21), each (n, 2) float64: the two computeError statements at S."""
    c = lambda a: np.asarray(a, dtype)
    Sd = (c(S[0]), c(S[1]), dtype(S[2]))
    with np.errstate(all="ignore"):
        y12 = sim3_map(Sd, c(pb.P2c))
        y21 = sim3_map(sim3_inv(Sd), c(pb.P1c))
        e12 = c(pb.obs1) - _project(y12, c(pb.K1))
        e21 = c(pb.obs2) - _project(y21, c(pb.K2))
    return e12.astype(np.float64), e21.astype(np.float64)


def chi2s(pb, S, dtype=np.float64):
    e12, e21 = errors(pb, S, dtype)
    return pb.w1 * np.sum(e12 * e12, 1), pb.w2 * np.sum(e21 * e21, 1)


def huber(pb, chi2):
    """(rho, rho') of RobustKernelHuber::robustify on the squared error."""
    with np.errstate(all="ignore"):
        inl = chi2 <= pb.dsqr
        sq = np.sqrt(np.where(inl, 1.0, chi2))
        return (np.where(inl, chi2, 2 * sq * pb.delta - pb.dsqr),
                np.where(inl, 1.0, pb.delta / sq))


def robust_chi2(pb, S, act, dtype=np.float64):
    c12, c21 = chi2s(pb, S, dtype)
    return float(np.sum(huber(pb, c12[act])[0]) + np.sum(huber(pb, c21[act])[0]))


def jacobians_numeric(pb, S, dtype=np.float64):
    """BaseBinaryEdge::linearizeOplus: column d = (e(oplus(+delta e_d)) - e(oplus(-delta e_d)))
    * (1 / (2 delta)).  (J12, J21), each (n, 2, 7)."""
    scalar = 1.0 / (2 * DELTA)
    J12 = np.empty((pb.n, 2, 7))
    J21 = np.empty((pb.n, 2, 7))
    for d in range(7):
        u = np.zeros(7)
        u[d] = DELTA
        ap, bp = errors(pb, sim3_oplus(S, u, pb.fix_scale), dtype)
        u[d] = -DELTA
        am, bm = errors(pb, sim3_oplus(S, u, pb.fix_scale), dtype)
        J12[:, :, d] = scalar * (ap - am)
        J21[:, :, d] = scalar * (bp - bm)
    return J12, J21


def _dproj(y, K):
    """d (K project(y)) / d y, (n, 2, 3)."""
    J = np.zeros((len(y), 2, 3))
    J[:, 0, 0] = K[0] / y[:, 2]
    J[:, 0, 2] = -K[0] * y[:, 0] / y[:, 2] ** 2
    J[:, 1, 1] = K[1] / y[:, 2]
    J[:, 1, 2] = -K[1] * y[:, 1] / y[:, 2] ** 2
    return J


def _generators(y):
    """d (exp(u) y) / d u at u = 0: omega x y + upsilon + sigma y -> [-[y]x, I, y], (n, 3, 7)."""
    G = np.zeros((len(y), 3, 7))
    G[:, 0, 1], G[:, 0, 2] = y[:, 2], -y[:, 1]
    G[:, 1, 0], G[:, 1, 2] = -y[:, 2], y[:, 0]
    G[:, 2, 0], G[:, 2, 1] = y[:, 1], -y[:, 0]
    G[:, :, 3:6] = np.eye(3)
    G[:, :, 6] = y
    return G


def jacobians_analytic(pb, S):
    """The derivative the difference quotients approximate.  e12 = obs - K1 pi(y), y =
    (exp(u) S) P2c = exp(u) y: de/du = -dpi(y) G(y).  e21 = obs - K2 pi(y), y = (exp(u) S)^-1
    P1c = S^-1 exp(-u) P1c: de/du = +dpi(y) (1 / s) R^T G(P1c).  Column 6 is 0 under
    fix_scale."""
    with np.errstate(all="ignore"):
        y12 = sim3_map(S, pb.P2c)
        Si = sim3_inv(S)
        y21 = sim3_map(Si, pb.P1c)
        J12 = -np.einsum("nij,njk->nik", _dproj(y12, pb.K1), _generators(y12))
        A = Si[2] * rot_of_quat(Si[0])
        J21 = np.einsum("nij,jl,nlk->nik", _dproj(y21, pb.K2), A, _generators(pb.P1c))
    if pb.fix_scale:
        J12[:, :, 6] = 0.0
        J21[:, :, 6] = 0.0
    return J12, J21


def linearize(pb, S, act, jacobian="numeric", dtype=np.float64):
    """(H, b, robust chi2) over the active pairs: H = sum J^T (rho' Omega) J,
    b = -sum J^T Omega e rho' (base_binary_edge.hpp:91-113)."""
    e12, e21 = errors(pb, S, dtype)
    J12, J21 = jacobians_numeric(pb, S, dtype) if jacobian == "numeric" else jacobians_analytic(pb, S)
    H = np.zeros((7, 7))
    b = np.zeros(7)
    F = 0.0
    for e, J, w in ((e12, J12, pb.w1), (e21, J21, pb.w2)):
        e, J, w = e[act], J[act], w[act]
        r0, r1 = huber(pb, w * np.sum(e * e, 1))
        H += np.einsum("n,nri,nrj->ij", w * r1, J, J)
        b -= np.einsum("n,nri,nr->i", w * r1, J, e)
        F += float(np.sum(r0))
    return H, b, F


# --------------------------------------------------------------------------- g2o's LM
def _solve_damped(H, b, lam):
    A = H + lam * np.eye(7)
    try:
        np.linalg.cholesky(A)
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return np.zeros(7), False
    return x, bool(np.isfinite(x).all())


def lm(pb, S, act, iterations, jacobian, dtype):
    """OptimizationAlgorithmLevenberg::solve under SparseOptimizer::optimize (see
    tests/ref_optim.py lm for the rules).  Returns (S, last, trace): `last` the estimate of the
    last trial evaluated; trace = one dict per iteration: chi (robust chi2 at its start),
    lam (lambda entering the first trial), trials, rejected."""
    lam, ni, nbad = 0.0, 2.0, 0
    last = S
    trace = []
    for it in range(iterations):
        H, b, cur = linearize(pb, S, act, jacobian, dtype)
        if it == 0:
            lam = 1e-5 * float(np.abs(np.diag(H)).max())
            ni, nbad = 2.0, 0
        ini = cur
        rec = dict(chi=cur, lam=lam, trials=0, rejected=0)
        trace.append(rec)
        q = 0
        while True:
            dx, ok = _solve_damped(H, b, lam)
            St = sim3_oplus(S, dx, pb.fix_scale)
            tmp = robust_chi2(pb, St, act, dtype)
            last = St
            if not ok:
                tmp = np.finfo(np.float64).max
            rho = (cur - tmp) / (float(dx @ (lam * dx + b)) + 1e-3)
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
                S = St
            else:
                lam *= ni
                ni *= 2
                rec["rejected"] += 1
            q += 1
            rec["trials"] += 1
            if not (rho < 0 and q < 10):
                break
        if q == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    return S, last, trace


# --------------------------------------------------------------------------- OptimizeSim3
def optimize_sim3(sc, jacobian="numeric", err_dtype=np.float64):
    """Optimizer::OptimizeSim3 on a scene dict (see `scene`).  Returns a dict: q, t, s (the
    g2oS12 the caller holds afterwards), nIn (the return value), nBad, keep bool [n1],
    alive bool [n] (per correspondence), chi2 = [first, second] classification points, each
    (n, 2) of (e12.chi2, e21.chi2) (NaN where the pair was no longer in the graph; second is
    None on the return-0 path), trace = [trace of optimize 1, trace of optimize 2]."""
    pb = Problem(sc)
    S0 = sim3_from_float(sc["R12"], sc["t12"], sc["s12"])
    n = pb.n
    alive = np.ones(n, bool)
    out = dict(q=S0[0], t=S0[1], s=S0[2], nIn=0, nBad=0, chi2=[None, None], trace=[[], []],
               ncorr=n)

    def finish():
        keep = np.zeros(int(sc["n1"]), bool)
        keep[np.asarray(sc["index1"], np.int64)[alive]] = True
        out["keep"], out["alive"] = keep, alive.copy()
        return out

    if n == 0:
        return finish()
    S, last, out["trace"][0] = lm(pb, S0, alive, 5, jacobian, err_dtype)
    c12, c21 = chi2s(pb, last, err_dtype)
    out["chi2"][0] = np.stack([c12, c21], 1)
    with np.errstate(invalid="ignore"):
        bad = (c12 > pb.th2) | (c21 > pb.th2)
    alive &= ~bad
    out["nBad"] = int(bad.sum())
    if n - out["nBad"] < 10:
        return finish()
    S, last, out["trace"][1] = lm(pb, S, alive, 10 if out["nBad"] > 0 else 5, jacobian, err_dtype)
    c12, c21 = chi2s(pb, last, err_dtype)
    c2 = np.stack([c12, c21], 1)
    c2[~alive] = np.nan
    out["chi2"][1] = c2
    with np.errstate(invalid="ignore"):
        bad = ((c12 > pb.th2) | (c21 > pb.th2)) & alive
    alive &= ~bad
    out["nIn"] = int(alive.sum())
    out["q"], out["t"], out["s"] = S
    return finish()


def kept_cost(sc, S, alive):
    """The robust cost of the pairs `alive` at the Sim3 S = (q, t, s)."""
    return robust_chi2(Problem(sc), (np.asarray(S[0], np.float64), np.asarray(S[1], np.float64),
                                     float(S[2])), np.asarray(alive, bool))


# --------------------------------------------------------------------------- comparison rule
CLOSE = 1e-3      # a chi2 within this (relative) of th2 makes its pair's decision ambiguous
MAX_SKIPPED = 1   # ambiguous pairs a scene may have


def ambiguous(ref, th2=TH2):
    """bool [n]: pairs whose reference chi2 lies within CLOSE of th2 at either classification."""
    amb = np.zeros(ref["ncorr"], bool)
    for c in ref["chi2"]:
        if c is not None:
            with np.errstate(invalid="ignore"):
                amb |= (np.abs(c / th2 - 1) < CLOSE).any(1)
    return amb


def distance(a, b):
    """(max |Ra - Rb|, |ta - tb| / (|tb| + 1), |sa - sb| / sb) of two results."""
    Ra = rot_of_quat(np.asarray(a["q"]) / np.linalg.norm(a["q"]))
    Rb = rot_of_quat(np.asarray(b["q"]) / np.linalg.norm(b["q"]))
    tb = np.asarray(b["t"], np.float64)
    return (float(np.abs(Ra - Rb).max()),
            float(np.linalg.norm(np.asarray(a["t"]) - tb) / (np.linalg.norm(tb) + 1)),
            float(abs(a["s"] - b["s"]) / b["s"]))


# SIM3_TOL: the bound on each component of `distance` and on the relative excess of the kept
# robust cost, for an implementation of the numeric-Jacobian sequence against
# optimize_sim3(jacobian="numeric").  4 x the larger of two figures measured from this file
# alone over every case of CASES, before any GPU run (tests/test_sim3opt_ref.py
# test_tolerance_is_measured recomputes both and asserts the constant is 4 x their maximum,
# rounded up, and no more than 5 % above it):
#   numeric against analytic Jacobian:       R 1.31e-09, t 3.23e-08, s 1.147e-07
#   float64 against longdouble computeError: R 1.31e-09, t 3.03e-08, s 1.144e-07
# (the maxima come from "two_cameras").  Both variants remove or change the rounding noise of
# the difference quotients, eps64 |projection| / delta ~ 1e-7 relative per entry of J; a
# different summation order perturbs the same quotients at the same scale.
SIM3_TOL = 4 * 1.15e-07


# --------------------------------------------------------------------------- scenes
K_A = (718.856, 718.856, 607.1928, 185.2157)
K_B = (525.0, 531.5, 319.5, 241.75)


def _rotvec(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(np.asarray(w) / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _pose(rng, ang, dist):
    a = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = _rotvec(a / np.linalg.norm(a) * ang)
    T[:3, 3] = rng.normal(size=3) * dist
    return T


def scene(n, seed, n_out=0, fix_scale=False, init_angle=0.05, K2=K_A, n1_extra=7):
    """Two cameras over a random cloud at depth 4 .. 30 m of camera 1; a true Sim3 (rotation up
    to 0.3 rad, scale 0.6 .. 2.15, 1 under fix_scale); pixel noise N(0, sigma_level) with
    sigma_level = 1.2^octave; the first n_out correspondences (in a shuffled order) get a gross
    error of 20 .. 60 px on one observation; the initial Sim3 is off by up to init_angle rad,
    5 % of the translation and 5 % of the scale (0 under fix_scale).  index1 = n distinct slots
    of [0, n + n1_extra)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    s = 1.0 if fix_scale else float(rng.uniform(0.6, 2.15))
    ax = rng.normal(size=3)
    R = _rotvec(ax / np.linalg.norm(ax) * rng.uniform(0.05, 0.3))
    t = rng.uniform(-1, 1, 3) * np.array([0.8, 0.3, 0.8])
    z = rng.uniform(4, 30, n)
    P1 = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
    P2 = (P1 - t) @ R / s
    T1w, T2w = _pose(rng, 0.7, 5.0), _pose(rng, 1.1, 8.0)
    Xw1 = (P1 - T1w[:3, 3]) @ T1w[:3, :3]
    Xw2 = (P2 - T2w[:3, 3]) @ T2w[:3, :3]
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    K1 = K_A

    def proj(P, K):
        return np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], 1)
    obs1 = proj(P1, K1) + rng.normal(size=(n, 2)) * (1.2 ** o1)[:, None]
    obs2 = proj(P2, K2) + rng.normal(size=(n, 2)) * (1.2 ** o2)[:, None]
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:n_out]] = True
    for i in np.flatnonzero(outlier):
        a = rng.uniform(0, 2 * np.pi)
        d = rng.uniform(20, 60) * 1.2 ** max(o1[i], o2[i]) * np.array([np.cos(a), np.sin(a)])
        if rng.random() < 0.5:
            obs1[i] += d
        else:
            obs2[i] += d
    ax = rng.normal(size=3)
    R0 = _rotvec(ax / np.linalg.norm(ax) * init_angle * rng.uniform(0.5, 1.0)) @ R
    t0 = t * (1 + rng.uniform(-0.05, 0.05, 3))
    s0 = 1.0 if fix_scale else s * (1 + rng.uniform(-0.05, 0.05))
    n1 = n + n1_extra
    return {"T1w": T1w.astype(f), "T2w": T2w.astype(f), "K1": tuple(K1), "K2": tuple(K2),
            "Xw1": Xw1.astype(f), "Xw2": Xw2.astype(f), "obs1": obs1.astype(f),
            "obs2": obs2.astype(f), "inv_sigma2_1": (1.0 / 1.2 ** (2 * o1)).astype(f),
            "inv_sigma2_2": (1.0 / 1.2 ** (2 * o2)).astype(f),
            "index1": rng.permutation(n1)[:n].astype(np.int32), "n1": n1, "n": n,
            "R12": R0.astype(f), "t12": t0.astype(f), "s12": f(s0), "th2": TH2,
            "fix_scale": bool(fix_scale), "outlier": outlier, "true": (R, t, s)}


# name -> scene arguments.  The count cases come with fix_scale 0 and 1 ("_fs").  The seeds are
# chosen so that the premises tests/test_sim3opt_ref.py asserts hold (a case "without outlier"
# drops nothing, no decision hinges on an ambiguous pair).
_COUNT = [("n0", 0, 0), ("n9", 9, 0), ("n10", 10, 0), ("n10_out1", 10, 1), ("n11", 11, 0),
          ("n11_out1", 11, 1), ("n40", 40, 0), ("n40_out8", 40, 8), ("n257", 257, 40),
          ("n300", 300, 60)]
_SEEDS = {"n40_fs": 200}
CASES = {}
for _i, (_name, _n, _o) in enumerate(_COUNT):
    for _fs in (False, True):
        _k = _name + ("_fs" if _fs else "")
        CASES[_k] = dict(n=_n, n_out=_o, fix_scale=_fs, seed=_SEEDS.get(_k, 100 + 2 * _i + _fs))
CASES["far_init"] = dict(n=60, n_out=6, seed=_SEEDS.get("far_init", 130), init_angle=0.3)
CASES["mostly_outliers"] = dict(n=30, n_out=22, seed=_SEEDS.get("mostly_outliers", 131))
CASES["two_cameras"] = dict(n=50, n_out=8, seed=_SEEDS.get("two_cameras", 132), K2=K_B)

_cache = {}


def case(name):
    """(scene, reference result with the numeric Jacobian), computed once per process."""
    if name not in _cache:
        sc = scene(**CASES[name])
        _cache[name] = (sc, optimize_sim3(sc, "numeric"))
    return _cache[name]


def compare(sc, ref, got):
    """The comparison rule for an implementation of the numeric-Jacobian sequence.  got: dict
    with q, t, s, keep (bool [n1]), nIn, nBad, ncorr.  A pair whose reference chi2 lies within
    CLOSE of th2 at either classification is not compared (at most MAX_SKIPPED per scene);
    every other keep flag equals the reference's, slots no correspondence names are False, the
    counts equal the reference's up to the skipped pairs.  Where the second optimize ran, the
    estimate lies within SIM3_TOL of the reference's (`distance`) and the robust cost of the
    reference's kept pairs at it is at most SIM3_TOL (relative) above the reference's own; on
    the return-0 path the estimate is the input: q within INIT_Q_BOUND, t and s exact.
    Asserts; returns the figures."""
    amb = ambiguous(ref, float(sc["th2"]))
    na = int(amb.sum())
    assert na <= MAX_SKIPPED, na
    idx = np.asarray(sc["index1"], np.int64)
    keep = np.asarray(got["keep"], bool)
    assert keep.shape == ref["keep"].shape
    named = np.zeros(len(keep), bool)
    named[idx] = True
    assert not keep[~named].any()
    clear = idx[~amb]
    assert np.array_equal(keep[clear], ref["keep"][clear]), "keep differs on an unambiguous pair"
    assert int(got["ncorr"]) == ref["ncorr"]
    assert abs(int(got["nBad"]) - ref["nBad"]) <= na and abs(int(got["nIn"]) - ref["nIn"]) <= na
    fig = dict(skipped=na)
    if ref["chi2"][1] is None:
        dq = float(np.abs(np.asarray(got["q"]) - ref["q"]).max())
        fig["dq"] = dq
        assert dq <= INIT_Q_BOUND
        assert np.array_equal(np.asarray(got["t"]), ref["t"]) and float(got["s"]) == ref["s"]
        assert int(got["nIn"]) == 0
    else:
        d = distance(got, ref)
        c_ref = robust_chi2(Problem(sc), (ref["q"], ref["t"], ref["s"]), ref["alive"])
        c_got = kept_cost(sc, (got["q"], got["t"], got["s"]), ref["alive"])
        fig.update(dR=d[0], dt=d[1], ds=d[2], cost_excess=(c_got - c_ref) / c_ref)
        assert max(d) <= SIM3_TOL, d
        assert c_got <= c_ref * (1 + SIM3_TOL), (c_got, c_ref)
    return fig
