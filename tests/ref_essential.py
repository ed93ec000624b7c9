"""An independent statement of Optimizer::OptimizeEssentialGraph's optimisation
(src/Optimizer.cc:1021-1286) in NumPy float64, written from g2o's definitions
(Thirdparty/g2o/g2o/types/sim3.h, se3_ops.hpp, types_seven_dof_expmap.h,
core/base_binary_edge.hpp, core/optimization_algorithm_levenberg.cpp) and not from the kernels:
nothing here is imported from the package's csrc or from oracle/.

  - one VertexSim3Expmap per keyframe, estimate (q, t, s) with q = (x, y, z, w) never
    re-normalised; oplus is Sim3(update) * estimate, update[6] = 0 under fix_scale; one vertex
    is fixed;
  - EdgeSim3 (i, j, kind): measurement C = Sjw * Swi from Scw (kind 0) or Snc (kind 1), error
    log(C * est[i] * est[j]^-1), information I, no robust kernel;
  - the numeric Jacobian of BaseBinaryEdge::linearizeOplus: central differences through oplus,
    `delta` a parameter (g2o: 1e-9), times 1 / (2 delta);
  - H and b assembled dense over the free vertices, edge by edge (`reverse` walks the edges
    backwards: another summation order), solved with np.linalg.cholesky;
  - g2o's Levenberg-Marquardt with setUserLambdaInit(1e-16), optimize(20).

Everything is vectorised over vertices or edges: a Sim3 array is a tuple (q (n, 4), t (n, 3),
s (n,)).
"""
import numpy as np

DELTA = 1e-9          # base_binary_edge.hpp:147
LAMBDA_INIT = 1e-16   # Optimizer.cc:1037
ITERATIONS = 20       # :1262
EPS = 1e-5            # sim3.h's branch threshold


# --------------------------------------------------------------------------- quaternions
def q_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def q_rotate(q, v):
    u, w = q[..., :3], q[..., 3:]
    uv = np.cross(u, v)
    return v + 2 * (w * uv + np.cross(u, uv))


def rot_of_quat(q):
    """Quaterniond::toRotationMatrix of q as it is, (..., 3, 3)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy,
                  txy + twz, 1 - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def quat_of_rot(R):
    """Eigen's Quaterniond(Matrix3d), (n, 3, 3) -> (n, 4): the branch on the trace, then on the
    largest diagonal entry (the first on ties); no normalisation."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    n = len(R)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    q = np.zeros((n, 4))
    pos = tr > 0
    with np.errstate(all="ignore"):
        s = np.sqrt(np.where(pos, tr + 1.0, 1.0))
        qa = np.stack([(R[:, 2, 1] - R[:, 1, 2]) * (0.5 / s), (R[:, 0, 2] - R[:, 2, 0]) * (0.5 / s),
                       (R[:, 1, 0] - R[:, 0, 1]) * (0.5 / s), 0.5 * s], 1)
    q[pos] = qa[pos]
    for m in np.flatnonzero(~pos):
        i = int(np.argmax(np.diag(R[m])))
        j, k = (i + 1) % 3, (i + 2) % 3
        s1 = np.sqrt(R[m, i, i] - R[m, j, j] - R[m, k, k] + 1.0)
        q[m, i] = 0.5 * s1
        s1 = 0.5 / s1
        q[m, 3] = (R[m, k, j] - R[m, j, k]) * s1
        q[m, j] = (R[m, j, i] + R[m, i, j]) * s1
        q[m, k] = (R[m, k, i] + R[m, i, k]) * s1
    return q


def skew(w):
    z = np.zeros(w.shape[:-1])
    return np.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0],
                     -w[..., 1], w[..., 0], z], -1).reshape(w.shape[:-1] + (3, 3))


# --------------------------------------------------------------------------- g2o::Sim3
def _abc(theta, sigma, s, small):
    """The coefficients of W = A Omega + B Omega^2 + C I (sim3.h:95-139 and :169-213), the
    four branches on |sigma| < 1e-5 and `small` (theta < 1e-5 in exp, d > 1 - 1e-5 in log)."""
    flat = np.abs(sigma) < EPS
    with np.errstate(all="ignore"):
        th2, sg2 = theta * theta, sigma * sigma
        C = np.where(flat, 1.0, (s - 1) / sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), th2 + sg2
        A = np.where(flat, np.where(small, 0.5, (1 - np.cos(theta)) / th2),
                     np.where(small, ((sigma - 1) * s + 1) / sg2,
                              (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(flat, np.where(small, 1.0 / 6.0, (theta - np.sin(theta)) / (th2 * theta)),
                     np.where(small, ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma),
                              (C - ((b - 1) * sigma + a * theta) / c) / th2))
    return A, B, C


def _W(A, B, C, Om):
    return A[:, None, None] * Om + B[:, None, None] * (Om @ Om) + C[:, None, None] * np.eye(3)


def sim3_exp(u):
    """Sim3(const Vector7d&), sim3.h:70-142, u (n, 7) = (omega, upsilon, sigma)."""
    u = np.asarray(u, np.float64).reshape(-1, 7)
    w, ups, sigma = u[:, :3], u[:, 3:6], u[:, 6]
    theta = np.linalg.norm(w, axis=1)
    Om = skew(w)
    s = np.exp(sigma)
    small = theta < EPS
    with np.errstate(all="ignore"):
        ra = np.where(small, 1.0, np.sin(theta) / theta)
        rb = np.where(small, 1.0, (1 - np.cos(theta)) / (theta * theta))
    R = np.eye(3) + ra[:, None, None] * Om + rb[:, None, None] * (Om @ Om)
    A, B, C = _abc(theta, sigma, s, small)
    t = np.einsum("nij,nj->ni", _W(A, B, C, Om), ups)
    return quat_of_rot(R), t, s


def sim3_log(S):
    """Sim3::log, sim3.h:148-230: (n, 7)."""
    q, t, s = S
    sigma = np.log(s)
    R = rot_of_quat(q)
    d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    small = d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.where(small, 0.0, np.arccos(np.where(small, 1.0, d)))
        k = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))
    omega = k[:, None] * dR
    A, B, C = _abc(theta, sigma, s, small)
    ups = np.linalg.solve(_W(A, B, C, skew(omega)), t[:, :, None])[:, :, 0]
    return np.concatenate([omega, ups, sigma[:, None]], 1)


def sim3_mul(a, b):
    return q_mul(a[0], b[0]), a[2][:, None] * q_rotate(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inv(a):
    qc = a[0] * np.array([-1.0, -1.0, -1.0, 1.0])
    return qc, q_rotate(qc, (-1.0 / a[2])[:, None] * a[1]), 1.0 / a[2]


def sim3_map(a, x):
    return a[2][:, None] * q_rotate(a[0], x) + a[1]


def sim3_oplus(S, u, fix_scale):
    u = np.array(u, np.float64).reshape(-1, 7)
    if fix_scale:
        u[:, 6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


# --------------------------------------------------------------------------- the graph
def measurements(sc):
    """C = Sjw * Swi per edge from Scw (kind 0) or Snc (kind 1), Optimizer.cc:1104-1258."""
    e = sc["edges"]
    k0 = (e[:, 2] == 0)
    src = tuple(np.where(k0.reshape((-1,) + (1,) * (a.ndim - 1)), a[e[:, 1]], b[e[:, 1]])
                for a, b in zip(sc["Scw"], sc["Snc"]))
    srci = tuple(np.where(k0.reshape((-1,) + (1,) * (a.ndim - 1)), a[e[:, 0]], b[e[:, 0]])
                 for a, b in zip(sc["Scw"], sc["Snc"]))
    return sim3_mul(src, sim3_inv(srci))


def edge_errors(C, Si, Sj):
    """EdgeSim3::computeError for every edge: (C * Si * Sj^-1).log(), (nedge, 7)."""
    return sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inv(Sj)))


def chi2_of(sc, C, est):
    e = sc["edges"]
    err = edge_errors(C, take(est, e[:, 0]), take(est, e[:, 1]))
    return float(np.sum(err * err))


def jacobians(sc, C, est, delta):
    """(Ji, Jj), each (nedge, 7, 7): column d = (e(+delta e_d) - e(-delta e_d)) / (2 delta),
    the perturbation applied to vertex i or to vertex j through oplus."""
    e = sc["edges"]
    Si, Sj = take(est, e[:, 0]), take(est, e[:, 1])
    scalar = 1.0 / (2 * delta)
    Ji = np.empty((len(e), 7, 7))
    Jj = np.empty((len(e), 7, 7))
    for d in range(7):
        u = np.zeros((1, 7))
        u[0, d] = delta
        Pp = sim3_oplus(est, np.repeat(u, len(est[2]), 0), sc["fix_scale"])
        Pm = sim3_oplus(est, np.repeat(-u, len(est[2]), 0), sc["fix_scale"])
        Ji[:, :, d] = scalar * (edge_errors(C, take(Pp, e[:, 0]), Sj) - edge_errors(C, take(Pm, e[:, 0]), Sj))
        Jj[:, :, d] = scalar * (edge_errors(C, Si, take(Pp, e[:, 1])) - edge_errors(C, Si, take(Pm, e[:, 1])))
    return Ji, Jj


def linearize(sc, C, est, delta=DELTA, reverse=False):
    """(H, b, chi2) dense over the free vertices (the fixed one has no rows): H += J^T J,
    b -= J^T e, edge by edge."""
    e = sc["edges"]
    n = len(est[2])
    err = edge_errors(C, take(est, e[:, 0]), take(est, e[:, 1]))
    Ji, Jj = jacobians(sc, C, est, delta)
    Hii = np.einsum("era,erb->eab", Ji, Ji)
    Hij = np.einsum("era,erb->eab", Ji, Jj)
    Hjj = np.einsum("era,erb->eab", Jj, Jj)
    bi = -np.einsum("era,er->ea", Ji, err)
    bj = -np.einsum("era,er->ea", Jj, err)
    H = np.zeros((7 * n, 7 * n))
    b = np.zeros(7 * n)
    order = range(len(e) - 1, -1, -1) if reverse else range(len(e))
    for k in order:
        i, j = 7 * e[k, 0], 7 * e[k, 1]
        H[i:i + 7, i:i + 7] += Hii[k]
        H[j:j + 7, j:j + 7] += Hjj[k]
        H[i:i + 7, j:j + 7] += Hij[k]
        H[j:j + 7, i:i + 7] += Hij[k].T
        b[i:i + 7] += bi[k]
        b[j:j + 7] += bj[k]
    free = np.ones(7 * n, bool)
    free[7 * sc["fixed"]:7 * sc["fixed"] + 7] = False
    return H[np.ix_(free, free)], b[free], float(np.sum(err * err)), free


def _solve(H, b, lam):
    A = H + lam * np.eye(len(b))
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return np.zeros(len(b)), False
    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
    return x, bool(np.isfinite(x).all())


def optimize(sc, delta=DELTA, reverse=False, iterations=ITERATIONS):
    """OptimizationAlgorithmLevenberg::solve under SparseOptimizer::optimize(iterations) with
    setUserLambdaInit(1e-16) (the rules: tests/ref_optim.py lm).  Returns a dict: q, t, s (the
    estimates), chi2 (initial, final), iterations, trials, stop = "" (every iteration ran),
    "rho" (rho == 0 or 10 failed trials) or "gain" (three iterations below 1e-3)."""
    est = tuple(np.array(a, np.float64) for a in sc["Scw"])
    n = len(est[2])
    out = dict(q=est[0], t=est[1], s=est[2], chi2=(0.0, 0.0), iterations=0, trials=0, stop="")
    if n < 2 or len(sc["edges"]) == 0 or iterations == 0:
        return out
    C = measurements(sc)
    lam, ni, nbad = 0.0, 2.0, 0
    chi0 = None
    for it in range(iterations):
        H, b, cur, free = linearize(sc, C, est, delta, reverse)
        if it == 0:
            chi0 = cur
            lam, ni, nbad = LAMBDA_INIT, 2.0, 0
        ini = cur
        q = 0
        while True:
            dx, ok = _solve(H, b, lam)
            u = np.zeros(7 * n)
            u[free] = dx
            trial = sim3_oplus(est, u.reshape(n, 7), sc["fix_scale"])
            f = sc["fixed"]
            for a, a0 in zip(trial, est):
                a[f] = a0[f]
            tmp = chi2_of(sc, C, trial)
            if not ok:
                tmp = np.finfo(np.float64).max
            rho = (cur - tmp) / (float(dx @ (lam * dx + b)) + 1e-3)
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
                est = trial
            else:
                lam *= ni
                ni *= 2
            q += 1
            out["trials"] += 1
            if not (rho < 0 and q < 10):
                break
        out["iterations"] = it + 1
        if q == 10 or rho == 0:
            out["stop"] = "rho"
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            out["stop"] = "gain"
            break
    out.update(q=est[0], t=est[1], s=est[2], chi2=(chi0, cur))
    return out


def final_chi2(sc, S):
    """sum e^T e of the scene's edges at the estimates S = (q, t, s)."""
    if len(sc["edges"]) == 0:
        return 0.0
    return chi2_of(sc, measurements(sc), tuple(np.asarray(a, np.float64) for a in S))


def poses(S):
    """Tiw = [R(q) | t * (1 / s)] in float32, (n, 3, 4) (Optimizer.cc:1266-1286)."""
    q, t, s = (np.asarray(a, np.float64) for a in S)
    return np.concatenate([rot_of_quat(q), (t * (1.0 / s)[:, None])[:, :, None]], 2).astype(np.float32)


def correct_points(Scw, Siw, ref, pts):
    """correctedSwr.map(Srw.map(P)) in double, (n, 3) float64 (:1288-1323)."""
    ref = np.asarray(ref, np.int64)
    P = np.asarray(pts, np.float32).astype(np.float64)
    Srw = take(Scw, ref)
    Swr = sim3_inv(take(Siw, ref))
    return sim3_map(Swr, sim3_map(Srw, P))


# --------------------------------------------------------------------------- scenes
def _rotvec(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(np.asarray(w, np.float64) / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(n, seed, ncorr=3, fix_scale=False, fixed=0, rot_drift=0.004, scale_drift=0.01,
          dup=False, old_loop=None, radius=10.0):
    """A camera on a circle of `radius` m, n keyframes, one lap; the odometry drifts by
    rot_drift rad and scale_drift (relative) per step (no scale drift under fix_scale).  The
    last keyframe closes the loop with keyframe `fixed`: its corrected Sim3 is the true
    relative pose on top of keyframe `fixed`'s, and the last ncorr keyframes are propagated
    from it (LoopClosing.cc:426-460).  Edges: spanning tree i -> i - 1, covisibility i -> i - 2
    and i -> i - 3 (kind 1), LoopConnections between the corrected keyframes and `fixed` and
    its two successors (kind 0).  dup: LoopConnections edges on pairs that already have a kind
    1 edge; old_loop = (i, j): a kind 1 loop edge of an earlier closure."""
    rng = np.random.default_rng(seed)
    if n < 2:
        S = (np.array([[0.0, 0.0, 0.0, 1.0]] * n), rng.normal(size=(n, 3)), np.ones(n))
        return dict(Scw=S, Snc=S, edges=np.zeros((0, 3), np.int64), fixed=0, fix_scale=fix_scale,
                    n=n)
    phi = 2 * np.pi * np.arange(n) / n
    true = []
    for a in phi:   # Tiw of a camera at 10 (cos a, sin a, 0) heading along the tangent
        Rwc = _rotvec([0, 0, a]) @ _rotvec([np.pi / 2, 0, 0])
        c = radius * np.array([np.cos(a), np.sin(a), 0.05 * np.sin(3 * a)])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rwc.T, -Rwc.T @ c
        true.append(T)
    sd = 0.0 if fix_scale else scale_drift
    drift = [true[0]]
    for i in range(1, n):
        rel = true[i] @ np.linalg.inv(true[i - 1])
        ax = rng.normal(size=3)
        rel[:3, :3] = _rotvec(ax / np.linalg.norm(ax) * rot_drift * rng.uniform(0.5, 1.5)) @ rel[:3, :3]
        rel[:3, 3] *= (1 + sd) ** i * (1 + rng.uniform(-0.01, 0.01))
        drift.append(rel @ drift[i - 1])
    Snc = (quat_of_rot(np.array([T[:3, :3] for T in drift])), np.array([T[:3, 3] for T in drift]),
           np.ones(n))
    cur = n - 1
    rel = true[cur] @ np.linalg.inv(true[fixed])
    s_loop = 1.0 if fix_scale else (1 + sd) ** (-(cur - fixed))
    Scm = (quat_of_rot(rel[None, :3, :3]), rel[None, :3, 3], np.array([s_loop]))
    S_cur = sim3_mul(Scm, take(Snc, [fixed]))
    corrected = list(range(n - ncorr, n))
    Scw = tuple(a.copy() for a in Snc)
    for i in corrected:
        Sic = sim3_mul(take(Snc, [i]), sim3_inv(take(Snc, [cur])))
        Si = sim3_mul(Sic, S_cur)
        for a, v in zip(Scw, Si):
            a[i] = v[0]
    edges = []
    for i in corrected:
        for j in (fixed, fixed + 1, fixed + 2):
            if j < n - ncorr and (i + j) % 2 == 0 or (i == cur and j == fixed):
                edges.append((i, j, 0))
    if dup:
        edges += [(cur, cur - 1, 0), (cur - 1, cur - 3, 0)]
    for i in range(1, n):
        edges.append((i, i - 1, 1))
        if old_loop and old_loop[0] == i:
            edges.append((old_loop[0], old_loop[1], 1))
        if i >= 2:
            edges.append((i, i - 2, 1))
        if i >= 3:
            edges.append((i, i - 3, 1))
    return dict(Scw=Scw, Snc=Snc, edges=np.array(edges, np.int64).reshape(-1, 3), fixed=fixed,
                fix_scale=fix_scale, n=n)


# name -> scene arguments.  "ring24_mid" also runs under fix scale ("ring24_mid_fs": the same
# scene, scale drift and all, with the scales held).
CASES = {
    "ring12": dict(n=12, seed=1),
    "ring12_fs": dict(n=12, seed=2, fix_scale=True),
    "ring24_mid": dict(n=24, seed=3, fixed=6, ncorr=4, dup=True, old_loop=(15, 3)),
    "ring24_mid_fs": dict(n=24, seed=3, fixed=6, ncorr=4, dup=True, old_loop=(15, 3)),
    "ring40": dict(n=40, seed=4, ncorr=5),
    # a long chain is badly conditioned (the smallest eigenvalue of H falls with 1 / n^2), and
    # the rounding of the difference quotients, about 1e-6 relative in H, is multiplied by the
    # condition number in the step: with the drift of the small cases the Gauss-Newton step of
    # iteration 2 is rejected ten times and where iteration 1 landed depends on the summation
    # order (chi2 differs by tens of percent).  With this drift iteration 1 lands on the optimum.
    "ring256": dict(n=256, seed=5, ncorr=6, rot_drift=0.0002, scale_drift=0.0002),
    "big_angle": dict(n=12, seed=16, rot_drift=0.25),
    "n1": dict(n=1, seed=7),
    "e0": dict(n=5, seed=8),
}

_cache = {}


def case(name):
    """(scene, reference result), computed once per process and not modified afterwards."""
    if name not in _cache:
        sc = scene(**CASES[name])
        if name == "ring24_mid_fs":
            sc["fix_scale"] = True
        if name == "e0":
            sc["edges"] = np.zeros((0, 3), np.int64)
        _cache[name] = (sc, optimize(sc))
    return _cache[name]


# EG_TOL: the bound on each component of ref_sim3opt.distance per vertex, and on the relative
# excess of the final chi2, for an implementation of this sequence against optimize(sc).  4 x
# the largest figure measured from this file alone over every case of CASES, before any GPU run
# (tests/test_essential_ref.py test_tolerance_is_measured recomputes them and asserts the
# constant is no more than 5 % above 4 x their maximum): the delta 1e-9 run against the run
# with reversed edge summation and against the run with delta 1e-6.  Both change the rounding
# of the difference quotients, eps64 |e| / delta per entry of J.  Measured per case, distance /
# relative chi2 (the maximum of the two variants):
#   ring12 4.7e-06 / 1.6e-06      ring12_fs 1.1e-07 / 1.5e-10    ring24_mid 2.4e-06 / 1.8e-06
#   ring24_mid_fs 5.6e-06 / 1.4e-09   ring40 8.7e-06 / 4.54e-05  ring256 6.9e-07 / 1.2e-05
#   big_angle 1.0e-05 / 1.4e-09
EG_TOL = 4 * 4.55e-05
