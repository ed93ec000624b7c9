"""An independent statement of Optimizer::PoseOptimization and of the LocalBundleAdjustment
arithmetic (residuals, Huber, Jacobians, the normal-equation blocks, the damped solve, the
SE3 update and g2o's Levenberg-Marquardt), in NumPy float64.

It is written from the definitions of the operations and from the text of the reference
(src/Optimizer.cc, Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp}, se3quat.h,
core/robust_kernel_impl.{h,cpp}, core/optimization_algorithm_levenberg.cpp,
core/sparse_optimizer.cpp, core/base_{unary,binary}_edge.hpp), not from oracle/*.c or the
kernels, and imports nothing from oracle/.  Where the reference departs from the pure
definition (float casts, a float Huber threshold, a first-order exp map below 1e-5 rad) the
departure is a named switch here and the pure definition is the other setting.

What is deliberately *not* taken from g2o:
  - Jacobians.  They are complex-step derivatives of `project(casts=None)`; g2o's analytic
    formulas appear nowhere in this file.
  - The exp map.  `se3_exp` is scipy's `expm` of the 4x4 twist.
  - The linear solve.  `np.linalg.solve` on the full damped system; no Schur complement,
    no LDLT.
  - Summation order.  Plain NumPy sums.

Conventions: a pose is a 4x4 float64 world -> camera matrix; quaternions are (x, y, z, w);
a twist is (omega, upsilon) in g2o's order and acts by left multiplication
(types_six_dof_expmap.h:73-76); `cam` is (fx, fy, cx, cy, bf), scalars or per-edge arrays.
"""
import numpy as np
from scipy.linalg import expm

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)

CHI2_MONO, CHI2_STEREO = 5.991, 7.815            # Optimizer.cc:510-511, :879, :895
# `const float deltaMono = sqrt(5.991)` (Optimizer.cc:393-394, :758-759): delta is a float
DELTA_MONO = float(np.float32(np.sqrt(5.991)))
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))

# The float casts of the two stereo cam_project variants.
#   CASTS_ONLY_POSE  EdgeStereoSE3ProjectXYZOnlyPose::cam_project, types_six_dof_expmap.cpp:
#                    299-306: `const float invz = 1.0f/trans_xyz[2]`; `bf` is the edge's double
#                    member (types_six_dof_expmap.h:201), so `bf*invz` is a double product.
#   CASTS_BA         EdgeStereoSE3ProjectXYZ::cam_project(trans_xyz, const float &bf), .cpp:
#                    150-157: the same float invz, and the argument binds the double member
#                    (h:140) to a `const float&`, so bf is rounded to float and `bf*invz` is a
#                    float product, widened only for the subtraction.
# The mono edges (cpp:141-147, :290-296) go through project2d in double: no cast in either.
CASTS_ONLY_POSE = "only_pose"
CASTS_BA = "ba"


# --------------------------------------------------------------------------- projection
def _cam(cam):
    return [np.asarray(c, np.float64) for c in cam]


def project(xc, cam, stereo, casts=None):
    """(u, v, u_r) of camera-frame points xc (..., 3): u = fx x/z + cx, v = fy y/z + cy,
    u_r = u - bf/z.  `stereo` (bool, per edge) only matters for the casts: a mono edge has
    none.  casts=None is the definition (and accepts complex xc); CASTS_ONLY_POSE / CASTS_BA
    add the reference's float roundings listed above."""
    fx, fy, cx, cy, bf = _cam(cam)
    x, y, z = xc[..., 0], xc[..., 1], xc[..., 2]
    u = fx * x / z + cx
    v = fy * y / z + cy
    ur = u - bf / z
    if casts is None:
        return np.stack([u, v, ur], -1)
    if casts not in (CASTS_ONLY_POSE, CASTS_BA):
        raise ValueError(casts)
    st = np.broadcast_to(np.asarray(stereo, bool), u.shape)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        invz32 = (1.0 / z).astype(np.float32)
        invz = invz32.astype(np.float64)
        us = x * invz * fx + cx
        vs = y * invz * fy + cy
        if casts == CASTS_ONLY_POSE:
            urs = us - bf * invz
        else:
            urs = us - (bf.astype(np.float32) * invz32).astype(np.float64)
    return np.stack([np.where(st, us, u), np.where(st, vs, v), np.where(st, urs, ur)], -1)


def residuals(obs, xc, cam, stereo, casts=None):
    """measurement - projection (computeError, types_six_dof_expmap.h:90-95, :122-127,
    :153-157, :184-188); a mono edge has two rows, its third is 0 here."""
    r = np.asarray(obs, np.float64) - project(xc, cam, stereo, casts)
    st = np.broadcast_to(np.asarray(stereo, bool), r.shape[:-1])
    r[..., 2] = np.where(st, r[..., 2], 0.0)
    return r


def chi2_of(err, inv_sigma2):
    """e^T (inv_sigma2 I) e (setInformation(Identity * invSigma2), Optimizer.cc:427, :469)."""
    return np.asarray(inv_sigma2, np.float64) * np.sum(err * err, -1)


def huber(chi2, delta, float_dsqr=True):
    """Huber on the squared error e = chi2: rho = e, rho' = 1 for e <= delta^2, else
    rho = 2 delta sqrt(e) - delta^2, rho' = delta / sqrt(e).  float_dsqr: the reference keeps
    delta^2 in a `float dsqr` member (robust_kernel_impl.h:84, set from delta*delta in
    robust_kernel_impl.cpp:65-69) and uses it in both the <= test and rho (cpp:78-91)."""
    chi2 = np.asarray(chi2, np.float64)
    delta = np.asarray(delta, np.float64)
    dsqr = delta * delta
    if float_dsqr:
        dsqr = dsqr.astype(np.float32).astype(np.float64)
    inl = chi2 <= dsqr
    s = np.sqrt(np.where(inl, 1.0, chi2))
    return np.where(inl, chi2, 2 * s * delta - dsqr), np.where(inl, 1.0, delta / s)


# --------------------------------------------------------------------------- SE3
def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def quat_to_rot(q):
    """Rotation matrix of a quaternion (x, y, z, w), normalised first; q: (..., 4)."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - z * w)
    R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w)
    R[..., 2, 1] = 2 * (y * z + x * w)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def rot_to_quat(R):
    """Unit quaternion (x, y, z, w) with w >= 0 of a (nearly) orthogonal 3x3 R: the branch on
    the trace / largest diagonal entry that keeps the square root well conditioned."""
    R = np.asarray(R, np.float64)
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s,
                      0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def rot_dist(Ra, Rb):
    """||Ra Rb^T - I||_max: about the rotation angle between them for small angles, and it
    does not quantise near 0 as arccos of the trace does."""
    return float(np.abs(np.asarray(Ra) @ np.asarray(Rb).T - np.eye(3)).max())


def pose_matrix(q, t):
    T = np.eye(4)
    T[:3, :3] = quat_to_rot(q)
    T[:3, 3] = t
    return T


def pose_from_float(Tcw):
    """Converter::toSE3Quat (Converter.cc:37-47): the float pose widened to double, its
    rotation block replaced by the rotation of its unit quaternion (SE3Quat keeps a
    quaternion, so whatever non-orthogonality the float matrix has is dropped)."""
    T = np.asarray(Tcw, np.float32).astype(np.float64)
    return pose_matrix(rot_to_quat(T[:3, :3]), T[:3, 3])


def se3_exp(dx, first_order_below=None):
    """exp of the twist (omega, upsilon): expm([[skew(omega), upsilon], [0, 0]]).
    first_order_below=1e-5 adds SE3Quat::exp's other branch (se3quat.h:237-243): for
    |omega| below it, R = I + W + W^2 and V = R (translation R upsilon), the rotation then
    re-normalised through the quaternion as SE3Quat's constructor does."""
    dx = np.asarray(dx, np.float64)
    w, v = dx[:3], dx[3:]
    if first_order_below is not None and np.linalg.norm(w) < first_order_below:
        W = skew(w)
        R = np.eye(3) + W + W @ W
        T = np.eye(4)
        T[:3, :3] = quat_to_rot(rot_to_quat(R))
        T[:3, 3] = R @ v
        return T
    A = np.zeros((4, 4))
    A[:3, :3] = skew(w)
    A[:3, 3] = v
    return expm(A)


def oplus(T, dx, first_order_below=None):
    """VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:73-76): exp(dx) * T."""
    return se3_exp(dx, first_order_below) @ T


# --------------------------------------------------------------------------- Jacobians
_H = 1e-30
_E6 = np.eye(6)


def jacobian_pose(xc, cam, stereo):
    """d residual / d twist at the identity increment, by complex step through
    project(casts=None): column k is Im r(xc + i h (omega_k x xc + upsilon_k)) / h for the
    k-th unit twist, order (omega, upsilon), left multiplication.  (..., 3, 6); the third row
    of a mono edge is 0."""
    xc = np.asarray(xc, np.float64)
    J = np.empty(xc.shape[:-1] + (3, 6))
    st = np.broadcast_to(np.asarray(stereo, bool), xc.shape[:-1])
    for k in range(6):
        d = np.cross(_E6[k, :3], xc) + _E6[k, 3:]
        J[..., k] = -project(xc + 1j * _H * d, cam, stereo).imag / _H
    J[..., 2, :] = np.where(st[..., None], J[..., 2, :], 0.0)
    return J


def jacobian_point(xc, R, cam, stereo):
    """d residual / d world point: Im r(xc + i h R d_k) / h.  (..., 3, 3)."""
    xc = np.asarray(xc, np.float64)
    J = np.empty(xc.shape[:-1] + (3, 3))
    st = np.broadcast_to(np.asarray(stereo, bool), xc.shape[:-1])
    for k in range(3):
        d = R[..., :, k]
        J[..., k] = -project(xc + 1j * _H * d, cam, stereo).imag / _H
    J[..., 2, :] = np.where(st[..., None], J[..., 2, :], 0.0)
    return J


# --------------------------------------------------------------------------- g2o's LM
def _solve_damped(H, b, lam):
    """(H + lam I) x = b; ok is False when the damped matrix is not positive definite (the
    reference's Cholesky-type solvers report failure then) or the solution is not finite."""
    A = H + lam * np.eye(len(b))
    try:
        np.linalg.cholesky(A)
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return np.zeros_like(b), False
    return x, bool(np.isfinite(x).all())


def lm(x, iterations, linearize, robust_chi2, apply):
    """OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-164)
    under SparseOptimizer::optimize (sparse_optimizer.cpp:354-419), generic over the problem:
      linearize(x) -> (H, b, F)   the undamped normal equations H dx = b and the robust chi2
      robust_chi2(x) -> F
      apply(x, dx) -> x'
    Rules: lambda starts at 1e-5 max|diag H| of the first system (computeLambdaInit, tau
    1e-5); a trial solves with lambda added to the diagonal, applies it and is accepted when
    rho = (F - F') / (dx.(lambda dx + b) + 1e-3) > 0 and F' is finite; then lambda *=
    clamp(1 - (2 rho - 1)^3, 1/3, 2/3) and ni = 2; else lambda *= ni, ni *= 2 and the
    state is restored.  An iteration retries while rho < 0, at most 10 trials.  It terminates
    on 10 trials or rho == 0, and on the third consecutive iteration that improved F by less
    than 0.1 %.  Returns (x, report); report["last_trial"] is the state of the last error
    pass (the last trial, accepted or not), which is what the edges' errors refer to
    afterwards."""
    rep = dict(iterations=0, trials=0, terminated=0, initial_chi2=None, final_chi2=None,
               last_trial=x, min_abs_rho=np.inf, min_stop_margin=np.inf)
    lam, ni, nbad = 0.0, 2.0, 0
    cur = None
    for it in range(iterations):
        H, b, cur = linearize(x)
        if it == 0:
            rep["initial_chi2"] = cur
            lam = 1e-5 * float(np.abs(np.diag(H)).max()) if len(b) else 0.0
            ni, nbad = 2.0, 0
        ini = cur
        q = 0
        step = 0.0
        while True:
            dx, ok = _solve_damped(H, b, lam)
            xt = apply(x, dx)
            tmp = robust_chi2(xt)
            rep["last_trial"] = xt
            if not ok:
                tmp = np.finfo(np.float64).max
            rho = (cur - tmp) / (float(dx @ (lam * dx + b)) + 1e-3)
            step = float(np.abs(dx).max()) if len(dx) else 0.0
            if step > 1e-6:
                rep["min_abs_rho"] = min(rep["min_abs_rho"], abs(rho))
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
                x = xt
            else:
                lam *= ni
                ni *= 2
            q += 1
            rep["trials"] += 1
            if not (rho < 0 and q < 10):
                break
        rep["iterations"] += 1
        if q == 10 or rho == 0:
            rep["terminated"] = 1
            break
        small = (ini - cur) * 1e3 < ini
        if step > 1e-6 and ini > 0:
            rep["min_stop_margin"] = min(rep["min_stop_margin"], abs((ini - cur) * 1e3 / ini - 1))
        nbad = nbad + 1 if small else 0
        if nbad >= 3:
            rep["terminated"] = 2
            break
    if cur is None:
        cur = robust_chi2(x)
        rep["initial_chi2"] = cur
    rep["final_chi2"] = cur
    rep["lambda"] = lam
    return x, rep


# --------------------------------------------------------------------------- PoseOptimization
def _pose_edges(edges):
    st = np.asarray(edges["stereo"]) != 0
    return (np.asarray(edges["obs"], np.float64), np.asarray(edges["xw"], np.float64),
            np.asarray(edges["inv_sigma2"], np.float64), st)


def pose_edge_terms(T, obs, xw, w, st, cam, casts=CASTS_ONLY_POSE):
    xc = xw @ T[:3, :3].T + T[:3, 3]
    err = residuals(obs, xc, cam, st, casts)
    return xc, err, chi2_of(err, w)


def _pose_problem(obs, xw, w, st, cam, active, robust, casts, float_dsqr):
    o, x, ww, s = obs[active], xw[active], w[active], st[active]
    delta = np.where(s, DELTA_STEREO, DELTA_MONO)

    def rchi2(T):
        c = pose_edge_terms(T, o, x, ww, s, cam, casts)[2]
        return float(np.sum(huber(c, delta, float_dsqr)[0] if robust else c))

    def linearize(T):
        xc, err, c = pose_edge_terms(T, o, x, ww, s, cam, casts)
        r0, r1 = huber(c, delta, float_dsqr) if robust else (c, np.ones_like(c))
        J = jacobian_pose(xc, cam, s)
        wt = ww * r1
        H = np.einsum("e,eri,erj->ij", wt, J, J)
        b = -np.einsum("e,eri,er->i", wt, J, err)
        return H, b, float(np.sum(r0))

    return linearize, rchi2, oplus


def pose_optimization(edges, cam, Tcw0, casts=CASTS_ONLY_POSE, float_dsqr=True,
                      classify_at_last_trial=True):
    """Optimizer::PoseOptimization (Optimizer.cc:356-596).  Fewer than 3 edges: nothing
    happens (:497).  Otherwise 4 rounds; each resets the pose to the frame's (:518), runs
    optimize(10) over the edges not flagged in the previous round (level 0, :520), with
    Huber in rounds 0-2 (:551, :581), then classifies every edge by float chi2 > float
    threshold (:537-539, :567-569).  A flagged edge is evaluated at the estimate (:532-535);
    an unflagged one keeps the error of the optimiser's last error pass, i.e. the last LM
    trial, accepted or not.  With fewer than 10 edges only round 0 runs (:585).

    classify_at_last_trial=False reads every edge at the estimate instead (not the
    reference's behaviour; the two differ only after a rejected last trial).

    Returns (T, outlier flags, inliers, ambiguity) where ambiguity[e] is the smallest
    |chi2 / threshold - 1| the edge showed at any round's classification."""
    obs, xw, w, st = _pose_edges(edges)
    cam = tuple(float(np.float32(c)) for c in cam)   # Frame's fx .. mbf are floats
    n = len(obs)
    T0 = pose_from_float(Tcw0)
    out = np.zeros(n, bool)
    amb = np.full(n, np.inf)
    if n < 3:
        return T0, out, 0, amb
    thr = np.where(st, np.float32(CHI2_STEREO), np.float32(CHI2_MONO)).astype(np.float32)
    T = T0
    for rnd in range(4):
        T = T0
        act = ~out
        Tl = T0
        if act.any():
            lin, rc, ap = _pose_problem(obs, xw, w, st, cam, act, rnd < 3, casts, float_dsqr)
            T, rep = lm(T0, 10, lin, rc, ap)
            Tl = rep["last_trial"]
        c_est = pose_edge_terms(T, obs, xw, w, st, cam, casts)[2]
        c_last = pose_edge_terms(Tl, obs, xw, w, st, cam, casts)[2]
        c = np.where(act, c_last, c_est) if classify_at_last_trial else c_est
        amb = np.minimum(amb, np.abs(c / thr.astype(np.float64) - 1))
        out = c.astype(np.float32) > thr
        if n < 10:
            break
    return T, out, int(n - out.sum()), amb


def pose_minimiser(edges, cam, Tcw0, casts=CASTS_ONLY_POSE, float_dsqr=True, max_iter=200):
    """The same four rounds stated from the definition only: each round minimises the
    (Huber, rounds 0-2) cost over the edges not flagged before by iteratively reweighted
    Gauss-Newton from the frame's pose until the step is below 1e-13, then flags by chi2 at
    the minimiser.  No damping, no trial rules, no early stop."""
    obs, xw, w, st = _pose_edges(edges)
    cam = tuple(float(np.float32(c)) for c in cam)
    n = len(obs)
    T0 = pose_from_float(Tcw0)
    out = np.zeros(n, bool)
    if n < 3:
        return T0, out, 0
    thr = np.where(st, CHI2_STEREO, CHI2_MONO)
    T = T0
    for rnd in range(4):
        act = ~out
        T = T0
        if act.any():
            lin = _pose_problem(obs, xw, w, st, cam, act, rnd < 3, casts, float_dsqr)[0]
            for _ in range(max_iter):
                H, b, _F = lin(T)
                dx = np.linalg.lstsq(H, b, rcond=None)[0]
                T = oplus(T, dx)
                if np.abs(dx).max() < 1e-13:
                    break
        out = pose_edge_terms(T, obs, xw, w, st, cam, casts)[2] > thr
        if n < 10:
            break
    return T, out, int(n - out.sum())


def pose_chi2_sensitivity(edges, cam, T, casts=CASTS_ONLY_POSE):
    """|d chi2_e / d xi_k| at T (by the complex-step Jacobian), (n, 6): how much a pose error
    of unit size in twist component k moves edge e's chi2."""
    obs, xw, w, st = _pose_edges(edges)
    cam = tuple(float(np.float32(c)) for c in cam)
    xc, err, _ = pose_edge_terms(T, obs, xw, w, st, cam, casts)
    J = jacobian_pose(xc, cam, st)
    return np.abs(2 * w[:, None] * np.einsum("er,erk->ek", err, J))


# --------------------------------------------------------------------------- local BA
def ba_system(poses, points, edges, casts=CASTS_BA, float_dsqr=True):
    """Everything g2o holds after computeActiveErrors + buildSystem for the LBA graph:
    per edge err / chi2 / rho0 / rho1 / Jp (d err / d point) / Jt (d err / d pose twist) /
    hpl = Jp^T W Jt with W = inv_sigma2 rho' I, depth_ok (z > 0, isDepthPositive); per
    vertex H_pp = sum Jt^T W Jt, b_p = -sum Jt^T W err, H_ll, b_l by plain sums
    (base_binary_edge.hpp constructQuadraticForm).  A fixed pose gets no block and no H_pl
    (its edges still feed the point); an inactive edge (level 1) contributes nothing and its
    record is zero.  "index": the unknowns of the assembled system -- free poses and points
    with an active edge -- and H, b the dense undamped system over them, poses first."""
    P = np.asarray(poses)
    X = np.asarray(points, np.float64).reshape(-1, 3)
    E = np.asarray(edges)
    npo, npt, ne = len(P), len(X), len(E)
    R = quat_to_rot(P["q"]) if npo else np.zeros((0, 3, 3))
    t = np.asarray(P["t"], np.float64)
    ip, iq = E["pose"].astype(np.int64), E["point"].astype(np.int64)
    st = E["stereo"] != 0
    act = E["active"] != 0
    cam = (E["fx"], E["fy"], E["cx"], E["cy"], E["bf"])
    Re = R[ip]
    xc = np.einsum("eij,ej->ei", Re, X[iq]) + t[ip]
    err = residuals(E["obs"], xc, cam, st, casts)
    chi2 = chi2_of(err, E["inv_sigma2"])
    r0, r1 = huber(chi2, E["huber_delta"], float_dsqr)
    rob = E["robust"] != 0
    r0, r1 = np.where(rob, r0, chi2), np.where(rob, r1, 1.0)
    Jt = jacobian_pose(xc, cam, st)
    Jp = jacobian_point(xc, Re, cam, st)
    free = (P["fixed"] == 0)[ip] if npo else np.zeros(0, bool)
    wt = E["inv_sigma2"] * r1
    a = act[:, None]
    aa = act[:, None, None]
    err, chi2, r0, r1 = err * a, chi2 * act, r0 * act, np.where(act, r1, 0.0)
    Jt, Jp = Jt * aa, Jp * aa
    wt = wt * act
    hpl = np.einsum("e,eri,erj->eij", wt * free, Jp, Jt)
    Hpp = np.zeros((npo, 6, 6))
    bp = np.zeros((npo, 6))
    Hll = np.zeros((npt, 3, 3))
    bl = np.zeros((npt, 3))
    np.add.at(Hpp, ip, np.einsum("e,eri,erj->eij", wt * free, Jt, Jt))
    np.add.at(bp, ip, -np.einsum("e,eri,er->ei", wt * free, Jt, err))
    np.add.at(Hll, iq, np.einsum("e,eri,erj->eij", wt, Jp, Jp))
    np.add.at(bl, iq, -np.einsum("e,eri,er->ei", wt, Jp, err))
    # the unknowns and the dense system
    pose_on = np.zeros(npo, bool)
    pose_on[ip[act & free]] = True
    point_on = np.zeros(npt, bool)
    point_on[iq[act]] = True
    pidx, qidx = np.flatnonzero(pose_on), np.flatnonzero(point_on)
    pmap = -np.ones(npo, np.int64)
    pmap[pidx] = np.arange(len(pidx))
    qmap = -np.ones(npt, np.int64)
    qmap[qidx] = np.arange(len(qidx))
    n6 = 6 * len(pidx)
    N = n6 + 3 * len(qidx)
    H = np.zeros((N, N))
    b = np.zeros(N)
    for k, i in enumerate(pidx):
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = Hpp[i]
        b[6 * k:6 * k + 6] = bp[i]
    for k, j in enumerate(qidx):
        H[n6 + 3 * k:n6 + 3 * k + 3, n6 + 3 * k:n6 + 3 * k + 3] = Hll[j]
        b[n6 + 3 * k:n6 + 3 * k + 3] = bl[j]
    for e in np.flatnonzero(act & free):
        r, c = n6 + 3 * qmap[iq[e]], 6 * pmap[ip[e]]
        H[r:r + 3, c:c + 6] += hpl[e]
        H[c:c + 6, r:r + 3] += hpl[e].T
    return dict(err=err, chi2=chi2, rho0=r0, rho1=r1, jp=Jp, jt=Jt, hpl=hpl, depth_ok=xc[:, 2] > 0,
                hpose=Hpp, bpose=bp, hpoint=Hll, bpoint=bl, H=H, b=b, pose_index=pidx,
                point_index=qidx, npose=npo, npoint=npt, robust_chi2=float(np.sum(r0)))


def ba_scatter(system, x):
    """The solution vector of the assembled system as (dx_pose (npose, 6), dx_point
    (npoint, 3)), zero for vertices that are not unknowns."""
    dp = np.zeros((system["npose"], 6))
    dq = np.zeros((system["npoint"], 3))
    n6 = 6 * len(system["pose_index"])
    dp[system["pose_index"]] = x[:n6].reshape(-1, 6)
    dq[system["point_index"]] = x[n6:].reshape(-1, 3)
    return dp, dq


def ba_solve_dense(system, lam):
    """One solve of the full [[H_pp, H_pl^T], [H_pl, H_ll]] + lam I (setLambda adds lam to
    every diagonal entry of both block families, block_solver.hpp).  Returns (ok, dx_pose,
    dx_point)."""
    x, ok = _solve_damped(system["H"], system["b"], lam)
    return (ok,) + ba_scatter(system, x)


def ba_apply(poses, points, dx_pose, dx_point, first_order_below=1e-5):
    """SparseOptimizer::update: exp(dx) * T per free pose, += per point.  Returns copies."""
    P = np.array(poses)
    X = np.array(points, np.float64).reshape(-1, 3) + np.asarray(dx_point).reshape(-1, 3)
    for i in np.flatnonzero(P["fixed"] == 0):
        T = oplus(pose_matrix(P["q"][i], P["t"][i]), dx_pose[i], first_order_below)
        P["q"][i] = rot_to_quat(T[:3, :3])
        P["t"][i] = T[:3, 3]
    return P, X


def ba_optimize(poses, points, edges, iterations, casts=CASTS_BA, float_dsqr=True):
    """optimizer.optimize(iterations) on the LBA graph (Optimizer.cc:857, :905): `lm` over
    ba_system / ba_solve_dense / ba_apply.  Returns (poses, points, report)."""
    def linearize(s):
        sy = ba_system(s[0], s[1], edges, casts, float_dsqr)
        linearize.last = sy
        return sy["H"], sy["b"], sy["robust_chi2"]

    def rchi2(s):
        return ba_system_chi2(s[0], s[1], edges, casts, float_dsqr)

    def apply(s, x):
        return ba_apply(s[0], s[1], *ba_scatter(linearize.last, x))

    (P, X), rep = lm((np.array(poses), np.array(points, np.float64).reshape(-1, 3)), iterations,
                     linearize, rchi2, apply)
    return P, X, rep


def ba_system_chi2(poses, points, edges, casts=CASTS_BA, float_dsqr=True):
    """activeRobustChi2 alone (sparse_optimizer.cpp:100-114)."""
    P, E = np.asarray(poses), np.asarray(edges)
    X = np.asarray(points, np.float64).reshape(-1, 3)
    ip, iq = E["pose"].astype(np.int64), E["point"].astype(np.int64)
    xc = np.einsum("eij,ej->ei", quat_to_rot(P["q"])[ip], X[iq]) + P["t"][ip]
    st = E["stereo"] != 0
    c = chi2_of(residuals(E["obs"], xc, (E["fx"], E["fy"], E["cx"], E["cy"], E["bf"]), st, casts),
                E["inv_sigma2"])
    r0 = np.where(E["robust"] != 0, huber(c, E["huber_delta"], float_dsqr)[0], c)
    return float(np.sum(r0[E["active"] != 0]))


# --------------------------------------------------------------------------- comparison rules
def rel(a, b):
    """max |a - b| over max |b|: the array-scaled relative difference of test_gpu_ba.py."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def stereo_cast_bound(proj, cam):
    """Bound on |err(casts) - err(casts=None)| of a stereo edge, per component: the float invz
    carries a relative error of eps32 / 2, which multiplies u - cx, v - cy and bf / z; the
    float bf and the float product of CASTS_BA add eps32 / 2 each on bf / z.  We allow
    eps32 of each magnitude (twice the half-ulp) and the sum of the three on bf / z."""
    fx, fy, cx, cy, bf = _cam(cam)
    du = np.abs(proj[..., 0] - cx)
    dv = np.abs(proj[..., 1] - cy)
    d = np.abs(proj[..., 0] - proj[..., 2])     # bf / z
    return EPS32 * np.stack([du, dv, du + 3 * d], -1)


def ba_tolerances(poses, points, edges, sy):
    """Derived bounds for an implementation that applies the same casts as `sy` =
    ba_system(...) did, against it.

    Everything hangs on xc = R x + t.  R comes from the quaternion (each entry rounds ~4
    times) and the three-term dot products round ~3 times per term, so each side carries up
    to ~10 eps64 (|R x| + |t|) on xc; two sides, rounded up: 32 eps64 mag.  Relative to the
    depth that is base_e = 32 eps64 (1 + mag_e / |z_e|), the relative error of 1/z (twice
    that for 1/z^2), which enters every output of edge e:
      err    absolute: d_err = base_e (|obs|_max + |proj|_max)
      chi2   d_chi2 = 2 inv_sigma2 |err|_1 d_err + 8 eps64 chi2      (rho the same)
      rho'   d_chi2 / (2 chi2) + 8 eps64      (relative; the Huber branch is continuous)
      jp jt  2 base_e max|J_e|                                   (absolute, per edge)
      hpl    q_e max|Jp_e| max|Jt_e| w_e, q_e = 4 base_e + d_rho'_e   (absolute, per edge)
    and the vertex blocks by summing their edges' bounds, plus n eps64 sum|term| for the
    summation itself (n edges in any order):
      H_pp H_ll   sum_e (q_e + n eps64) max|J_e|^2 w_e
      b_p b_l     sum_e ((q_e + n eps64) |err|_max + d_err) max|J_e| w_e."""
    P, E = np.asarray(poses), np.asarray(edges)
    X = np.asarray(points, np.float64).reshape(-1, 3)
    ip, iq = E["pose"].astype(np.int64), E["point"].astype(np.int64)
    cam = (E["fx"], E["fy"], E["cx"], E["cy"], E["bf"])
    act = E["active"] != 0
    Re = quat_to_rot(P["q"])[ip]
    rx = np.einsum("eij,ej->ei", Re, X[iq])
    xc = rx + P["t"][ip]
    mag = np.linalg.norm(rx, axis=1) + np.linalg.norm(P["t"][ip], axis=1)
    base = 32 * EPS64 * (1 + mag / np.abs(xc[:, 2]))
    proj = project(xc, cam, E["stereo"] != 0)
    d_err = base * (np.abs(E["obs"]).max(1) + np.abs(proj).max(1))
    err = residuals(E["obs"], xc, cam, E["stereo"] != 0, CASTS_BA)
    chi2 = chi2_of(err, E["inv_sigma2"])
    d_chi2 = 2 * E["inv_sigma2"] * np.abs(err).sum(1) * d_err + 8 * EPS64 * chi2
    d_rho1 = d_chi2 / (2 * np.maximum(chi2, 1e-300)) + 8 * EPS64
    jpm = np.abs(sy["jp"]).max((1, 2))
    jtm = np.abs(sy["jt"]).max((1, 2))
    w = E["inv_sigma2"] * sy["rho1"]
    q = 4 * base + d_rho1
    em = np.abs(sy["err"]).max(1)
    free = (P["fixed"] == 0)[ip]
    npo, npt = len(P), len(X)
    cnt_p = np.bincount(ip[act], minlength=npo)
    cnt_q = np.bincount(iq[act], minlength=npt)

    def vsum(idx, n, term, mask):
        out = np.zeros(n)
        np.add.at(out, idx[mask], term[mask])
        return out

    qp, qq = q + cnt_p[ip] * EPS64, q + cnt_q[iq] * EPS64
    return dict(err=d_err[:, None], chi2=d_chi2, rho0=d_chi2, rho1=d_rho1 * sy["rho1"],
                jp=(2 * base * jpm)[:, None, None], jt=(2 * base * jtm)[:, None, None],
                hpl=(q * jpm * jtm * w)[:, None, None],
                hpose=vsum(ip, npo, 9 * qp * jtm * jtm * w, act & free)[:, None, None],
                bpose=vsum(ip, npo, 3 * (qp * em + d_err) * jtm * w, act & free)[:, None],
                hpoint=vsum(iq, npt, 9 * qq * jpm * jpm * w, act)[:, None, None],
                bpoint=vsum(iq, npt, 3 * (qq * em + d_err) * jpm * w, act)[:, None])


BA_OUTPUTS = ("err", "chi2", "rho1", "jp", "jt", "hpl", "hpose", "bpose", "hpoint", "bpoint")


def ba_compare(got, sy, tol, what=BA_OUTPUTS, rows=None):
    """difference / bound, the maximum per output (<= 1 passes), of an implementation's
    outputs `got` (arrays named as ba_system's) against sy under ba_tolerances' bounds; where
    the bound is 0 (an empty vertex, an inactive edge) the output must be exactly the
    reference's 0.  rows: restrict the per-edge outputs to these edges."""
    fig = {}
    for k in what:
        r = sy[k]
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        d = np.abs(g - r)
        t = np.broadcast_to(tol[k], r.shape)
        if rows is not None and len(r) == len(sy["chi2"]) and k not in ("hpose", "bpose",
                                                                        "hpoint", "bpoint"):
            d, t = d[rows], t[rows]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(t > 0, d / t, np.where(d == 0, 0.0, np.inf))
        fig[k] = float(ratio.max()) if ratio.size else 0.0
    return fig


def schur_tolerance(sy, lam):
    """The device's block elimination and one dense solve of the same symmetric positive
    definite system differ by the backward error of a Cholesky-type factorisation carried to
    the solution: n eps64 cond(H + lam I), relative to max|dx| (Higham, Accuracy and
    Stability of Numerical Algorithms, thm 10.4 with its constant taken as 1), n the number of
    unknowns.  The blocks fed to the device are the reference's own, so nothing else differs."""
    n = len(sy["b"])
    return n * EPS64 * float(np.linalg.cond(sy["H"] + lam * np.eye(n))) if n else 0.0


def update_bounds(poses, dx_pose):
    """Per pose, the bounds of the update test.  Against oplus with the reference's
    first-order branch: a 3x3 product, V upsilon, a quaternion extraction and a
    normalisation, each a few roundings: 64 eps64 on R, 64 eps64 (1 + |t| + |upsilon|) on t.
    Against the pure expm the first-order branch itself errs (|omega| = th < 1e-5): R by
    th^2 / 2 (W^2 instead of W^2 / 2), V by th / 2 (W instead of W / 2), so t by
    th^2 |t| / 2 + th |upsilon|; both doubled here for the higher-order terms."""
    t = np.linalg.norm(poses["t"], axis=1)
    th = np.linalg.norm(dx_pose[:, :3], axis=1)
    ups = np.linalg.norm(dx_pose[:, 3:], axis=1)
    tight = (np.full(len(t), 64 * EPS64), 64 * EPS64 * (1 + t + ups))
    small = th < 1e-5
    pure = (tight[0] + np.where(small, th * th, 0.0),
            tight[1] + np.where(small, th * th * t + 2 * th * ups, 0.0))
    return tight, pure


# Measured tolerances: where no bound can be derived (poses, chi2 and estimates after up to 40
# LM iterations) the constant is 4 x the larger of two maxima over the cases the tests use:
# the CPU oracle against this file, and the MI355X kernels against this file.  Rounding carried
# through the iterations varies that much between seeds.  Never GPU against oracle.
#
# PoseOptimization against pose_optimization (same LM rules), POSE_CASES and POSE_BATCH_CASES:
#   translation (m): CPU oracle 2.13e-10, MI355X 2.13e-10; rot_dist: CPU 8.2e-13, MI355X 8.2e-13
TOL_POSE_T = 4 * 2.2e-10
TOL_POSE_R = 4 * 8.2e-13
# PoseOptimization against pose_minimiser (no LM rules), on POSE_MIN_CASES, the cases where
# this file's own LM and minimiser agree to a quarter of the constant (asserted in
# test_optim_ref.py; g2o stops after three iterations that improve chi2 by < 0.1 %, short of
# the minimum):
#   translation: this file's LM vs its minimiser 2.36e-7, CPU oracle 2.36e-7, MI355X 2.36e-7;
#   rot_dist: 2.38e-9, 2.38e-9, 2.38e-9
TOL_POSE_MIN_T = 4 * 2.4e-7
TOL_POSE_MIN_R = 4 * 2.4e-9
# Flag ambiguity margin: the relative chi2 change the tight pose tolerance can cause, the
# maximum over the cases and their edges of
#   sum_k |d chi2_e / d xi_k| tol_k / threshold_e,  tol = TOL_POSE_R (omega), TOL_POSE_T (upsilon)
# over the edges whose chi2 is within 50 % of its threshold (the others cannot flip)
# (pose_chi2_sensitivity; test_optim_ref.py recomputes it -- 1.7e-7 -- and asserts it stays
# below this rounded-up value).  No edge of any case lies within it in the reference.
FLAG_MARGIN = 1e-6
# DeviceLBA.optimize against ba_optimize on LM_CASES and the LBA sequence.  Relative initial
# chi2: CPU 4.3e-14, MI355X 4.2e-14.  Relative final chi2: CPU 4.6e-10, MI355X 8.7e-8 -- both
# from the sequence's non-robust optimize(10); the float invz makes a stereo residual a step
# function of depth (steps of eps32 |u|, ~4e-5 px), so estimates that agree to 2e-11 still
# land some edges on different steps; the robust cases stay below 1.5e-12 on both.  Estimates
# (points and t relative to the array maximum, q absolute): CPU 1.7e-11, MI355X 1.8e-11.
TOL_LM_CHI2_INITIAL = 4 * 4.3e-14
TOL_LM_CHI2 = 4 * 8.7e-8
TOL_LM_EST = 4 * 1.8e-11
# An LM decision is "clear" when |rho| and the distance of the relative improvement from the
# 0.1 % stop rule stay this far from zero while the step is still above 1e-6.
LM_CLEAR = 1e-6


# --------------------------------------------------------------------------- scenes
# (n, seed, stereo fraction, outlier fraction): the edge counts at which a 256-thread strided
# pass with four waves can go wrong, the three stereo mixes, outliers 5 .. 40 %.  On these
# seeds, in this file alone, at most max(1, 1 % of n) edges lie within FLAG_MARGIN of a
# threshold (test_optim_ref.py asserts it; in fact none does).
POSE_CASES = [(3, 1, 0.5, 0.05), (9, 2, 1.0, 0.1), (10, 3, 0.0, 0.1), (63, 4, 0.5, 0.2),
              (64, 5, 1.0, 0.05), (65, 6, 0.0, 0.3), (255, 7, 0.5, 0.4), (256, 8, 1.0, 0.2),
              (257, 9, 0.0, 0.05), (513, 10, 0.5, 0.3)]


def pose_scene(n, seed, stereo_frac, outlier_frac):
    from orb_slam2_test_amd import synthetic as S
    return S.pose_frame(n=n, seed=seed, stereo_frac=stereo_frac, outlier_frac=outlier_frac)


def pose_figures(got, ref):
    """got = (q, t, outlier, ninliers) of an implementation, ref = pose_optimization's result
    (or pose_minimiser's, which has no ambiguity: every edge counts).  Returns (|dt| max,
    rot_dist, mismatching flags among edges outside FLAG_MARGIN, edges inside it,
    ninliers == number of unflagged edges)."""
    q, t, out, ni = got
    T, rout = ref[0], ref[1]
    amb = ref[3] if len(ref) > 3 else np.full(len(rout), np.inf)
    clear = amb > FLAG_MARGIN
    return (float(np.abs(np.asarray(t) - T[:3, 3]).max()),
            rot_dist(quat_to_rot(np.asarray(q)), T[:3, :3]),
            int((np.asarray(out, bool) != rout)[clear].sum()), int((~clear).sum()),
            int(ni) == int(len(rout) - np.asarray(out, bool).sum()) if len(rout) >= 3 else ni == 0)


def _prune(edges, counts):
    """Delete the last edges of each pose in `counts` until it has exactly that many."""
    keep = np.ones(len(edges), bool)
    for p, c in counts.items():
        idx = np.flatnonzero(edges["pose"] == p)
        assert len(idx) >= c, (p, len(idx), c)
        keep[idx[c:]] = False
    return edges[keep]


def ba_shaped_window(seed=300, n_points=400, stereo_frac=0.6, robust=True):
    """A small LBA window (4 free + 3 fixed poses) shaped to hit the kernels' structure:
    free poses with exactly 63 / 64 / 65 / 129 edges (the pose slices hold 64), a point whose
    edges straddle edge 256 (edges are in point order), a free pose and a point with no edge,
    a point 0.6 m in front of its camera (the float invz matters most) and one behind its
    camera (depth_ok false).  Observations stay float-exact."""
    from orb_slam2_test_amd import synthetic as S
    poses, pts, edges = S.ba_window(n_local=4, n_fixed=3, n_points=n_points, seed=seed,
                                    stereo_frac=stereo_frac, robust=robust)
    edges = _prune(edges, {0: 63, 1: 64, 2: 65, 3: 129})
    while edges["point"][255] != edges["point"][256]:
        k = np.flatnonzero(edges["pose"][:255] >= 4)[-1]   # drop a fixed pose's edge before it
        edges = np.delete(edges, k)
    R = quat_to_rot(poses["q"])
    extra_pts, extra_edges = [], []
    for pose, depth, stereos in ((4, 0.6, (1, 0)), (5, -2.0, (1, 0))):
        xc = np.array([0.11 * depth, -0.07 * depth, depth])
        extra_pts.append(R[pose].T @ (xc - poses["t"][pose]))
        for s in stereos:
            e = edges[0].copy()
            e["point"] = len(pts) + len(extra_pts) - 1
            e["pose"] = pose
            e["stereo"] = s
            u = S.KITTI_FX * 0.11 + S.KITTI_CX + 0.7
            v = S.KITTI_FY * -0.07 + S.KITTI_CY - 0.4
            e["obs"] = [float(np.float32(u)), float(np.float32(v)),
                        float(np.float32(u - S.KITTI_BF / depth + 0.5)) if s else 0.0]
            e["huber_delta"] = DELTA_STEREO if s else DELTA_MONO
            e["inv_sigma2"] = 1.0
            extra_edges.append(e)
    pts = np.concatenate([pts, np.array(extra_pts), pts[:1] + 1.0])      # + a point with no edge
    edges = np.concatenate([edges, np.array(extra_edges, dtype=edges.dtype)])
    lone = poses[:1].copy()
    lone["fixed"] = 0
    poses = np.concatenate([poses, lone])                               # + a pose with no edge
    return poses, pts, edges


def ba_concat(ws):
    """Independent windows as one graph (vertex indices offset per window)."""
    poses, pts, edges = [], [], []
    po = qo = 0
    for p, q, e in ws:
        e = e.copy()
        e["pose"] += po
        e["point"] += qo
        poses.append(p)
        pts.append(q)
        edges.append(e)
        po += len(p)
        qo += len(q)
    return np.concatenate(poses), np.concatenate(pts), np.concatenate(edges)


def ba_two_cameras(seed=320, n_points=60):
    """Two windows with different calibrations, per-edge information and Huber deltas off the
    octave table, in one graph."""
    from orb_slam2_test_amd import synthetic as S
    ws = [S.ba_window(n_local=4, n_fixed=3, n_points=n_points, seed=seed + i) for i in range(2)]
    ws[1][2]["fx"] += 3.0
    ws[1][2]["cy"] -= 1.5
    ws[1][2]["bf"] *= 1.1
    poses, pts, edges = ba_concat(ws)
    edges["inv_sigma2"][::13] *= 0.5
    edges["huber_delta"][::17] = 2.0
    return poses, pts, edges


def ba_perturbed(seed, n_points, s_pose=2e-3, s_point=5e-2, **kw):
    """A window (4 free + 3 fixed poses) with its free poses and points moved off the truth."""
    from orb_slam2_test_amd import synthetic as S
    poses, pts, edges = S.ba_window(n_local=4, n_fixed=3, n_points=n_points, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    poses = poses.copy()
    free = poses["fixed"] == 0
    poses["t"][free] += rng.normal(0, s_pose, (int(free.sum()), 3))
    return poses, pts + rng.normal(0, s_point, pts.shape), edges


# (seed, points, iterations, pose sigma, point sigma): windows of <= 150 points; the last one
# starts far enough off that the LM rejects trials.
LM_CASES = [(70, 60, 5, 2e-3, 5e-2), (71, 120, 10, 2e-3, 5e-2), (73, 100, 10, 2e-3, 5e-2),
            (47, 150, 10, 2e-2, 0.5)]


def update_twists(npose, seed=5):
    """Increments for the update test: |omega| from 1e-7 across SE3Quat::exp's 1e-5 branch
    switch (just below, just above) up to 3.1 rad, with translations up to 100 m."""
    rng = np.random.default_rng(seed)
    mags = [1e-7, 9.999e-6, 1.0001e-5, 1e-3, 0.5, 3.1, 0.0, 2.0]
    dx = np.zeros((npose, 6))
    for i in range(npose):
        a = rng.normal(size=3)
        dx[i, :3] = a / np.linalg.norm(a) * mags[i % len(mags)]
        dx[i, 3:] = rng.normal(0, 1.0, 3) * (100.0 if i % 3 == 0 else 0.1)
    return dx


# --------------------------------------------------------------------------- shared checks
# Both test modules run these, test_optim_ref.py on the CPU oracle and test_gpu_optim_ref.py on
# the kernels.  `impl` supplies the implementation under test:
#   impl.pose(edges, cam, Tcw0)                -> (q, t, outlier, ninliers)
#   impl.linearize(poses, points, edges)       -> dict of the BA_OUTPUTS it produces
#   impl.errors(poses, points, edges)          -> (err, chi2, rho0, depth_ok, robust chi2 sum),
#                                                 None for what the path does not produce
#   impl.schur(poses, npoint, edges, sy, lam)  -> (ok, dx_pose, dx_point), fed sy's blocks
#   impl.update(poses, points, dxp, dxq)       -> (poses, points)
#   impl.optimize(poses, points, edges, iters, active=None, robust=None)
#                                              -> (poses, points, report)
# Every check prints its figures before it asserts, so a run with -s is also a measurement.
CAM = (718.856, 718.856, 607.1928, 185.2157, 386.1448)     # synthetic.KITTI_*


def check_pose(impl, edges, T0, ref=None, ref_min=None, name=""):
    """The implementation's pose within TOL_POSE_* of pose_optimization, every flag outside
    FLAG_MARGIN equal, ninliers consistent with the flags; with ref_min also within
    TOL_POSE_MIN_* of pose_minimiser."""
    ref = pose_optimization(edges, CAM, T0) if ref is None else ref
    got = impl.pose(edges, CAM, T0)
    dt, dr, bad, namb, consistent = pose_figures(got, ref)
    print("pose %s n=%d: dt %.3g dR %.3g flags differing %d (ambiguous %d)"
          % (name, len(edges), dt, dr, bad, namb))
    assert consistent
    assert got[3] == ref[2] or namb > 0
    assert bad == 0
    assert dt <= TOL_POSE_T and dr <= TOL_POSE_R
    if ref_min is not None:
        mt, mr, mbad, _, _ = pose_figures(got, ref_min)
        print("pose %s vs minimiser: dt %.3g dR %.3g flags differing %d" % (name, mt, mr, mbad))
        assert mt <= TOL_POSE_MIN_T and mr <= TOL_POSE_MIN_R
    return dt, dr


def check_linearize(impl, poses, pts, edges, what=BA_OUTPUTS, name=""):
    sy = ba_system(poses, pts, edges)
    tol = ba_tolerances(poses, pts, edges, sy)
    got = impl.linearize(poses, pts, edges)
    fig = ba_compare(got, sy, tol, [k for k in what if k in got])
    print("linearize %s (%d edges), difference / bound: %s"
          % (name, len(edges), " ".join("%s %.2g" % kv for kv in fig.items())))
    assert fig and all(v <= 1 for v in fig.values()), fig
    return sy, got


def check_errors(impl, poses, pts, edges, name=""):
    """The per-trial error pass computes every edge (the LM reads the active ones): err,
    chi2, rho, depth_ok against the reference with every edge switched on, the sum against
    the active robust chi2."""
    on = np.array(edges)
    on["active"] = 1
    sy = ba_system(poses, pts, on)
    tol = ba_tolerances(poses, pts, on, sy)
    err, chi2, rho0, dok, tot = impl.errors(poses, pts, edges)
    act = edges["active"] != 0
    got = {k: v for k, v in (("err", err), ("chi2", chi2), ("rho0", rho0)) if v is not None}
    fig = ba_compare(got, sy, tol, tuple(got), rows=act)
    print("errors %s, difference / bound: %s"
          % (name, " ".join("%s %.2g" % kv for kv in fig.items())))
    assert fig and all(v <= 1 for v in fig.values()), fig
    if dok is not None:
        assert np.array_equal(np.asarray(dok, bool)[act], sy["depth_ok"][act])
    if tot is not None:
        want = float(np.sum(sy["rho0"][act]))
        dsum = abs(tot - want) / max(want, 1e-300)
        bsum = float(np.sum(tol["rho0"][act])) / max(want, 1e-300) + len(edges) * EPS64
        print("errors %s: sum %.2g (bound %.2g)" % (name, dsum, bsum))
        assert dsum <= bsum


def check_schur(impl, poses, pts, edges, lam_scale, name=""):
    sy = ba_system(poses, pts, edges)
    diag = np.abs(sy["hpose"].reshape(len(poses), 36)[:, ::7]).max() if len(sy["pose_index"]) \
        else np.abs(sy["hpoint"].reshape(-1, 9)[:, ::4]).max()
    lam = lam_scale * float(diag)
    rok, rdp, rdq = ba_solve_dense(sy, lam)
    ok, dp, dq = impl.schur(poses, len(pts), edges, sy, lam)
    tol = schur_tolerance(sy, lam)
    scale = max(np.abs(rdp).max(), np.abs(rdq).max())
    fp = float(np.abs(np.asarray(dp).reshape(rdp.shape) - rdp).max() / scale)
    fq = float(np.abs(np.asarray(dq).reshape(rdq.shape) - rdq).max() / scale)
    print("schur %s lam %.3g: pose %.3g point %.3g bound %.3g" % (name, lam, fp, fq, tol))
    assert rok and ok
    assert fp <= tol and fq <= tol
    return sy


def check_update(impl, poses, pts, dxp, dxq, name=""):
    """Against oplus with the reference's first-order branch (tight) and against the pure
    expm (its own bound); fixed poses untouched; points += dx exactly; quaternions unit."""
    gp, gq = impl.update(poses, pts, dxp, dxq)
    fixed = poses["fixed"] != 0
    assert fixed.any() and gp[fixed].tobytes() == np.asarray(poses)[fixed].tobytes()
    assert np.array_equal(gq, np.asarray(pts) + dxq)
    (tr, tt), (pr, pt) = update_bounds(poses, dxp)
    worst = np.zeros(4)
    for i in np.flatnonzero(~fixed):
        T0 = pose_matrix(poses["q"][i], poses["t"][i])
        G = pose_matrix(gp["q"][i], gp["t"][i])
        for j, (T, br, bt) in enumerate(((oplus(T0, dxp[i], 1e-5), tr[i], tt[i]),
                                         (oplus(T0, dxp[i]), pr[i], pt[i]))):
            fr = rot_dist(G[:3, :3], T[:3, :3]) / br
            ft = np.abs(G[:3, 3] - T[:3, 3]).max() / bt
            worst[2 * j:2 * j + 2] = np.maximum(worst[2 * j:2 * j + 2], (fr, ft))
            assert fr <= 1 and ft <= 1, (i, j, fr, ft, dxp[i])
    qn = np.abs(np.linalg.norm(gp["q"], axis=1) - 1).max()
    print("update %s difference / bound: g2o branch R %.2g t %.2g, expm R %.2g t %.2g; "
          "| |q| - 1 | %.2g" % ((name,) + tuple(worst) + (qn,)))
    assert qn <= 1e-15
    return gp, gq


def check_optimize(impl, poses, pts, edges, iters, active=None, robust=None, name="",
                   clear=True):
    e2 = np.array(edges)
    if active is not None:
        e2["active"] = active
    if robust is not None:
        e2["robust"] = robust
    rp, rq, rrep = ba_optimize(poses, pts, e2, iters)
    gp, gq, rep = impl.optimize(poses, pts, edges, iters, active=active, robust=robust)
    fi = abs(rep["initial_chi2"] - rrep["initial_chi2"]) / rrep["initial_chi2"]
    ff = abs(rep["final_chi2"] - rrep["final_chi2"]) / rrep["final_chi2"]
    sgn = np.where(np.sum(gp["q"] * rp["q"], 1) < 0, -1.0, 1.0)[:, None]   # q and -q: one rotation
    fe = max(rel(gq, rq), rel(gp["t"], rp["t"]), float(np.abs(sgn * gp["q"] - rp["q"]).max()))
    print("optimize %s (%d): %d it / %d trials (ref %d / %d, terminated %d / %d); chi2 initial "
          "%.3g final %.3g; estimates %.3g; min |rho| %.3g stop margin %.3g"
          % (name, iters, rep["iterations"], rep["trials"], rrep["iterations"], rrep["trials"],
             rep["terminated"], rrep["terminated"], fi, ff, fe, rrep["min_abs_rho"],
             rrep["min_stop_margin"]))
    if clear:   # every decision is clear in the reference: the same path is required
        assert min(rrep["min_abs_rho"], rrep["min_stop_margin"]) > LM_CLEAR
        for k in ("iterations", "trials", "terminated"):
            assert rep[k] == rrep[k], (k, rep, rrep)
    assert fi <= TOL_LM_CHI2_INITIAL and ff <= TOL_LM_CHI2 and fe <= TOL_LM_EST
    fx = poses["fixed"] != 0
    assert gp[fx].tobytes() == np.asarray(poses)[fx].tobytes()
    return (gp, gq, rep), (rp, rq, rrep)


def lba_outlier_pass(poses, pts, edges):
    """Optimizer.cc:871-901 in the reference's terms: after optimize(5), an edge stays on
    when its chi2 is at most 5.991 / 7.815 and its depth is positive; the robust kernels are
    dropped.  Returns (active, margin): margin is the smallest |chi2 / thr - 1|."""
    sy = ba_system(poses, pts, edges)
    thr = np.where(edges["stereo"] != 0, CHI2_STEREO, CHI2_MONO)
    on = edges["active"] != 0
    active = ((sy["chi2"] <= thr) & sy["depth_ok"] & on).astype(np.uint8)
    return active, float(np.abs(sy["chi2"][on] / thr[on] - 1).min())


def check_lba_sequence(impl):
    """optimize(5), the outlier pass, optimize(10) without robust kernels, on two windows in
    one graph.  The second call starts from the reference's estimates and active set, so
    the two calls are checked independently."""
    poses, pts, edges = ba_concat([ba_perturbed(75, 100), ba_perturbed(76, 140)])
    _, (rp, rq, _) = check_optimize(impl, poses, pts, edges, 5, name="lba 5")
    active, margin = lba_outlier_pass(rp, rq, edges)
    print("outlier pass: %d of %d edges stay, nearest to a threshold %.3g"
          % (int(active.sum()), len(edges), margin))
    assert 0 < active.sum() < len(edges)
    (gp, gq, rep), _ = check_optimize(impl, rp, rq, edges, 10, active=active,
                                      robust=np.zeros(len(edges), np.uint8), name="lba 10")
    assert rep["iterations"] >= 1


def _plain(**kw):
    from orb_slam2_test_amd import synthetic as S
    return S.ba_window(n_local=4, n_fixed=3, n_points=60, **kw)


def _third_inactive():
    poses, pts, edges = ba_shaped_window()
    edges["active"][::3] = 0
    return poses, pts, edges


BA_SCENES = {
    "shaped": ba_shaped_window,
    "mono": lambda: _plain(seed=302, stereo_frac=0.0),
    "stereo": lambda: _plain(seed=303, stereo_frac=1.0),
    "non_robust": lambda: _plain(seed=304, robust=False),
    "third_inactive": _third_inactive,
    "two_cameras": ba_two_cameras,
}

# The batched entry: counts mixed below the capacity, 0 and 2 among them.
POSE_BATCH_CASES = [(0, 20, 0.5, 0.1), (2, 21, 0.5, 0.1), (40, 22, 0.3, 0.1), (300, 23, 1.0, 0.2),
                    (7, 24, 0.0, 0.1)]
# The cases on which this file's LM and its from-definition minimiser agree to
# TOL_POSE_MIN_* / 4 (g2o's three-small-improvements stop leaves the others short of the
# minimum); test_optim_ref.py asserts it.
POSE_MIN_CASES = [c for c in POSE_CASES if c[0] >= 63]
