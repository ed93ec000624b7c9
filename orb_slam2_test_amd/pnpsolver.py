"""PnPsolver -- ORB-SLAM2's RANSAC over EPnP (include/PnPsolver.h, src/PnPsolver.cc;
Tracking::Relocalization, Tracking.cc:1958-2180), evaluated on the device behind liborbg's
orbg_pnp_* entry points.

The caller compacts the correspondences the way the constructor does (:79-101): world
positions of the matched MapPoints, the undistorted keypoints, mvLevelSigma2 of their octaves
and index = the slot in vpMapPointMatches.  Every RANSAC iteration (and Refine() at every
record iteration) is evaluated once, in one launch; iterate() then serves its windows from the
downloaded records by the reference's sequential rule, so iterate(5) can be called again and
again as Tracking does, after a hit too.

    solver = PnPsolver(K, Xw, uv, sigma2, index, n1)
    solver.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    Tcw, bNoMore, vbInliers, nInliers = solver.iterate(5)

The reference's loop runs while `mnIterations < mRansacMaxIts || nCurrentIterations <
nIterations`: an OR, so the first iterate(5) already runs to mRansacMaxIts unless it hits, and
a later call runs its nIterations more.  iterate() here does the same over the evaluated
iterations and reports bNoMore once they are used up.

The random draws are the reference's (DUtils::Random::RandomInt on rand(), with the
swap-remove of PnPsolver.cc:191-201) applied to a stream of 31-bit integers: `stream`, or a
NumPy generator seeded with `seed` (the integer stream of Sim3Solver).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .orbmatcher import _ctx
from .sim3solver import _rand_stream, _intrinsics, mask_bits  # noqa: F401

MAX_N = 8192   # correspondences per candidate (ORBG_ENOTSUP past it)
MAX_SET = L.PNP_MAX_SET


def draw_samples(n, its, min_set, stream):
    """The min_set distinct correspondence indices of `its` iterations over `n` correspondences
    (int32 [its][min_set]).  `stream` yields what rand() would: integers in [0, 2^31).  Per
    draw (PnPsolver.cc:191-201, Random.cpp:47-50): randi = int(r / 2^31 * m) over the m indices
    still available, the chosen one is replaced by the back and the back is popped."""
    out = np.zeros((int(its), int(min_set)), np.int32)
    if n < min_set:
        return out
    it = iter(stream)
    base = list(range(int(n)))
    for k in range(int(its)):
        avail = base.copy()
        for j in range(int(min_set)):
            r = int(next(it))
            if not 0 <= r < 2147483648:
                raise ValueError("the stream must yield integers in [0, 2^31)")
            randi = int(r / 2147483648.0 * len(avail))
            out[k, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def make_problem(K, n, min_set, min_inliers, iterations, th2=5.991):
    """One orbg_pnp_problem record (PNP_PROBLEM_DTYPE array of shape (1,)); min_inliers and
    iterations as ransac_parameters adjusted them."""
    p = np.zeros(1, L.PNP_PROBLEM_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = _intrinsics(K)
    p["n"], p["min_set"] = int(n), int(min_set)
    p["min_inliers"], p["iterations"] = int(min_inliers), int(iterations)
    p["th2"] = np.float32(th2)
    return p


def make_corrs(Xw, uv, sigma2, index):
    """orbg_pnp_corr records (PNP_CORR_DTYPE [n]) from the per-correspondence arrays."""
    Xw = np.asarray(Xw, np.float32).reshape(-1, 3)
    n = len(Xw)
    c = np.zeros(n, L.PNP_CORR_DTYPE)
    c["Xw"] = Xw
    c["uv"] = np.asarray(uv, np.float32).reshape(n, 2)
    c["sigma2"] = np.asarray(sigma2, np.float32).reshape(n)
    c["index"] = np.asarray(index, np.int32).reshape(n)
    return c


def ransac_parameters(prob, min_inliers, max_its, min_set, epsilon, n):
    """(mRansacMinInliers, mRansacMaxIts) of SetRansacParameters (:121-152) for n
    correspondences (host only)."""
    mi, its = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().orbg_pnp_ransac_parameters(float(prob), int(min_inliers), int(max_its),
                                               int(min_set), float(epsilon), int(n),
                                               C.byref(mi), C.byref(its)),
            "orbg_pnp_ransac_parameters")
    return int(mi.value), int(its.value)


def solve(problem, corrs, samples, n1, ctx=None, device=0):
    """orbg_pnp_solve on one candidate's host records.  Returns a dict: counts [its], hyps
    [its], masks uint64 [its][ceil(n / 64)], refines [its], refined_masks (as masks), result
    (a PNP_RESULT_DTYPE record) and inliers uint8 [n1]."""
    problem = np.ascontiguousarray(problem, L.PNP_PROBLEM_DTYPE).reshape(1)
    corrs = np.ascontiguousarray(corrs, L.PNP_CORR_DTYPE).reshape(-1)
    n, its, m = int(problem["n"][0]), int(problem["iterations"][0]), int(problem["min_set"][0])
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, max(m, 1))
    if len(corrs) < n or len(samples) < max(its, 0):
        raise ValueError("fewer correspondences or samples than the problem names")
    its0, words = max(its, 0), (max(n, 0) + 63) // 64
    out = {"counts": np.zeros(its0, np.int32), "hyps": np.zeros(its0, L.PNP_HYP_DTYPE),
           "masks": np.zeros((its0, words), np.uint64),
           "refines": np.zeros(its0, L.PNP_REFINE_DTYPE),
           "refined_masks": np.zeros((its0, words), np.uint64)}
    result = np.zeros(1, L.PNP_RESULT_DTYPE)
    inl = np.zeros(int(n1), np.uint8)
    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_pnp_solve(h, L.ptr(problem), L.ptr(corrs), L.ptr(samples), int(n1),
                                   L.ptr(out["counts"]), L.ptr(out["hyps"]), L.ptr(out["masks"]),
                                   L.ptr(out["refines"]), L.ptr(out["refined_masks"]),
                                   L.ptr(result), L.ptr(inl)), "orbg_pnp_solve")
    out["result"], out["inliers"] = result[0], inl
    return out


def solve_batch(problems, corrs, samples, ncand, cap, max_its, n1cap, out=None, ctx=None, device=0):
    """orbg_pnp_solve_batch_device on torch tensors of the device: `problems` the bytes of
    PNP_PROBLEM_DTYPE [ncand], `corrs` of PNP_CORR_DTYPE [ncand][cap], `samples` int32
    [ncand][max_its][8].  Returns (and, given as `out`, reuses) a dict of tensors: counts int32
    [ncand][max_its], hyps float64 [ncand][max_its][12] (R, t), masks and refined_masks int64
    [ncand][max_its][cap / 64] (the uint64 words), refines uint8 [ncand][max_its][112]
    (PNP_REFINE_DTYPE records), results uint8 [ncand][68] (PNP_RESULT_DTYPE records), inliers
    uint8 [ncand][n1cap].  Stream-ordered on the context stream with no host synchronisation:
    the inputs must be complete there (Context.set_stream or a synchronize before), and
    Context.sync() completes the outputs."""
    import torch
    dev = problems.device
    if out is None:
        words = max(cap // 64, 1)
        out = {"counts": torch.empty((ncand, max_its), dtype=torch.int32, device=dev),
               "hyps": torch.empty((ncand, max_its, 12), dtype=torch.float64, device=dev),
               "masks": torch.empty((ncand, max_its, words), dtype=torch.int64, device=dev),
               "refines": torch.empty((ncand, max_its, L.PNP_REFINE_DTYPE.itemsize),
                                      dtype=torch.uint8, device=dev),
               "refined_masks": torch.empty((ncand, max_its, words), dtype=torch.int64, device=dev),
               "results": torch.empty((ncand, L.PNP_RESULT_DTYPE.itemsize), dtype=torch.uint8,
                                      device=dev),
               "inliers": torch.empty((ncand, n1cap), dtype=torch.uint8, device=dev)}
    need = {"problems": (problems, ncand * L.PNP_PROBLEM_DTYPE.itemsize),
            "corrs": (corrs, ncand * cap * L.PNP_CORR_DTYPE.itemsize),
            "samples": (samples, ncand * max_its * MAX_SET * 4)}
    for k, (t, nbytes) in need.items():
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < nbytes:
            raise ValueError("%s: a contiguous device tensor of at least %d bytes" % (k, nbytes))
    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_pnp_solve_batch_device(
        h, problems.data_ptr(), corrs.data_ptr(), samples.data_ptr(), int(ncand), int(cap),
        int(max_its), out["counts"].data_ptr(), out["hyps"].data_ptr(), out["masks"].data_ptr(),
        out["refines"].data_ptr(), out["refined_masks"].data_ptr(), out["results"].data_ptr(),
        out["inliers"].data_ptr(), int(n1cap)), "orbg_pnp_solve_batch_device")
    return out


def _tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3).astype(np.float32)
    T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


class PnPsolver:
    def __init__(self, K, Xw, uv, sigma2, index, n1, device=0, seed=0, stream=None):
        """K: the Frame's fx, fy, cx, cy (or 3x3); the correspondence arrays as make_corrs; n1 =
        vpMapPointMatches.size(); `stream`: the rand() values to draw from (an iterable of
        integers in [0, 2^31); default: a NumPy generator seeded with `seed`)."""
        self.device = device
        self._corrs = make_corrs(Xw, uv, sigma2, index)
        self.N = len(self._corrs)
        self.mN1 = int(n1)
        if self.N > MAX_N:
            raise L.OrbgError(L.ORBG_ENOTSUP, "PnPsolver: more than %d correspondences" % MAX_N)
        if self.N and not (0 <= self._corrs["index"].min() and self._corrs["index"].max() < self.mN1):
            raise ValueError("index outside [0, n1)")
        self._K = K
        self._stream = iter(stream) if stream is not None else _rand_stream(seed)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = -1
        self._eval = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                            epsilon=0.4, th2=5.991):
        if not 4 <= int(minSet) <= MAX_SET:
            raise ValueError("minSet outside 4 .. %d" % MAX_SET)
        self.mRansacProb = float(probability)
        self.mRansacMinSet = int(minSet)
        self.mRansacTh2 = float(th2)
        if self.N > 0:
            self.mRansacMinInliers, self.mRansacMaxIts = ransac_parameters(
                probability, minInliers, maxIterations, minSet, epsilon, self.N)
        else:
            self.mRansacMinInliers = max(int(minInliers), int(minSet))
            self.mRansacMaxIts = max(1, int(maxIterations))
        self._eval = None   # the next iterate() draws and evaluates mRansacMaxIts iterations

    def _evaluate(self):
        its = self.mRansacMaxIts
        self.samples = draw_samples(self.N, its, self.mRansacMinSet, self._stream)
        prob = make_problem(self._K, self.N, self.mRansacMinSet, self.mRansacMinInliers, its,
                            self.mRansacTh2)
        d = solve(prob, self._corrs, self.samples, self.mN1, device=self.device)
        d["bits"] = mask_bits(d["masks"], self.N)
        d["refined_bits"] = mask_bits(d["refined_masks"], self.N)
        self._eval = d
        self.result, self.inliers = d["result"], d["inliers"]   # find() from a fresh solver

    def _scatter(self, bits):
        inl = np.zeros(self.mN1, bool)
        inl[self._corrs["index"][bits]] = True
        return inl

    def iterate(self, nIterations):
        """cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers) -> (Tcw 4x4 float32 or
        None, bNoMore, vbInliers bool [n1], nInliers)."""
        none = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers or self.N < self.mRansacMinSet:
            return None, True, none, 0
        if self._eval is None:
            self._evaluate()
        d = self._eval
        cur = 0
        # the reference's OR: up to mRansacMaxIts in the first call, nIterations more in a
        # later one; the evaluated iterations are all there are
        while (self.mnIterations < self.mRansacMaxIts or cur < nIterations) and \
                self.mnIterations < len(d["counts"]):
            i = self.mnIterations
            cur += 1
            self.mnIterations += 1
            c = int(d["counts"][i])
            if c >= self.mRansacMinInliers:
                if c > self.mnBestInliers:
                    self.mnBestInliers, self._best = c, i
                r = d["refines"][self._best]   # Refine() on the best set so far
                if r["ok"]:
                    return (_tcw(r["hyp"]["R"], r["hyp"]["t"]), False,
                            self._scatter(d["refined_bits"][self._best]), int(r["count"]))
        if self.mnIterations >= self.mRansacMaxIts:
            if self._best >= 0:
                h = d["hyps"][self._best]
                return (_tcw(h["R"], h["t"]), True, self._scatter(d["bits"][self._best]),
                        self.mnBestInliers)
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        """cv::Mat find(vbInliers, nInliers) -> (Tcw or None, vbInliers, nInliers)."""
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n

    @property
    def best_iteration(self):
        """The record iteration holding mBestTcw / the set Refine() works on (-1: none yet)."""
        return self._best

    solve_batch = staticmethod(solve_batch)
