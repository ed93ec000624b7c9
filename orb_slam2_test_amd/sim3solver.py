"""Sim3Solver -- ORB-SLAM2's RANSAC over Horn's closed-form Sim3 (include/Sim3Solver.h,
src/Sim3Solver.cc; LoopClosing::ComputeSim3, LoopClosing.cc:530-594), evaluated on the device
behind liborbg's orbg_sim3_* entry points.

The caller compacts the correspondences the way the constructor does (:62-102): world
positions of pMP1 / pMP2, mvLevelSigma2 of the two keypoints and index1 = the slot in
vpMatched12.  Every RANSAC iteration is evaluated once, in one launch; iterate() then serves
its windows from the downloaded counts, hypotheses and masks by the reference's sequential
rule, so iterate(5) can be called again and again as LoopClosing does, after a hit too.

    solver = Sim3Solver(T1w, T2w, K1, K2, Xw1, Xw2, sigma2_1, sigma2_2, index1, n1, bFixScale)
    solver.SetRansacParameters(0.99, 20, 300)
    T12, bNoMore, vbInliers, nInliers = solver.iterate(5)
    R, t, s = (solver.GetEstimatedRotation(), solver.GetEstimatedTranslation(),
               solver.GetEstimatedScale())

The random draws are the reference's (DUtils::Random::RandomInt on rand(), with the
swap-remove of Sim3Solver.cc:163-177) applied to a stream of 31-bit integers: `stream`, or a
NumPy generator seeded with `seed`.
"""
import numpy as np

from . import _lib as L
from .orbmatcher import _ctx

MAX_N = 8192   # correspondences per pair (ORBG_ENOTSUP past it)


def draw_samples(n, its, stream):
    """The three distinct correspondence indices of `its` iterations over `n` correspondences
    (int32 [its][3]).  `stream` yields what rand() would: integers in [0, 2^31).  Per draw
    (Sim3Solver.cc:163-177, Random.cpp:47-50): randi = int(r / 2^31 * m) over the m indices
    still available, the chosen one is replaced by the back and the back is popped."""
    out = np.zeros((int(its), 3), np.int32)
    if n < 3:
        return out
    it = iter(stream)
    base = list(range(int(n)))
    for k in range(int(its)):
        avail = base.copy()
        for j in range(3):
            r = int(next(it))
            if not 0 <= r < 2147483648:
                raise ValueError("the stream must yield integers in [0, 2^31)")
            randi = int(r / 2147483648.0 * len(avail))
            out[k, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def _rand_stream(seed):
    rng = np.random.default_rng(seed)
    while True:
        for r in rng.integers(0, 2147483648, 4096):
            yield int(r)


def _pose34(T):
    T = np.asarray(T, np.float32)
    if T.shape not in ((3, 4), (4, 4)):
        raise ValueError("a pose is 3x4 or 4x4")
    return np.ascontiguousarray(T[:3, :4]).reshape(12)


def _intrinsics(K):
    K = np.asarray(K, np.float32)
    if K.shape == (3, 3):
        return K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if K.shape == (4,):
        return tuple(K)
    raise ValueError("K is 3x3 or (fx, fy, cx, cy)")


def make_problem(T1w, T2w, K1, K2, n, fix_scale, min_inliers, iterations):
    """One orbg_sim3_problem record (SIM3_PROBLEM_DTYPE scalar array of shape (1,))."""
    p = np.zeros(1, L.SIM3_PROBLEM_DTYPE)
    p["T1w"][0], p["T2w"][0] = _pose34(T1w), _pose34(T2w)
    p["fx1"], p["fy1"], p["cx1"], p["cy1"] = _intrinsics(K1)
    p["fx2"], p["fy2"], p["cx2"], p["cy2"] = _intrinsics(K2)
    p["n"], p["fix_scale"] = int(n), 1 if fix_scale else 0
    p["min_inliers"], p["iterations"] = int(min_inliers), int(iterations)
    return p


def make_corrs(Xw1, Xw2, sigma2_1, sigma2_2, index1):
    """orbg_sim3_corr records (SIM3_CORR_DTYPE [n]) from the per-correspondence arrays."""
    Xw1 = np.asarray(Xw1, np.float32).reshape(-1, 3)
    n = len(Xw1)
    c = np.zeros(n, L.SIM3_CORR_DTYPE)
    c["Xw1"] = Xw1
    c["Xw2"] = np.asarray(Xw2, np.float32).reshape(n, 3)
    c["sigma2_1"] = np.asarray(sigma2_1, np.float32).reshape(n)
    c["sigma2_2"] = np.asarray(sigma2_2, np.float32).reshape(n)
    c["index1"] = np.asarray(index1, np.int32).reshape(n)
    return c


def ransac_iterations(prob, min_inliers, max_its, n):
    """mRansacMaxIts of SetRansacParameters (:114-138) for n correspondences (host only)."""
    return int(L.lib().orbg_sim3_ransac_iterations(float(prob), int(min_inliers), int(max_its),
                                                   int(n)))


def mask_bits(words, n):
    """bool [..., n] from mask words uint64 [..., ceil(n / 64)] (bit i % 64 of word i / 64)."""
    w = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1,
                         bitorder="little")
    return bits[..., :n].astype(bool)


def solve(problem, corrs, samples, n1, ctx=None, device=0):
    """orbg_sim3_solve: (counts [its], hyps [its], masks uint64 [its][ceil(n / 64)], result,
    inliers12 uint8 [n1]) of one pair from host records."""
    problem = np.ascontiguousarray(problem, L.SIM3_PROBLEM_DTYPE).reshape(1)
    corrs = np.ascontiguousarray(corrs, L.SIM3_CORR_DTYPE).reshape(-1)
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
    n, its = int(problem["n"][0]), int(problem["iterations"][0])
    if len(corrs) < n or len(samples) < max(its, 0):
        raise ValueError("fewer correspondences or sample triples than the problem names")
    counts = np.zeros(max(its, 0), np.int32)
    hyps = np.zeros(max(its, 0), L.SIM3_HYP_DTYPE)
    masks = np.zeros((max(its, 0), (max(n, 0) + 63) // 64), np.uint64)
    result = np.zeros(1, L.SIM3_RESULT_DTYPE)
    inl = np.zeros(int(n1), np.uint8)
    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_sim3_solve(h, L.ptr(problem), L.ptr(corrs), L.ptr(samples), int(n1),
                                    L.ptr(counts), L.ptr(hyps), L.ptr(masks), L.ptr(result),
                                    L.ptr(inl)), "orbg_sim3_solve")
    return counts, hyps, masks, result[0], inl


class Sim3Solver:
    def __init__(self, T1w, T2w, K1, K2, Xw1, Xw2, sigma2_1, sigma2_2, index1, n1,
                 bFixScale=False, device=0, seed=0, stream=None):
        """T1w / T2w: pKF1 / pKF2 GetPose(); K1 / K2: mK (3x3, or fx, fy, cx, cy); the
        correspondence arrays as make_corrs; n1 = vpMatched12.size(); `stream`: the rand()
        values to draw from (an iterable of integers in [0, 2^31); default: a NumPy generator
        seeded with `seed`)."""
        self.device = device
        self._corrs = make_corrs(Xw1, Xw2, sigma2_1, sigma2_2, index1)
        self.N = len(self._corrs)
        self.mN1 = int(n1)
        if self.N > MAX_N:
            raise L.OrbgError(L.ORBG_ENOTSUP, "Sim3Solver: more than %d correspondences" % MAX_N)
        if self.N and not (0 <= self._corrs["index1"].min() and self._corrs["index1"].max() < self.mN1):
            raise ValueError("index1 outside [0, n1)")
        self._geo = (T1w, T2w, K1, K2)
        self.mbFixScale = bool(bFixScale)
        self._stream = iter(stream) if stream is not None else _rand_stream(seed)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = -1
        self._eval = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb = float(probability)
        self.mRansacMinInliers = int(minInliers)
        self.mRansacMaxIts = (ransac_iterations(probability, minInliers, maxIterations, self.N)
                              if self.N > 0 else max(1, int(maxIterations)))
        self.mnIterations = 0
        self._eval = None   # the next iterate() draws and evaluates mRansacMaxIts iterations

    def _evaluate(self):
        its = self.mRansacMaxIts
        self.samples = draw_samples(self.N, its, self._stream)
        prob = make_problem(*self._geo, self.N, self.mbFixScale, self.mRansacMinInliers, its)
        counts, hyps, masks, result, inl = solve(prob, self._corrs, self.samples, self.mN1,
                                                 device=self.device)
        self._eval = (counts, hyps, mask_bits(masks, self.N))
        self.result, self.inliers12 = result, inl   # find() from a fresh solver, as the device sees it

    def iterate(self, nIterations):
        """cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers) -> (T12 4x4 float32 or
        None, bNoMore, vbInliers bool [n1], nInliers)."""
        inl = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers or self.N < 3:
            return None, True, inl, 0
        if self._eval is None:
            self._evaluate()
        counts, hyps, bits = self._eval
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            i = self.mnIterations
            cur += 1
            self.mnIterations += 1
            c = int(counts[i])
            if c >= self.mnBestInliers:
                self.mnBestInliers, self._best = c, i
                self._best_hyp = hyps[i].copy()
                if c > self.mRansacMinInliers:
                    inl[self._corrs["index1"][bits[i]]] = True
                    return self._T12(self._best_hyp), False, inl, c
        return None, self.mnIterations >= self.mRansacMaxIts, inl, 0

    def find(self):
        """cv::Mat find(vbInliers12, nInliers) -> (T12 or None, vbInliers12, nInliers)."""
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n

    @staticmethod
    def _T12(h):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.float32(h["s"]) * h["R"].reshape(3, 3)
        T[:3, 3] = h["t"]
        return T

    @property
    def best_iteration(self):
        """The iteration whose hypothesis GetEstimated* return (-1: none yet)."""
        return self._best

    def GetEstimatedRotation(self):
        return None if self._best < 0 else self._best_hyp["R"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return None if self._best < 0 else self._best_hyp["t"].copy()

    def GetEstimatedScale(self):
        return None if self._best < 0 else float(self._best_hyp["s"])

    @staticmethod
    def solve_batch(problems, corrs, samples, npairs, cap, max_its, n1cap, out=None, ctx=None,
                    device=0):
        """orbg_sim3_solve_batch_device on torch tensors of the device: `problems` the bytes
        of SIM3_PROBLEM_DTYPE [npairs], `corrs` of SIM3_CORR_DTYPE [npairs][cap], `samples`
        int32 [npairs][max_its][3].  Returns (and, given as `out`, reuses) a dict of tensors:
        counts int32 [npairs][max_its], hyps float32 [npairs][max_its][13] (R, t, s), masks
        int64 [npairs][max_its][cap / 64] (the uint64 words), results uint8 [npairs][68]
        (SIM3_RESULT_DTYPE records), inliers12 uint8 [npairs][n1cap].  Stream-ordered on the
        context stream with no host synchronisation: the inputs must be complete there
        (Context.set_stream or a synchronize before), and Context.sync() completes the outputs."""
        import torch
        dev = problems.device
        if out is None:
            out = {"counts": torch.empty((npairs, max_its), dtype=torch.int32, device=dev),
                   "hyps": torch.empty((npairs, max_its, 13), dtype=torch.float32, device=dev),
                   "masks": torch.empty((npairs, max_its, max(cap // 64, 1)), dtype=torch.int64,
                                        device=dev),
                   "results": torch.empty((npairs, L.SIM3_RESULT_DTYPE.itemsize),
                                          dtype=torch.uint8, device=dev),
                   "inliers12": torch.empty((npairs, n1cap), dtype=torch.uint8, device=dev)}
        need = {"problems": (problems, npairs * L.SIM3_PROBLEM_DTYPE.itemsize),
                "corrs": (corrs, npairs * cap * L.SIM3_CORR_DTYPE.itemsize),
                "samples": (samples, npairs * max_its * 12)}
        for k, (t, nbytes) in need.items():
            if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < nbytes:
                raise ValueError("%s: a contiguous device tensor of at least %d bytes" % (k, nbytes))
        h = (ctx if ctx is not None else _ctx(device)).handle
        L.check(L.lib().orbg_sim3_solve_batch_device(
            h, problems.data_ptr(), corrs.data_ptr(), samples.data_ptr(), int(npairs), int(cap),
            int(max_its), out["counts"].data_ptr(), out["hyps"].data_ptr(),
            out["masks"].data_ptr(), out["results"].data_ptr(), out["inliers12"].data_ptr(),
            int(n1cap)), "orbg_sim3_solve_batch_device")
        return out
