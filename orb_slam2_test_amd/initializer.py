"""Initializer -- ORB-SLAM2's monocular two-view initialisation (include/Initializer.h,
src/Initializer.cc; Tracking::MonocularInitialization), evaluated on the device behind
liborbg's orbg_initialize* entry points: the H / F RANSAC over the eight-point sets, the model
choice and ReconstructH / ReconstructF with their triangulation passes.

    init = Initializer(reference_keys, K, sigma=1.0, iterations=200)
    ok, R21, t21, vP3D, vbTriangulated = init.Initialize(current_keys, vMatches12)

The keys are the frames' undistorted keypoints (KP_DTYPE records or [n][2] positions) and
vMatches12 is what ORBmatcher.SearchForInitialization returns.  The device compacts
mvMatches12 itself, so in the batched form (initialize_batch) the matcher's device output feeds
the call directly.

The random draws are the reference's (DUtils::Random::RandomInt on rand(), with the
swap-remove of Initializer.cc:135-150) applied to a stream of 31-bit integers: `stream`, or a
NumPy generator seeded with `seed` (the integer stream of Sim3Solver and PnPsolver).
"""
import numpy as np

from . import _lib as L
from .orbmatcher import _ctx
from .sim3solver import _rand_stream, _intrinsics, mask_bits  # noqa: F401

MAX_N = L.INIT_MAX_N   # keypoints per frame (ORBG_ENOTSUP past it)


def draw_sets(n, iterations, stream):
    """mvSets (Initializer.cc:131-150): the eight distinct match indices of `iterations`
    iterations over `n` matches (int32 [iterations][8]; zeros for n < 8, where the reference's
    draw is undefined).  `stream` yields what rand() would: integers in [0, 2^31).  Per draw
    (Random.cpp:47-50): randi = int(r / 2^31 * m) over the m indices still available, the
    chosen one is replaced by the back and the back is popped."""
    out = np.zeros((int(iterations), 8), np.int32)
    if n < 8:
        return out
    it = iter(stream)
    base = list(range(int(n)))
    for k in range(int(iterations)):
        avail = base.copy()
        for j in range(8):
            r = int(next(it))
            if not 0 <= r < 2147483648:
                raise ValueError("the stream must yield integers in [0, 2^31)")
            randi = int(r / 2147483648.0 * len(avail))
            out[k, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def make_problem(K, sigma=1.0, iterations=200, min_parallax=1.0, min_triangulated=50):
    """One orbg_init_problem record (INIT_PROBLEM_DTYPE array of shape (1,))."""
    p = np.zeros(1, L.INIT_PROBLEM_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = _intrinsics(K)
    p["sigma"], p["min_parallax"] = np.float32(sigma), np.float32(min_parallax)
    p["min_triangulated"], p["iterations"] = int(min_triangulated), int(iterations)
    return p


def as_keys(keys):
    """KP_DTYPE records from records or from [n][2] positions."""
    a = np.asarray(keys)
    if a.dtype == L.KP_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.asarray(keys, np.float32).reshape(-1, 2)
    k = np.zeros(len(a), L.KP_DTYPE)
    k["x"], k["y"] = a[:, 0], a[:, 1]
    return k


def count_matches(matches12, n2):
    m = np.asarray(matches12)
    return int(((m >= 0) & (m < n2)).sum())


def initialize(problem, keys1, keys2, matches12, sets, ctx=None, device=0):
    """orbg_initialize on one pair's host arrays.  Returns a dict: result (an
    INIT_RESULT_DTYPE record), p3d float32 [n1][3], triangulated uint8 [n1], scores_h / scores_f
    [its], H21 / F21 float32 [its][9], masks_h / masks_f uint64 [its][ceil(N / 64)]."""
    problem = np.ascontiguousarray(problem, L.INIT_PROBLEM_DTYPE).reshape(1)
    k1, k2 = as_keys(keys1), as_keys(keys2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    if len(m12) != len(k1):
        raise ValueError("matches12 has one entry per reference keypoint")
    its = max(int(problem["iterations"][0]), 0)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    if len(sets) < its:
        raise ValueError("fewer sets than the problem's iterations")
    n1, n2 = len(k1), len(k2)
    words = (count_matches(m12, n2) + 63) // 64
    out = {"p3d": np.zeros((n1, 3), np.float32), "triangulated": np.zeros(n1, np.uint8),
           "scores_h": np.zeros(its, np.float32), "scores_f": np.zeros(its, np.float32),
           "H21": np.zeros((its, 9), np.float32), "F21": np.zeros((its, 9), np.float32),
           "masks_h": np.zeros((its, words), np.uint64), "masks_f": np.zeros((its, words), np.uint64)}
    result = np.zeros(1, L.INIT_RESULT_DTYPE)
    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_initialize(h, L.ptr(problem), L.ptr(k1), n1, L.ptr(k2), n2, L.ptr(m12),
                                    L.ptr(sets), L.ptr(result), L.ptr(out["p3d"]),
                                    L.ptr(out["triangulated"]), L.ptr(out["scores_h"]),
                                    L.ptr(out["scores_f"]), L.ptr(out["H21"]), L.ptr(out["F21"]),
                                    L.ptr(out["masks_h"]), L.ptr(out["masks_f"])), "orbg_initialize")
    out["result"] = result[0]
    return out


def initialize_batch(problems, kps, frame_stride, counts, nframes, f1, f2, matches12, sets, npairs,
                     cap, max_its, out=None, details=True, match_stride=None, ctx=None, device=0):
    """orbg_initialize_batch_device.  problems / f1 / f2 / sets are torch tensors of the device
    (the bytes of INIT_PROBLEM_DTYPE [npairs], int32 [npairs], int32 [npairs][max_its][8]); kps,
    counts and matches12 are device tensors or the integer device pointers orbg_batch_outputs /
    orbg_batch_keys_un / orbg_match_outputs return; match_stride is the row length of matches12
    (default: cap; the matcher's frame_cap for its output).  Returns (and, given as `out`, reuses) a
    dict of tensors: results uint8 [npairs][544] (INIT_RESULT_DTYPE records), p3d float32
    [npairs][cap][3], triangulated uint8 [npairs][cap] and, with `details`, scores_h / scores_f
    float32 [npairs][max_its], H21 / F21 float32 [npairs][max_its][9], masks_h / masks_f int64
    [npairs][max_its][cap / 64] (the uint64 words).  Stream-ordered on the context stream with
    no host synchronisation: the inputs must be complete there, and Context.sync() completes
    the outputs."""
    import torch
    dev = problems.device
    match_stride = int(cap if match_stride is None else match_stride)
    if out is None:
        words = max(cap // 64, 1)
        out = {"results": torch.empty((npairs, L.INIT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev),
               "p3d": torch.empty((npairs, cap, 3), dtype=torch.float32, device=dev),
               "triangulated": torch.empty((npairs, cap), dtype=torch.uint8, device=dev)}
        if details:
            out.update({"scores_h": torch.empty((npairs, max_its), dtype=torch.float32, device=dev),
                        "scores_f": torch.empty((npairs, max_its), dtype=torch.float32, device=dev),
                        "H21": torch.empty((npairs, max_its, 9), dtype=torch.float32, device=dev),
                        "F21": torch.empty((npairs, max_its, 9), dtype=torch.float32, device=dev),
                        "masks_h": torch.empty((npairs, max_its, words), dtype=torch.int64, device=dev),
                        "masks_f": torch.empty((npairs, max_its, words), dtype=torch.int64, device=dev)})
    need = {"problems": (problems, npairs * L.INIT_PROBLEM_DTYPE.itemsize), "f1": (f1, npairs * 4),
            "f2": (f2, npairs * 4), "sets": (sets, npairs * max_its * 32),
            "kps": (kps, nframes * frame_stride * L.KP_DTYPE.itemsize), "counts": (counts, nframes * 4),
            "matches12": (matches12, npairs * match_stride * 4)}
    ptrs = {}
    for k, (t, nbytes) in need.items():
        if isinstance(t, int):
            ptrs[k] = t
            continue
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < nbytes:
            raise ValueError("%s: a contiguous device tensor of at least %d bytes" % (k, nbytes))
        ptrs[k] = t.data_ptr()

    def opt(k):
        return out[k].data_ptr() if k in out else None

    h = (ctx if ctx is not None else _ctx(device)).handle
    L.check(L.lib().orbg_initialize_batch_device(
        h, ptrs["problems"], ptrs["kps"], int(frame_stride), ptrs["counts"], int(nframes),
        ptrs["f1"], ptrs["f2"], ptrs["matches12"], match_stride, ptrs["sets"], int(npairs), int(cap),
        int(max_its), out["results"].data_ptr(), out["p3d"].data_ptr(),
        out["triangulated"].data_ptr(), opt("scores_h"), opt("scores_f"), opt("H21"), opt("F21"),
        opt("masks_h"), opt("masks_f")), "orbg_initialize_batch_device")
    return out


def pack_host_batch(problems, kps, counts, f1, f2, matches12, sets):
    """The input file of lib/init_host (csrc/init_host.hip) for a batch given as host arrays:
    problems INIT_PROBLEM_DTYPE [npairs], kps KP_DTYPE [nframes][frame_stride], counts int32
    [nframes], f1 / f2 int32 [npairs], matches12 int32 [npairs][cap], sets int32
    [npairs][max_its][8].  Returns (bytes, (npairs, cap, max_its))."""
    problems = np.ascontiguousarray(problems, L.INIT_PROBLEM_DTYPE).reshape(-1)
    kps = np.ascontiguousarray(kps, L.KP_DTYPE)
    matches12 = np.ascontiguousarray(matches12, np.int32)
    sets = np.ascontiguousarray(sets, np.int32)
    npairs, cap, max_its = len(problems), matches12.shape[1], sets.shape[1]
    hd = np.array([npairs, cap, max_its, kps.shape[1], kps.shape[0], cap, 0, 0], np.int32)
    parts = [hd, problems, kps, np.ascontiguousarray(counts, np.int32),
             np.ascontiguousarray(f1, np.int32), np.ascontiguousarray(f2, np.int32), matches12, sets]
    return b"".join(a.tobytes() for a in parts), (npairs, cap, max_its)


def unpack_host_output(buf, npairs, cap, max_its):
    """The output file of lib/init_host as the dict initialize_batch returns (NumPy arrays)."""
    rows, words, o, out = npairs * max_its, cap // 64, 0, {}
    for k, dt, shape in (("results", L.INIT_RESULT_DTYPE, (npairs,)), ("p3d", np.float32, (npairs, cap, 3)),
                         ("triangulated", np.uint8, (npairs, cap)), ("scores_h", np.float32, (npairs, max_its)),
                         ("scores_f", np.float32, (npairs, max_its)), ("H21", np.float32, (npairs, max_its, 9)),
                         ("F21", np.float32, (npairs, max_its, 9)),
                         ("masks_h", np.uint64, (npairs, max_its, words)),
                         ("masks_f", np.uint64, (npairs, max_its, words))):
        n = int(np.prod(shape))
        out[k] = np.frombuffer(buf, dt, n, o).reshape(shape).copy()
        o += n * np.dtype(dt).itemsize
    assert o == len(buf) and rows >= 0
    return out


class Initializer:
    def __init__(self, reference_keys, K, sigma=1.0, iterations=200, device=0, seed=0, stream=None):
        """Initializer(ReferenceFrame, sigma, iterations) (:34-47): reference_keys =
        ReferenceFrame.mvKeysUn, K = ReferenceFrame.mK (3x3 or fx, fy, cx, cy); `stream`: the
        rand() values to draw from (default: a NumPy generator seeded with `seed`)."""
        self.device = device
        self.mvKeys1 = as_keys(reference_keys)
        if len(self.mvKeys1) > MAX_N:
            raise L.OrbgError(L.ORBG_ENOTSUP, "Initializer: more than %d keypoints" % MAX_N)
        self.mK = K
        self.mSigma = float(sigma)
        self.mMaxIterations = int(iterations)
        self._stream = iter(stream) if stream is not None else _rand_stream(seed)
        self.mvSets = None
        self.last = None

    def Initialize(self, current_keys, matches12, min_parallax=1.0, min_triangulated=50):
        """bool Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) ->
        (ok, R21 3x3 float32, t21 [3] float32, vP3D float32 [n1][3], vbTriangulated bool [n1]);
        R21 and t21 are None unless ok.  The records of the call stay in `last`."""
        k2 = as_keys(current_keys)
        n = count_matches(matches12, len(k2))
        self.mvSets = draw_sets(n, self.mMaxIterations, self._stream)
        prob = make_problem(self.mK, self.mSigma, self.mMaxIterations, min_parallax, min_triangulated)
        d = initialize(prob, self.mvKeys1, k2, matches12, self.mvSets, device=self.device)
        self.last = d
        r = d["result"]
        ok = bool(r["success"])
        return (ok, r["R21"].reshape(3, 3).copy() if ok else None, r["t21"].copy() if ok else None,
                d["p3d"], d["triangulated"].astype(bool))

    initialize_batch = staticmethod(initialize_batch)
