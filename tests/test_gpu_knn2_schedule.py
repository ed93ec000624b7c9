"""GPU: the knn2 train loop (knn2_block_fp4 in csrc/match_kernels.hip) at every boundary of
its schedule, against a NumPy brute force written here (independent of oracle/).

The loop walks the train rows in 32-row subtiles, two accumulator sets alternating, one
barrier per stage of 64 rows (a 128-row stage is a build variant), the top-2 update of one
subtile issued between the MFMAs of the next.  What can go wrong there shows at the subtile,
stage, wave (64 queries), 32-column half and workgroup (256 queries) boundaries, so the shapes
below sit on and around each of them; the results must be the reference's to the bit.
"""
import numpy as np
import pytest

from orb_slam2_test_amd import ORBextractor, ORBmatcher, synthetic as S

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
TRAIN_COUNTS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256,
                257]
QUERY_COUNTS = [1, 33, 64, 65, 255, 256, 257]
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def brute_knn2(q, t):
    """ORBmatcher's best / second rule: XOR, popcount, a strict-< scan in train order (so the
    first index wins a tie, and a second equal distance becomes the second best)."""
    nq = len(q)
    bi = np.full(nq, -1, np.int32)
    bd = np.full(nq, INT_MAX, np.int32)
    sd = np.full(nq, INT_MAX, np.int32)
    for j in range(len(t)):
        d = POPCOUNT[q ^ t[j]].sum(1).astype(np.int32)
        better = d < bd
        second = ~better & (d < sd)
        sd = np.where(better, bd, np.where(second, d, sd))
        bi = np.where(better, j, bi).astype(np.int32)
        bd = np.where(better, d, bd)
    return bi, bd, sd


@pytest.fixture(scope="module")
def base():
    rng = np.random.default_rng(20240611)
    t = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    t.setflags(write=False)
    q.setflags(write=False)
    return q, t


def flip(row, bit):
    r = row.copy()
    r[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return r


def plant(q, t, nq, nt):
    """Returns the planted copies (q', t').  Train side: row 3 repeated 32 rows (a later
    subtile), 64 and 128 rows (later stages) further on where nt reaches.  Query side, on
    distinct rows as far as nq has them: a copy of train row 3 (d = 0: index 3 must win over
    its duplicates, which make the second distance 0 too), the complement of the last train
    row (d = 256), and a row one bit away from two train rows (best == second == 1, the lower
    index wins)."""
    q, t = q[:nq].copy(), t[:nt].copy()
    src = min(3, nt - 1)
    for off in (32, 64, 128):
        if src + off < nt:
            t[src + off] = t[src]
    slots = [0, nq // 3, nq // 2, nq - 1]
    q[slots[0]] = t[src]
    if len(set(slots)) == 4:
        q[slots[1]] = ~t[nt - 1]
        if nt >= 12:
            tie = t[10].copy()
            t[10] = flip(tie, 5)
            t[11] = flip(tie, 77)
            q[slots[2]] = tie
    return q, t


def check(q, t):
    got = ORBmatcher().hamming_knn2(q, t)
    ref = brute_knn2(q, t)
    for name, g, r in zip(("best index", "best distance", "second distance"), got, ref):
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, "%s differs at queries %s (nq %d, nt %d): got %s, want %s" % (
            name, bad[:8], len(q), len(t), g[bad[:8]], r[bad[:8]])
    return ref


@pytest.mark.parametrize("nt", TRAIN_COUNTS)
def test_single_train_boundaries(base, nt):
    bq, bt = base
    for nq in QUERY_COUNTS:
        q, t = plant(bq, bt, nq, nt)
        bi, bd, sd = check(q, t)
        src = min(3, nt - 1)
        assert bi[0] == src and bd[0] == 0
        if src + 32 < nt:
            assert sd[0] == 0
        if nq >= 33 and nt >= 12:
            assert (bi[nq // 2], bd[nq // 2], sd[nq // 2]) == (10, 1, 1)


@pytest.mark.parametrize("what", ["equal", "complement", "tie"])
def test_single_one_query_plants(base, what):
    """nq = 1 holds one planted row at a time."""
    bq, bt = base
    for nt in TRAIN_COUNTS:
        t = bt[:nt].copy()
        if what == "equal":
            q = t[nt - 1:nt].copy()
            want = (nt - 1, 0)
        elif what == "complement":
            q = ~t[nt - 1:nt]
            want = (0, 256) if nt == 1 else None
        else:
            if nt < 2:
                continue
            q = t[nt - 1:nt].copy()
            t[nt - 2] = flip(q[0], 200)
            t[nt - 1] = flip(q[0], 9)
            want = (nt - 2, 1)
        bi, bd, sd = check(q, t)
        assert want is None or (bi[0], bd[0]) == want
        if what == "tie":
            assert sd[0] == 1


def test_single_empty_train(base):
    bq, bt = base
    for nq in QUERY_COUNTS:
        bi, bd, sd = ORBmatcher().hamming_knn2(bq[:nq], bt[:0])
        assert np.all(bi == -1) and np.all(bd == INT_MAX) and np.all(sd == INT_MAX)


def test_batched_pairs():
    """match_batch_device on 5 synthetic frames at 160 x 120 (4 pyramid levels: the image is
    too small for more), 200 features asked: the frames keep between about 180 and 200
    keypoints, different from frame to frame, and some of them an odd number of 32-row
    subtiles, so the trailing half stage runs beside full ones in one launch.  Every pair's
    rows are compared.  A synthetic sequence frame of this size never has zero keypoints, so
    download_matches does not reach an empty frame here; the single entry covers nt = 0."""
    import torch
    B = 5
    frames = S.sequence(B, 120, 160, seed=7101)
    d = torch.from_numpy(frames).cuda()
    ext = ORBextractor(200, 1.2, 4, 20, 7, max_batch=B)
    ext.extract_batch_device(d.data_ptr(), B, 160, 120)
    f1 = np.array([0, 1, 2, 3, 4, 2, 4], np.int32)
    f2 = np.array([1, 2, 3, 4, 0, 0, 1], np.int32)
    ext.match_batch_device(f1, f2, 100, 0.9, True)
    ext.ctx.sync()
    desc = [ext.download_frame(f)[1] for f in range(B)]
    counts = [len(x) for x in desc]
    assert len(set(counts)) > 1, counts
    assert any(((c + 31) // 32) % 2 == 1 for c in (counts[f] for f in f1)), counts
    for p in range(len(f1)):
        dq, dt = desc[f2[p]], desc[f1[p]]
        knn = ext.download_matches(p, max(len(dq), len(dt)))[0]
        ref = brute_knn2(dq, dt)
        for col in range(3):
            assert np.array_equal(knn[:len(dq), col], ref[col]), (p, col)
