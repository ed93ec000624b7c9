"""Independent pure-Python restatement of DBoW2's L1 score and ORB-SLAM2's KeyFrameDatabase,
written from Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68 and src/KeyFrameDatabase.cc in
their own shape: BowVectors are word -> weight maps walked by two iterators, the inverted
file is a list of per-word lists of KeyFrame objects, and the per-query bookkeeping
(mnRelocQuery, mnRelocWords, mRelocScore, mnLoopQuery, mnLoopWords, mLoopScore) lives on the
KeyFrame objects.  Doubles are Python floats; wherever the reference holds a `float`
(the scores si, accScore, bestAccScore, minScoreToRetain, maxCommonWords * 0.8f) the value is
an np.float32.

The one deliberate departure from the reference, shared with the library:
KeyFrame::mRelocScore, uninitialised in KeyFrame.cc:39-40, is 0 from add() on.
"""
import bisect

import numpy as np

F32 = np.float32


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2); v1, v2: dict word -> weight."""
    k1, k2 = sorted(v1), sorted(v2)
    i1 = i2 = 0
    score = 0.0
    while i1 < len(k1) and i2 < len(k2):
        vi, wi = v1[k1[i1]], v2[k2[i2]]
        if k1[i1] == k2[i2]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif k1[i1] < k2[i2]:
            i1 = bisect.bisect_left(k1, k2[i2])      # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect.bisect_left(k2, k1[i1])
    return -score / 2.0


class KeyFrame:
    def __init__(self, slot, bow):
        self.slot = slot
        self.mBowVec = dict(bow)
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)
        self.mnLoopQuery = -1
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.neighbours = []          # GetBestCovisibilityKeyFrames(10): KeyFrame objects


class RefKeyFrameDatabase:
    """KeyFrameDatabase over slots; the caller supplies what the reference reads from the
    covisibility graph (set_neighbours, `connected`)."""

    def __init__(self, nwords, max_keyframes):
        self.mvInvertedFile = [[] for _ in range(nwords)]
        self.kfs = [None] * max_keyframes
        self.next_id = 0              # Frame / KeyFrame mnId of the queries
        self.stored_reads = 0         # accumulations that read an unscored neighbour's score

    def add(self, slot, bow):
        assert self.kfs[slot] is None
        kf = self.kfs[slot] = KeyFrame(slot, bow)
        for w in sorted(kf.mBowVec):
            self.mvInvertedFile[w].append(kf)

    def erase(self, slot):
        kf = self.kfs[slot]
        if kf is None:
            return
        for w in sorted(kf.mBowVec):
            lst = self.mvInvertedFile[w]
            for i, o in enumerate(lst):
                if o is kf:
                    del lst[i]
                    break
        self.kfs[slot] = None

    def clear(self):
        self.mvInvertedFile = [[] for _ in self.mvInvertedFile]
        self.kfs = [None] * len(self.kfs)

    def set_neighbours(self, neigh):
        """neigh[slot] = up to 10 slots (-1 unused); dead slots are skipped."""
        for kf in self.kfs:
            if kf is not None:
                kf.neighbours = [self.kfs[s] for s in neigh[kf.slot]
                                 if 0 <= s < len(self.kfs) and self.kfs[s] is not None]

    def reloc_scores(self):
        return np.array([F32(0) if k is None else k.mRelocScore for k in self.kfs], F32)

    # KeyFrameDatabase.cc:291-419
    def DetectRelocalizationCandidates(self, bow, info=None):
        fid = self.next_id
        self.next_id += 1
        lKFsSharingWords = []
        for w in sorted(bow):
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != fid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = fid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if info is not None:
            info.update(max_common=0, nscored=0, counts={})
        if not lKFsSharingWords:
            return []
        maxCommonWords = max(k.mnRelocWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if info is not None:
            info.update(max_common=maxCommonWords, nscored=len(lScoreAndMatch),
                        min_common=minCommonWords,
                        counts={k.slot: k.mnRelocWords for k in lKFsSharingWords})
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours:
                if pKF2.mnRelocQuery != fid:
                    continue
                if not pKF2.mnRelocWords > minCommonWords:
                    self.stored_reads += 1
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF, out = set(), []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain and pKFi.slot not in spAlreadyAddedKF:
                out.append(pKFi.slot)
                spAlreadyAddedKF.add(pKFi.slot)
        return out

    # KeyFrameDatabase.cc:106-274
    def DetectLoopCandidates(self, bow, connected, minScore, info=None):
        minScore = F32(minScore)
        kid = self.next_id
        self.next_id += 1
        spConnectedKeyFrames = set(connected)
        lKFsSharingWords = []
        for w in sorted(bow):
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != kid:
                    pKFi.mnLoopWords = 0
                    if pKFi.slot not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = kid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if info is not None:
            info.update(max_common=0, nscored=0, counts={})
        if not lKFsSharingWords:
            return []
        maxCommonWords = max(k.mnLoopWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if info is not None:
            info.update(max_common=maxCommonWords, nscored=nscores, min_common=minCommonWords,
                        counts={k.slot: k.mnLoopWords for k in lKFsSharingWords})
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours:
                if pKF2.mnLoopQuery == kid and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF, out = set(), []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain and pKFi.slot not in spAlreadyAddedKF:
                out.append(pKFi.slot)
                spAlreadyAddedKF.add(pKFi.slot)
        return out


def place_dataset(seed, nwords=1000, nkf=40, nplaces=4, nbase=60, nq=8):
    """The parity tests' recipe: nkf KeyFrames over nplaces places of nbase base words each;
    a KeyFrame holds nk in [15, 55] of its place's words plus nbase - nk random ones, with
    random L1-normalised weights; 0-10 random neighbours per slot (-1 padded); nq queries
    built the same way.  Returns (kf_bows, neigh [nkf][10], query_bows)."""
    rng = np.random.default_rng(seed)
    places = [rng.choice(nwords, nbase, replace=False) for _ in range(nplaces)]

    def vector(place):
        nk = int(rng.integers(15, 56))
        own = rng.choice(places[place], nk, replace=False)
        rest = np.setdiff1d(np.arange(nwords), own)
        words = np.concatenate([own, rng.choice(rest, nbase - nk, replace=False)])
        x = rng.uniform(0.1, 1.0, len(words))
        x = x / x.sum()
        return {int(w): float(v) for w, v in zip(words, x)}

    kfs = [vector(i % nplaces) for i in range(nkf)]
    neigh = np.full((nkf, 10), -1, np.int32)
    for s in range(nkf):
        n = int(rng.integers(0, 11))
        others = np.setdiff1d(np.arange(nkf), [s])
        neigh[s, :n] = rng.choice(others, n, replace=False)
    queries = [vector(int(rng.integers(0, nplaces))) for _ in range(nq)]
    return kfs, neigh, queries


# ---------------------------------------------------------------------------
# A 5-KeyFrame database small enough to work out by hand (20-word vocabulary).  With equal
# signs the score reduces to the sum over the common words of min(vi, wi); every weight is a
# power of two, so every figure below is exact in float32.
#
#   query Q   words 0..9, weight 1/16 each
#   slot 0 A  words 0..9          (10 common)  weight 1/8   -> score 10/16 = 0.625
#   slot 1 B  words 1..9, 15      ( 9 common)  weight 1/32  -> score 9/32  = 0.28125
#   slot 2 C  words 2..9 (1/4), 16, 17 (1/2)   ( 8 common)  -> score 8/16  = 0.5 if scored
#   slot 3 D  words 0..8, 18      ( 9 common)  weight 1/16  -> score 9/16  = 0.5625
#   slot 4 E  word 19             ( 0 common)
#   query Q0  words 16, 17, weight 1 each: shares only with C, score 2 * 1/2 = 1.0
#
# maxCommonWords = 10 -> minCommonWords = int(10 * 0.8f) = 8: C (8 == 8) is not scored.
# lKFsSharingWords for Q = A, D (word 0, add order), B (word 1), C (word 2).
# Neighbours: A: [C], B: [E, C], C: [B], D: [A].
# ---------------------------------------------------------------------------
HAND_NWORDS = 20
HAND_Q = {w: 1 / 16 for w in range(10)}
HAND_Q0 = {16: 1.0, 17: 1.0}
HAND_KFS = [
    {w: 1 / 8 for w in range(10)},
    {**{w: 1 / 32 for w in range(1, 10)}, 15: 1 / 32},
    {**{w: 1 / 4 for w in range(2, 10)}, 16: 1 / 2, 17: 1 / 2},
    {**{w: 1 / 16 for w in range(9)}, 18: 1 / 16},
    {19: 1.0},
]
HAND_NEIGH = np.full((5, 10), -1, np.int32)
HAND_NEIGH[0, 0] = 2
HAND_NEIGH[1, :2] = (4, 2)
HAND_NEIGH[2, 0] = 1
HAND_NEIGH[3, 0] = 0
