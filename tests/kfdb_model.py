"""KeyFrameDatabase as the reference writes it, statement by statement (src/KeyFrameDatabase.cc:39-377, haloc::Hash::match
src/hash.cpp:189-205, DBoW2::L1Scoring::score Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the third statement the device
database (uvo_kfdb_*) and its host build are held to.

Literal on purpose: the inverted file is a dict of per-word Python lists that add appends to and erase removes from, the keyframes
carry the six mutable fields the queries leave behind, the loops run in the source's order, and every rounding is a numpy float64 /
float32 scalar operation.  Nothing here knows the closed-form list order the kernels use (first common word, add sequence): the
list is whatever order the walk over the inverted file first touches the keyframes in.

What the model adds to the source is only what the device API declares (include/uvo/uvo.h): a keyframe's slot is its index in kfVec;
the score of a keyframe never scored is 0.0f; clear also empties kfVec; equal haloc distances keep kfVec order; a covisible without a
slot is None and skipped; and a table of the listed keyframes is kept for the comparison."""
import numpy as np

F32, F64 = np.float32, np.float64
LISTED, SCORED, ENTERED, RETAINED = 1, 2, 4, 8


def bits32(x):
    return int(np.array(x, np.float32).view(np.uint32))


class KeyFrame:
    def __init__(self, mn_id, ids, vals, hash_):
        self.mnId = int(mn_id)
        self.mBowVec = [(int(i), F64(v)) for i, v in zip(ids, vals)]        # std::map<WordId, WordValue>: ascending ids
        self.hash = [] if hash_ is None else [F32(x) for x in hash_]          # GetHalocVector()
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)
        self.best_covisibles = []                                               # GetBestCovisibilityKeyFrames(10)
        self.slot = -1


def lower_bound(vec, pos, key):
    """std::map::lower_bound on the sorted (id, value) list: index of the first element with id >= key"""
    lo, hi = 0, len(vec)
    while lo < hi:
        mid = (lo + hi) // 2
        if vec[mid][0] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def l1_score(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68)"""
    i1, i2 = 0, 0
    score = F64(0)
    while i1 != len(v1) and i2 != len(v2):
        vi, wi = v1[i1][1], v2[i2][1]
        if v1[i1][0] == v2[i2][0]:
            score = F64(score + F64(F64(F64(np.abs(F64(vi - wi))) - np.abs(vi)) - np.abs(wi)))
            i1 += 1
            i2 += 1
        elif v1[i1][0] < v2[i2][0]:
            i1 = lower_bound(v1, i1, v2[i2][0])
        else:
            i2 = lower_bound(v2, i2, v1[i1][0])
    score = F64(-score / F64(2.0))
    return score


def hash_match(h1, h2):
    """haloc::Hash::match (hash.cpp:189-205); EXIT_FAILURE is 1"""
    if len(h1) == 0 or len(h2) == 0:
        return F32(1)
    s = F32(0.0)
    with np.errstate(all="ignore"):
        for a, b in zip(h1, h2):
            s = F32(s + F32(np.abs(F32(a - b))))
    if np.isnan(s):
        return F32(1)
    return s


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}     # word -> list of keyframes, in add order
        self.kfVec = []
        self.table = None            # (maxCommonWords, minCommonWords, rows) of the last BoW query
        self.haloc = None            # per kfVec entry (m, kept) of the last haloc query

    # :39-46
    def add(self, kf):
        kf.slot = len(self.kfVec)
        self.kfVec.append(kf)
        for w, _ in kf.mBowVec:
            self.mvInvertedFile.setdefault(w, []).append(kf)
        return kf.slot

    # :48-67
    def erase(self, kf):
        for w, _ in kf.mBowVec:
            lKFs = self.mvInvertedFile.get(w, [])
            for k, x in enumerate(lKFs):
                if x is kf:
                    del lKFs[k]
                    break

    # :69-73, and kfVec with it (declared)
    def clear(self):
        self.mvInvertedFile = {}
        self.kfVec = []
        self.table, self.haloc = None, None

    def _rows(self, lKFs, words, score, minc, detail):
        rows = []
        for kf in lKFs:
            flags, best, acc = LISTED, -1, F32(0)
            if words(kf) > minc:
                flags |= SCORED
            if id(kf) in detail:
                acc, pbest, retained = detail[id(kf)]
                flags |= ENTERED | (RETAINED if retained else 0)
                best = pbest.slot
            rows.append((kf.slot, int(words(kf)), flags, best, bits32(score(kf)), bits32(acc)))
        return rows

    # :267-377
    def DetectRelocalisationCandidates(self, f_id, f_bow):
        F_bow = [(int(i), F64(v)) for i, v in zip(*f_bow)]
        lKFsSharingWords = []
        for w, _ in F_bow:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != f_id:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = f_id
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        self.table = (0, 0, [])
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F32(F32(maxCommonWords) * F32(0.8)))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F_bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        detail = {}
        words, score = (lambda kf: kf.mnRelocWords), (lambda kf: kf.mRelocScore)
        if not lScoreAndMatch:
            self.table = (maxCommonWords, minCommonWords, self._rows(lKFsSharingWords, words, score, minCommonWords, detail))
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        with np.errstate(all="ignore"):
            for si, pKFi in lScoreAndMatch:
                bestScore = si
                accScore = bestScore
                pBestKF = pKFi
                for pKF2 in pKFi.best_covisibles:
                    if pKF2 is None:
                        continue
                    if pKF2.mnRelocQuery != f_id:
                        continue
                    accScore = F32(accScore + pKF2.mRelocScore)
                    if pKF2.mRelocScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mRelocScore
                lAccScoreAndMatch.append((accScore, pBestKF, pKFi))
                if accScore > bestAccScore:
                    bestAccScore = accScore
            minScoreToRetain = F32(F32(0.75) * bestAccScore)
            spAlreadyAddedKF, vpRelocCandidates = set(), []
            for acc, pBest, pKFi in lAccScoreAndMatch:
                detail[id(pKFi)] = (acc, pBest, bool(acc > minScoreToRetain))
                if acc > minScoreToRetain:
                    if id(pBest) not in spAlreadyAddedKF:
                        vpRelocCandidates.append(pBest)
                        spAlreadyAddedKF.add(id(pBest))
        self.table = (maxCommonWords, minCommonWords, self._rows(lKFsSharingWords, words, score, minCommonWords, detail))
        return vpRelocCandidates

    # :144-265
    def DetectLoopCandidates(self, kf_id, kf_bow, connected, minScore):
        minScore = F32(minScore)
        KF_bow = [(int(i), F64(v)) for i, v in zip(*kf_bow)]
        spConnectedKeyFrames = set(id(k) for k in connected)
        lKFsSharingWords = []
        for w, _ in KF_bow:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnLoopQuery != kf_id:
                    pKFi.mnLoopWords = 0
                    if id(pKFi) not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = kf_id
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        self.table = (0, 0, [])
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(F32(F32(maxCommonWords) * F32(0.8)))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(l1_score(KF_bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        detail = {}
        words, score = (lambda kf: kf.mnLoopWords), (lambda kf: kf.mLoopScore)
        if not lScoreAndMatch:
            self.table = (maxCommonWords, minCommonWords, self._rows(lKFsSharingWords, words, score, minCommonWords, detail))
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        with np.errstate(all="ignore"):
            for si, pKFi in lScoreAndMatch:
                bestScore = si
                accScore = si
                pBestKF = pKFi
                for pKF2 in pKFi.best_covisibles:
                    if pKF2 is None:
                        continue
                    if pKF2.mnLoopQuery == kf_id and pKF2.mnLoopWords > minCommonWords:
                        accScore = F32(accScore + pKF2.mLoopScore)
                        if pKF2.mLoopScore > bestScore:
                            pBestKF = pKF2
                            bestScore = pKF2.mLoopScore
                lAccScoreAndMatch.append((accScore, pBestKF, pKFi))
                if accScore > bestAccScore:
                    bestAccScore = accScore
            minScoreToRetain = F32(F32(0.75) * bestAccScore)
            spAlreadyAddedKF, vpLoopCandidates = set(), []
            for acc, pBest, pKFi in lAccScoreAndMatch:
                detail[id(pKFi)] = (acc, pBest, bool(acc > minScoreToRetain))
                if acc > minScoreToRetain:
                    if id(pBest) not in spAlreadyAddedKF:
                        vpLoopCandidates.append(pBest)
                        spAlreadyAddedKF.add(id(pBest))
        self.table = (maxCommonWords, minCommonWords, self._rows(lKFsSharingWords, words, score, minCommonWords, detail))
        return vpLoopCandidates

    # :74-136; no_candidates is handed in as the caller assembled it (cluster_lc_found_ and the covisibles' ids)
    def DetectLoopCandidatesHaloc(self, kf_id, hash_q, no_candidates, maxScore):
        maxScore = F32(maxScore)
        hash_q = [] if hash_q is None else [F32(x) for x in hash_q]
        no_candidates = [int(x) for x in no_candidates]
        all_matchings = []
        self.haloc = []
        for kf in self.kfVec:
            if kf.mnId == kf_id or kf.mnId in no_candidates:
                self.haloc.append((bits32(F32(0)), 0))
                continue
            m = hash_match(hash_q, kf.hash)
            keep = bool(F64(m) < F64(F64(maxScore) * F64(0.8)))
            self.haloc.append((bits32(m), int(keep)))
            if keep:
                all_matchings.append((kf, m))
        all_matchings = sorted(all_matchings, key=lambda p: float(p[1]))     # stable: equal m keep kfVec order (declared)
        HalocMatches = []
        max_size = 3
        if max_size > len(all_matchings):
            max_size = len(all_matchings)
        else:
            for i in range(max_size):
                HalocMatches.append(all_matchings[i][0])
        return HalocMatches

    def state(self):
        return [(kf.mnLoopQuery, kf.mnRelocQuery, int(kf.mnLoopWords), int(kf.mnRelocWords), bits32(kf.mLoopScore), bits32(kf.mRelocScore)) for kf in self.kfVec]
