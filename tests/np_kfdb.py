"""Plain Python restatement of the keyframe database (test infrastructure only).

Written after the reference text, container for container: an inverted file of lists, the lists
lKFsSharingWords / lScoreAndMatch / lAccScoreAndMatch, the set spAlreadyAddedKF and the six members
per keyframe (reference src/cMultiKeyFrameDatabase.cpp:43-340, L1Scoring::score
ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-68, cLoopClosing.cpp:141-157, BowVector.cpp:34-86,
TemplatedVocabulary.h:1126-1196).  Python floats are IEEE doubles and every expression below keeps
the reference's operand order, so the values agree with it to the bit.
"""
import bisect

import numpy as np

NEIGH = 10


def bow_vector(word, weight, weighting=0, scoring=0):
    """The BowVector half of transform(features, v, fv, levelsup) from per-descriptor word / weight
    -> (bow_word uint32 ascending, bow_value float64)."""
    tf = weighting in (0, 1)
    v = {}
    for wid, w in zip(np.asarray(word).tolist(), np.asarray(weight, np.float64).tolist()):
        if w > 0:
            if tf:
                if wid in v:
                    v[wid] += w          # addWeight
                else:
                    v[wid] = w
            elif wid not in v:           # addIfNotExist
                v[wid] = w
    keys = sorted(v)
    must, l2 = scoring != 5, scoring == 1
    if tf and keys and not must:
        nd = float(len(keys))
        for k in keys:
            v[k] /= nd
    if must:                             # BowVector::normalize
        norm = 0.0
        if not l2:
            for k in keys:
                norm += abs(v[k])
        else:
            for k in keys:
                norm += v[k] * v[k]
            norm = float(np.sqrt(np.float64(norm)))
        if norm > 0.0:
            for k in keys:
                v[k] /= norm
    return np.array(keys, np.uint32), np.array([v[k] for k in keys], np.float64)


def l1_score(w1, v1, w2, v2):
    """L1Scoring::score(v1, v2) over sorted (word, value) lists, with its lower_bound walk."""
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = v1[i], v2[j]
        if w1[i] == w2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j])
        else:
            j = bisect.bisect_left(w2, w1[i])
    return -score / 2.0


class KeyFrame:
    def __init__(self, slot, word, value, score_init):
        self.slot = slot
        self.word = [int(x) for x in word]
        self.value = [float(x) for x in value]
        self.loop_query, self.loop_words, self.loop_score = 0, 0, float(score_init)
        self.reloc_query, self.reloc_words, self.reloc_score = 0, 0, float(score_init)


class Database:
    """cMultiKeyFrameDatabase with keyframes named by slot (the add sequence number)."""

    def __init__(self):
        self.inverted = {}     # word -> list of KeyFrame, in add order
        self.kfs = []          # every keyframe ever added (an erased one keeps its members)
        self.alive = []

    def add(self, word, value, reloc_score_init=0.0):
        kf = KeyFrame(len(self.kfs), word, value, reloc_score_init)
        self.kfs.append(kf)
        self.alive.append(True)
        for w in kf.word:
            self.inverted.setdefault(w, []).append(kf)
        return kf.slot

    def erase(self, slot):
        kf = self.kfs[slot]
        if not self.alive[slot]:
            return
        self.alive[slot] = False
        for w in kf.word:
            self.inverted[w].remove(kf)

    def members(self):
        names = (("loop_query", np.int64), ("loop_words", np.int32), ("loop_score", np.float64),
                 ("reloc_query", np.int64), ("reloc_words", np.int32), ("reloc_score", np.float64))
        return {k: np.array([getattr(kf, k) for kf in self.kfs], dt) for k, dt in names}

    def score(self, qw, qv, slot):
        kf = self.kfs[slot]
        return l1_score(qw, qv, kf.word, kf.value)

    def min_score(self, qw, qv, slots):
        """cLoopClosing.cpp:144-157; slots outside the database are skipped."""
        qw, qv = [int(x) for x in qw], [float(x) for x in qv]
        m = 1.0
        for s in slots:
            if s < 0 or s >= len(self.kfs):
                continue
            sc = self.score(qw, qv, s)
            if sc < m:
                m = sc
        return m

    def _diagnostics(self, qw, qv):
        common = np.zeros(len(self.kfs), np.int32)
        score = np.zeros(len(self.kfs), np.float64)
        qs = set(qw)
        for kf in self.kfs:
            if self.alive[kf.slot]:
                common[kf.slot] = sum(1 for w in kf.word if w in qs)
                score[kf.slot] = self.score(qw, qv, kf.slot)
            else:
                score[kf.slot] = -0.0
        return common, score

    def _neighbours(self, neigh, slot):
        return [self.kfs[s] for s in np.asarray(neigh[slot]).tolist() if 0 <= s < len(self.kfs)]

    def detect_loop(self, qw, qv, query_id, connected, min_score, neigh):
        """DetectLoopCandidates (:82-221) -> dict(candidates, common, score)."""
        qw, qv = [int(x) for x in qw], [float(x) for x in qv]
        common, diag = self._diagnostics(qw, qv)
        out = {"candidates": [], "common": common, "score": diag}
        sharing = []
        for w in qw:
            for kf in self.inverted.get(w, []):
                if kf.loop_query != query_id:
                    kf.loop_words = 0
                    if not connected[kf.slot]:
                        kf.loop_query = query_id
                        sharing.append(kf)
                kf.loop_words += 1
        if not sharing:
            return out
        max_common = 0
        for kf in sharing:
            if kf.loop_words > max_common:
                max_common = kf.loop_words
        min_common = int(float(max_common) * 0.8)
        score_and_match = []
        for kf in sharing:
            if kf.loop_words > min_common:
                si = self.score(qw, qv, kf.slot)
                kf.loop_score = si
                if si >= min_score:
                    score_and_match.append((si, kf))
        if not score_and_match:
            return out
        acc_and_match = []
        best_acc = min_score
        for si, kf in score_and_match:
            best_score, acc, best_kf = si, si, kf
            for kf2 in self._neighbours(neigh, kf.slot):
                if kf2.loop_query == query_id and kf2.loop_words > min_common:
                    acc += kf2.loop_score
                    if kf2.loop_score > best_score:
                        best_kf = kf2
                        best_score = kf2.loop_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = 0.75 * best_acc
        added = set()
        for acc, kf in acc_and_match:
            if acc > retain and kf.slot not in added:
                out["candidates"].append(kf.slot)
                added.add(kf.slot)
        return out

    def detect_reloc(self, qw, qv, query_id, neigh):
        """DetectRelocalisationCandidates (:223-340) -> dict(candidates, common, score)."""
        qw, qv = [int(x) for x in qw], [float(x) for x in qv]
        common, diag = self._diagnostics(qw, qv)
        out = {"candidates": [], "common": common, "score": diag}
        sharing = []
        for w in qw:
            for kf in self.inverted.get(w, []):
                if kf.reloc_query != query_id:
                    kf.reloc_words = 0
                    kf.reloc_query = query_id
                    sharing.append(kf)
                kf.reloc_words += 1
        if not sharing:
            return out
        max_common = 0
        for kf in sharing:
            if kf.reloc_words > max_common:
                max_common = kf.reloc_words
        min_common = int(max_common * 0.8)
        score_and_match = []
        for kf in sharing:
            if kf.reloc_words > min_common:
                si = self.score(qw, qv, kf.slot)
                kf.reloc_score = si
                score_and_match.append((si, kf))
        if not score_and_match:
            return out
        acc_and_match = []
        best_acc = 0.0
        for si, kf in score_and_match:
            best_score, acc, best_kf = si, si, kf
            for kf2 in self._neighbours(neigh, kf.slot):
                if kf2.reloc_query != query_id:
                    continue
                acc += kf2.reloc_score
                if kf2.reloc_score > best_score:
                    best_kf = kf2
                    best_score = kf2.reloc_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = 0.75 * best_acc
        added = set()
        for acc, kf in acc_and_match:
            if acc > retain and kf.slot not in added:
                out["candidates"].append(kf.slot)
                added.add(kf.slot)
        return out
