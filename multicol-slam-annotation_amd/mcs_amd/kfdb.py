"""cMultiKeyFrameDatabase on the GPU (include/mcs_kfdb.h): loop and relocalisation candidates from
the BowVectors of the added keyframes (reference src/cMultiKeyFrameDatabase.cpp:43-340,
L1Scoring::score ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-68, the minScore loop of
cLoopClosing::DetectLoop src/cLoopClosing.cpp:141-157).

  KeyFrameDatabase(voc | n_words, max_keyframes, max_entries)
      add_device(bow_word, bow_value, bow_n, n_upper)   -> slot      torch tensors, stream-ordered
      erase(slot) / clear()
      min_score_device(query, slots, out)               cLoopClosing.cpp:144-157
      detect_loop_device(query, query_id, connected, min_score, neigh, result)
      detect_reloc_device(query, query_id, neigh, result)
      members()                                          the six members per slot, as numpy
      min_score / detect_loop / detect_reloc             host entries on NumPy

A query is (word int32, value float64, n int32[1]) torch tensors as Vocabulary.bow_vector returns
them.  There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import MCS_ERR_CAPACITY, McsError, _check, lib

NEIGH = 10   # MCS_KFDB_NEIGH


class Query(ctypes.Structure):
    """Mirror of mcs_kfdb_query."""
    _fields_ = [("d_word", ctypes.c_void_p), ("d_value", ctypes.c_void_p), ("d_n", ctypes.c_void_p),
                ("cap", ctypes.c_int32)]


class Result(ctypes.Structure):
    """Mirror of mcs_kfdb_result."""
    _fields_ = [("d_candidates", ctypes.c_void_p), ("cap", ctypes.c_int32), ("d_n_candidates", ctypes.c_void_p),
                ("d_common", ctypes.c_void_p), ("d_score", ctypes.c_void_p)]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _np(a):
    return a.ctypes.data if a is not None else None


def query_of(word, value, n):
    """Query over torch tensors (word int32 / value float64 [cap], n int32 [1])."""
    return Query(_ptr(word), _ptr(value), _ptr(n), int(word.shape[0]))


def new_result(cap, n_slots, device=0, diagnostics=True):
    """A Result of fresh device tensors -> (Result, tensors by name)."""
    import torch
    dev = "cuda:%d" % device
    ts = {"candidates": torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev),
          "n_candidates": torch.zeros(1, dtype=torch.int32, device=dev)}
    if diagnostics:
        ts["common"] = torch.zeros(max(n_slots, 1), dtype=torch.int32, device=dev)
        ts["score"] = torch.zeros(max(n_slots, 1), dtype=torch.float64, device=dev)
    return Result(_ptr(ts["candidates"]), int(cap), _ptr(ts["n_candidates"]), _ptr(ts.get("common")),
                  _ptr(ts.get("score"))), ts


class KeyFrameDatabase:
    """mcs_kfdb: the database of one vocabulary on one GPU."""

    def __init__(self, voc, max_keyframes, max_entries, device=0, scoring=0):
        """voc: a mcs_amd.vocab.Vocabulary, or the number of words (with `scoring`)."""
        h = ctypes.c_void_p()
        if isinstance(voc, (int, np.integer)):
            _check(lib().mcs_kfdb_create_n(int(device), int(voc), int(scoring), int(max_keyframes),
                                           int(max_entries), ctypes.byref(h)))
        else:
            _check(lib().mcs_kfdb_create(int(device), voc._h, int(max_keyframes), int(max_entries),
                                         ctypes.byref(h)))
        self._h, self.device = h, device

    def close(self):
        if getattr(self, "_h", None):
            lib().mcs_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(lib().mcs_kfdb_size(self._h))

    def _stream(self):
        import torch
        return torch.cuda.current_stream("cuda:%d" % self.device).cuda_stream

    def add_device(self, bow_word, bow_value, bow_n, n_upper=None, reloc_score_init=0.0):
        """add(pKF) -> slot.  n_upper bounds the device count bow_n (default: the buffers' size)."""
        slot = ctypes.c_int32(-1)
        n_upper = int(bow_word.shape[0]) if n_upper is None else int(n_upper)
        _check(lib().mcs_kfdb_add_device(self._h, _ptr(bow_word), _ptr(bow_value), _ptr(bow_n), n_upper,
                                         float(reloc_score_init), ctypes.byref(slot), self._stream()))
        return slot.value

    def add(self, word, value, reloc_score_init=0.0):
        """add(pKF) from host arrays -> slot."""
        w, v = self._q(word, value)
        slot = ctypes.c_int32(-1)
        _check(lib().mcs_kfdb_add(self._h, _np(w), _np(v), len(w), float(reloc_score_init), ctypes.byref(slot)))
        return slot.value

    def erase(self, slot):
        _check(lib().mcs_kfdb_erase(self._h, int(slot), self._stream()))

    def clear(self):
        _check(lib().mcs_kfdb_clear(self._h, self._stream()))

    def min_score_device(self, query, slots, out):
        """slots int32 [n] and out float64 [1]: torch tensors on the device."""
        _check(lib().mcs_kfdb_min_score_device(self._h, ctypes.byref(query), _ptr(slots), int(slots.shape[0]),
                                               _ptr(out), self._stream()))

    def detect_loop_device(self, query, query_id, connected, min_score, neigh, result):
        """connected uint8 [size], min_score float64 [1], neigh int32 [size, 10]: torch tensors."""
        _check(lib().mcs_kfdb_detect_loop_device(self._h, ctypes.byref(query), int(query_id), _ptr(connected),
                                                 _ptr(min_score), _ptr(neigh), ctypes.byref(result),
                                                 self._stream()))

    def detect_reloc_device(self, query, query_id, neigh, result):
        _check(lib().mcs_kfdb_detect_reloc_device(self._h, ctypes.byref(query), int(query_id), _ptr(neigh),
                                                  ctypes.byref(result), self._stream()))

    def members(self):
        """dict of numpy arrays [size]: loop_query, loop_words, loop_score, reloc_query, reloc_words,
        reloc_score (synchronises)."""
        import torch
        n, dev = max(len(self), 1), "cuda:%d" % self.device
        names = ("loop_query", "loop_words", "loop_score", "reloc_query", "reloc_words", "reloc_score")
        dts = (torch.int64, torch.int32, torch.float64) * 2
        ts = [torch.zeros(n, dtype=dt, device=dev) for dt in dts]
        _check(lib().mcs_kfdb_members_device(self._h, *[t.data_ptr() for t in ts], self._stream()))
        return {k: t.cpu().numpy()[:len(self)] for k, t in zip(names, ts)}

    # ---- host entries on NumPy

    @staticmethod
    def _q(word, value):
        w = np.ascontiguousarray(word, np.uint32).reshape(-1)
        v = np.ascontiguousarray(value, np.float64).reshape(-1)
        return w, v

    def min_score(self, word, value, slots):
        w, v = self._q(word, value)
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = ctypes.c_double()
        _check(lib().mcs_kfdb_min_score(self._h, _np(w), _np(v), len(w), _np(s), len(s), ctypes.byref(out)))
        return out.value

    def _detect(self, loop, word, value, query_id, connected, min_score, neigh, cap):
        w, v = self._q(word, value)
        n = len(self)
        cap = n if cap is None else int(cap)
        ng = np.ascontiguousarray(neigh, np.int32).reshape(n, NEIGH)
        cand, nc = np.full(max(cap, 1), -1, np.int32), ctypes.c_int32()
        common, score = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        if loop:
            cn = np.ascontiguousarray(connected, np.uint8).reshape(n)
            rc = lib().mcs_kfdb_detect_loop(self._h, _np(w), _np(v), len(w), int(query_id), _np(cn),
                                            float(min_score), _np(ng), _np(cand), cap, ctypes.byref(nc),
                                            _np(common), _np(score))
        else:
            rc = lib().mcs_kfdb_detect_reloc(self._h, _np(w), _np(v), len(w), int(query_id), _np(ng), _np(cand),
                                             cap, ctypes.byref(nc), _np(common), _np(score))
        if rc != MCS_ERR_CAPACITY:
            _check(rc)
        return {"candidates": cand[:min(nc.value, cap)].copy(), "n_candidates": nc.value, "common": common[:n],
                "score": score[:n], "capacity_exceeded": rc == MCS_ERR_CAPACITY}

    def detect_loop(self, word, value, query_id, connected, min_score, neigh, cap=None):
        return self._detect(True, word, value, query_id, connected, min_score, neigh, cap)

    def detect_reloc(self, word, value, query_id, neigh, cap=None):
        return self._detect(False, word, value, query_id, None, 0.0, neigh, cap)


__all__ = ["KeyFrameDatabase", "Query", "Result", "query_of", "new_result", "NEIGH", "McsError"]
