"""SearchByBoW on the GPU (include/mcs_matcher.h): relocalisation and loop detection matching.

  search_by_bow(f, kfs, ...)       ~ cORBmatcher::SearchByBoW(cMultiKeyFrame*, cMultiFrame&, ...)
                                     (reference src/cORBmatcher.cpp:179-323), frame `f` against a
                                     batch of candidate keyframes in one call
                                     (cTracking::Relocalisation, src/cTracking.cpp:1191-1203)
  search_by_bow_kf(kf1, kf2s, ...) ~ SearchByBoW(cMultiKeyFrame*, cMultiKeyFrame*, ...) (:885-966),
                                     `kf1` against a batch of loop candidates
                                     (cLoopClosing::ComputeSim3, src/cLoopClosing.cpp:285-304)
  feature_vector_device(...)       ~ the FeatureVector of TemplatedVocabulary::transform
                                     (TemplatedVocabulary.h:1126-1196) from the device output of
                                     Vocabulary.transform_words, without leaving the device

A frame is a dict: desc uint8 [n, bytes]; optional mask [n, bytes], angle float32 [n], has_mp
[n] (nonzero = holds a good map point); fv = (fv_node, fv_ptr, fv_feat) as
Vocabulary.transform / mcs_vocab_transform emit them, or a dict node -> feature list.
There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib


class BowSet(ctypes.Structure):
    """Mirror of mcs_bow_set: frames packed back to back."""
    _fields_ = [("n_frames", ctypes.c_int32), ("n_kp_total", ctypes.c_int32)] + \
               [(k, ctypes.c_void_p) for k in ("off", "desc", "mask", "angle", "has_mp", "fv_node",
                                               "fv_ptr", "fv_feat", "fv_n")]


_DTYPES = {"off": np.int32, "desc": np.uint8, "mask": np.uint8, "angle": np.float32,
           "has_mp": np.uint8, "fv_node": np.uint32, "fv_ptr": np.int32, "fv_feat": np.uint32,
           "fv_n": np.int32}


def th_low(nbytes, masked):
    """TH_LOW_ of the cORBmatcher ctor (src/cORBmatcher.cpp:46-65)."""
    return int(np.floor(nbytes)) if masked else 2 * int(nbytes)


def _fv_arrays(fv):
    if isinstance(fv, dict):
        node = np.array(sorted(fv), np.uint32)
        feat = [np.asarray(fv[int(k)], np.uint32) for k in node]
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in feat])]).astype(np.int32)
        return node, ptr, (np.concatenate(feat) if feat else np.zeros(0, np.uint32))
    node, ptr, feat = fv
    return np.asarray(node, np.uint32), np.asarray(ptr, np.int32), np.asarray(feat, np.uint32)


def pack(frames, nbytes, with_fv=True):
    """The packed arrays of mcs_bow_set for a list of frame dicts (see the header for the
    layout: frame k's FeatureVector at off[k], its fv_ptr at off[k] + k)."""
    n = [len(f["desc"]) for f in frames]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    tot, nf = int(off[-1]), len(frames)
    masked = [f.get("mask") is not None for f in frames]
    if masked and any(masked) != all(masked):
        raise ValueError("masks for every frame of a set or for none")
    p = {"n_frames": nf, "n_kp_total": tot, "off": off,
         "desc": np.zeros((tot, nbytes), np.uint8), "mask": np.zeros((tot, nbytes), np.uint8) if nf and masked[0] else None,
         "angle": np.zeros(tot, np.float32), "has_mp": np.zeros(tot, np.uint8)}
    if with_fv:
        p.update(fv_node=np.zeros(tot, np.uint32), fv_ptr=np.zeros(tot + nf, np.int32),
                 fv_feat=np.zeros(tot, np.uint32), fv_n=np.zeros(nf, np.int32))
    for k, f in enumerate(frames):
        o = int(off[k])
        p["desc"][o:o + n[k]] = np.asarray(f["desc"], np.uint8).reshape(n[k], nbytes)
        if p["mask"] is not None:
            p["mask"][o:o + n[k]] = np.asarray(f["mask"], np.uint8).reshape(n[k], nbytes)
        if f.get("angle") is not None:
            p["angle"][o:o + n[k]] = f["angle"]
        if f.get("has_mp") is not None:
            p["has_mp"][o:o + n[k]] = np.asarray(f["has_mp"]) != 0
        if with_fv:
            node, ptr, feat = _fv_arrays(f["fv"])
            m = len(node)
            if m > n[k] or len(feat) > n[k]:
                raise ValueError("FeatureVector larger than its frame")
            p["fv_n"][k] = m
            p["fv_node"][o:o + m] = node
            p["fv_ptr"][o + k:o + k + m + 1] = ptr[:m + 1]
            p["fv_feat"][o:o + len(feat)] = feat
    return p


def host_set(p):
    """(BowSet over the packed numpy arrays, the arrays to keep alive)."""
    s = BowSet(p["n_frames"], p["n_kp_total"])
    keep = []
    for k, dt in _DTYPES.items():
        a = p.get(k)
        if a is not None:
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            setattr(s, k, a.ctypes.data)
    return s, keep


def device_set(p, device=0):
    """(BowSet of device pointers, the torch tensors that own them)."""
    import torch
    s = BowSet(p["n_frames"], p["n_kp_total"])
    keep = {}
    for k, dt in _DTYPES.items():
        a = p.get(k)
        if a is None:
            continue
        a = np.ascontiguousarray(a, dt)
        if dt is np.uint32:
            a = a.view(np.int32)
        t = torch.from_numpy(a.copy()).to("cuda:%d" % device)
        keep[k] = t
        setattr(s, k, t.data_ptr())
    return s, keep


class Workspace(_Workspace):
    """mcs_bow_workspace: device scratch for frames of <= max_kp keypoints and batches of
    <= max_candidates candidates."""

    def __init__(self, max_kp, max_candidates, device=0):
        super().__init__("mcs_bow_workspace_create", "mcs_bow_workspace_destroy", device, max_kp, max_candidates)


def _stream(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def search_by_bow_device(ws, f_set, kf_set, nbytes, th, nnratio=0.75, check_orientation=False):
    """Device entry on BowSets of device pointers -> (match_f int32 [n_kf, n_f], n_matches
    int32 [n_kf]) torch tensors, stream-ordered on torch's current stream."""
    import torch
    dev = "cuda:%d" % ws.device
    m = torch.empty((kf_set.n_frames, f_set.n_kp_total), dtype=torch.int32, device=dev)
    n = torch.empty(kf_set.n_frames, dtype=torch.int32, device=dev)
    _check(lib().mcs_search_by_bow_device(ws._h, ctypes.byref(f_set), ctypes.byref(kf_set), int(nbytes), int(th),
                                          float(nnratio), int(bool(check_orientation)), m.data_ptr(),
                                          n.data_ptr(), _stream(ws.device)))
    return m, n


def search_by_bow_kf_device(ws, kf1_set, kf2_set, nbytes, th, nnratio=0.75):
    import torch
    dev = "cuda:%d" % ws.device
    m = torch.empty((kf2_set.n_frames, kf1_set.n_kp_total), dtype=torch.int32, device=dev)
    n = torch.empty(kf2_set.n_frames, dtype=torch.int32, device=dev)
    _check(lib().mcs_search_by_bow_kf_device(ws._h, ctypes.byref(kf1_set), ctypes.byref(kf2_set), int(nbytes),
                                             int(th), float(nnratio), m.data_ptr(), n.data_ptr(),
                                             _stream(ws.device)))
    return m, n


def _bytes_of(frames):
    return int(np.asarray(frames[0]["desc"]).shape[1])


def search_by_bow(f, kfs, th=None, nnratio=0.75, check_orientation=False, device=0, nbytes=None):
    """Overload A on host arrays: frame dict `f` against the list of keyframe dicts `kfs`
    -> (match_f [n_kf, n_f]: keyframe keypoint whose map point F's keypoint received or -1,
    n_matches [n_kf])."""
    nbytes = nbytes or _bytes_of([f])
    if th is None:
        th = th_low(nbytes, f.get("mask") is not None)
    fs, k1 = host_set(pack([f], nbytes))
    ks, k2 = host_set(pack(list(kfs), nbytes))
    m = np.full((len(kfs), fs.n_kp_total), -1, np.int32)
    n = np.zeros(len(kfs), np.int32)
    _check(lib().mcs_search_by_bow(int(device), ctypes.byref(fs), ctypes.byref(ks), nbytes, int(th),
                                   float(nnratio), int(bool(check_orientation)), m.ctypes.data, n.ctypes.data))
    return m, n


def search_by_bow_kf(kf1, kf2s, th=None, nnratio=0.75, device=0, nbytes=None):
    """Overload B on host arrays -> (matches12 [n_kf, n1]: KF2 keypoint index or -1,
    n_matches [n_kf])."""
    nbytes = nbytes or _bytes_of([kf1])
    if th is None:
        th = th_low(nbytes, kf1.get("mask") is not None)
    s1, k1 = host_set(pack([kf1], nbytes, with_fv=False))
    s2, k2 = host_set(pack(list(kf2s), nbytes, with_fv=False))
    m = np.full((len(kf2s), s1.n_kp_total), -1, np.int32)
    n = np.zeros(len(kf2s), np.int32)
    _check(lib().mcs_search_by_bow_kf(int(device), ctypes.byref(s1), ctypes.byref(s2), nbytes, int(th),
                                      float(nnratio), m.ctypes.data, n.ctypes.data))
    return m, n


def feature_vector_device(ws, node, weight):
    """torch int32 node [n] / float64 weight [n] on the GPU (Vocabulary.transform_words) ->
    (fv_node [n], fv_ptr [n + 1], fv_feat [n], fv_n [1]) torch int32 tensors on the GPU."""
    import torch
    n = int(node.shape[0])
    dev = node.device
    fv_node = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    fv_ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    fv_feat = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    fv_n = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(lib().mcs_feature_vector_device(ws._h, node.data_ptr(), weight.data_ptr(), n, fv_node.data_ptr(),
                                           fv_ptr.data_ptr(), fv_feat.data_ptr(), fv_n.data_ptr(),
                                           _stream(dev)))
    return fv_node, fv_ptr, fv_feat, fv_n


__all__ = ["BowSet", "Workspace", "pack", "host_set", "device_set", "th_low", "search_by_bow",
           "search_by_bow_kf", "search_by_bow_device", "search_by_bow_kf_device",
           "feature_vector_device", "McsError"]
