"""cSim3Solver on the GPU (include/mcs_matcher.h): the loop-closing Sim3 RANSAC of one keyframe
against a batch of loop candidates (reference src/cSim3Solver.cpp, called at
src/cLoopClosing.cpp:311-364 between SearchByBoW and SearchBySim3).

  draw_samples(n, draws)      the correspondence triples of :202-222 from the dis(gen) values (host)
  sim3_solver(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first1, first2s, sigma2, samples,
              n_iterations, prob, min_inliers, max_its_cap, ...)
        host entry on NumPy -> dict: the constructor's rows, the RANSAC state and outputs, and
        active1 / active2 for SearchBySim3 when good1 / good2s are given
  prepare_device / iterate_device / active_device
        the same on structs of device pointers and torch tensors, stream-ordered

rig, keyframes and points are the dicts of mcs_amd.sim3_match; of the points only pos is read.
matches12 int32 [T, n1] is the output of search_by_bow_kf; ok1 uint8 [n1], ok2s list of uint8
[n2_t]; first1 int32 [n1], first2s list of int32 [n2_t]; samples int32 [T, max_its_cap, 3].
There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib
from .fuse import pack_targets
from .sim3_match import device_sets, host_sets, pack_points

SET_PARAMS, INIT = 1, 2         # MCS_SIM3_SET_PARAMS, MCS_SIM3_INIT

_C_FIELDS = (("n", np.int32, 0), ("idx1", np.int32, 1), ("X1", np.float64, 3), ("X2", np.float64, 3),
             ("p1", np.float64, 2), ("p2", np.float64, 2), ("cam1", np.int32, 1), ("cam2", np.int32, 1),
             ("maxerr1", np.float64, 1), ("maxerr2", np.float64, 1))
_R_STATE = (("iterations", np.int32, 1), ("best_inliers", np.int32, 1), ("max_its", np.int32, 1),
            ("best_words", np.uint64, "W"), ("s12", np.float64, 1), ("R12", np.float64, 9), ("t12", np.float64, 3),
            ("T12", np.float64, 16))
_R_OUT = (("success", np.int32, 1), ("no_more", np.int32, 1), ("n_inliers", np.int32, 1), ("inlier", np.uint8, "n1"))


class Sim3Corr(ctypes.Structure):
    """Mirror of mcs_sim3_corr."""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_targets", "cap", "n_cams")] + \
               [(k, ctypes.c_void_p) for k in ("m_c", "cam")] + [(k, ctypes.c_void_p) for k, _, _ in _C_FIELDS]


class Sim3Ransac(ctypes.Structure):
    """Mirror of mcs_sim3_ransac."""
    _fields_ = [(k, ctypes.c_void_p) for k, _, _ in _R_STATE + _R_OUT] + \
               [("hyp_srt", ctypes.c_void_p), ("hyp_inl", ctypes.c_void_p)]


def draw_samples(n, draws):
    """mcs_sim3_draw_samples: draws int [n_its, 3] in [0, n) -> samples int32 [n_its, 3]."""
    d = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
    out = np.zeros_like(d)
    _check(lib().mcs_sim3_draw_samples(int(n), d.ctypes.data, len(d), out.ctypes.data))
    return out


def corr_shapes(T, n1):
    """name -> (dtype, shape) of the buffers of mcs_sim3_corr."""
    return {k: (dt, (T,) if w == 0 else (T, n1) if w == 1 else (T, n1, w)) for k, dt, w in _C_FIELDS}


def ransac_shapes(T, n1, n_iterations):
    """name -> (dtype, shape) of the buffers of mcs_sim3_ransac."""
    dims = {"W": (n1 + 63) // 64, "n1": n1}
    s = {k: (dt, (T,) if w == 1 else (T, dims.get(w, w))) for k, dt, w in _R_STATE + _R_OUT}
    s["hyp_srt"] = (np.float64, (T, n_iterations, 13))
    s["hyp_inl"] = (np.int32, (T, n_iterations))
    return s


def _np_struct(struct, shapes, given=None, skip=()):
    s, arrs = struct(), {}
    for k, (dt, shp) in shapes.items():
        if k in skip:
            continue
        a = np.zeros(shp, dt) if given is None or given.get(k) is None else np.ascontiguousarray(given[k], dt).reshape(shp)
        arrs[k] = a
        setattr(s, k, a.ctypes.data)
    return s, arrs


def _torch_struct(struct, shapes, dev, given=None, skip=()):
    import torch
    s, ts = struct(), {}
    for k, (dt, shp) in shapes.items():
        if k in skip:
            continue
        if given is not None and given.get(k) is not None:
            t = given[k]
        else:
            # uint64 is carried as int64 (same bits)
            t = torch.zeros(shp, dtype=getattr(torch, np.dtype(np.int64 if dt is np.uint64 else dt).name), device=dev)
        ts[k] = t
        setattr(s, k, t.data_ptr())
    return s, ts


class Workspace(_Workspace):
    """mcs_sim3_solver_workspace: scratch for <= max_targets candidates of <= max_kp correspondences
    and calls of <= max_its_cap iterations."""

    def __init__(self, max_targets, max_kp, max_its_cap, device=0):
        super().__init__("mcs_sim3_solver_workspace_create", "mcs_sim3_solver_workspace_destroy", device,
                         max_targets, max_kp, max_its_cap)


def pack_call(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first1, first2s, nbytes=None):
    """Packed keyframe sets, point sets and the per-slot arrays of one call ->
    (pk1, pp1, pk2, pp2, matches12 [T, n1], ok1, ok2, first1, first2)."""
    nbytes = nbytes or int(np.asarray(kf1["desc"]).shape[1])
    T = len(kf2s)
    pk1, pk2 = pack_targets(rig, [kf1], nbytes, False), pack_targets(rig, kf2s, nbytes, False)
    pp1, pp2 = pack_points([pts1], nbytes), pack_points(pts2s, nbytes)
    n1 = pk1["n_kp_total"]
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])  # noqa: E731
                                              if len(xs) else np.zeros(0, dt))
    return (pk1, pp1, pk2, pp2, np.ascontiguousarray(matches12, np.int32).reshape(T, n1),
            np.ascontiguousarray(ok1, np.uint8).reshape(n1), cat(ok2s, np.uint8),
            np.ascontiguousarray(first1, np.int32).reshape(n1), cat(first2s, np.int32))


def new_corr(k1, T, device=0, given=None):
    """A Sim3Corr of fresh device tensors for T candidates of k1 (FuseTargets of device pointers),
    projecting with k1's rig -> (Sim3Corr, tensors by name)."""
    c, ts = _torch_struct(Sim3Corr, corr_shapes(T, k1.n_kp_total), "cuda:%d" % device, given)
    c.n_targets, c.cap, c.n_cams, c.m_c, c.cam = T, k1.n_kp_total, k1.n_cams, k1.m_c, k1.cam
    return c, ts


def new_ransac(T, n1, n_iterations, device=0, hyp=True, given=None):
    """A Sim3Ransac of fresh device tensors -> (Sim3Ransac, tensors by name)."""
    return _torch_struct(Sim3Ransac, ransac_shapes(T, n1, n_iterations), "cuda:%d" % device, given,
                         () if hyp else ("hyp_srt", "hyp_inl"))


def _stream(device):
    import torch
    return torch.cuda.current_stream("cuda:%d" % device).cuda_stream


def prepare_device(k1, p1, k2, p2, matches12, ok1, ok2, first1, first2, sigma2, corr, device=0):
    """mcs_sim3_solver_prepare_device on torch tensors, stream-ordered on torch's current stream."""
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_sim3_solver_prepare_device(ctypes.byref(k1), ctypes.byref(p1), ctypes.byref(k2), ctypes.byref(p2),
                                                ptr(matches12), ptr(ok1), ptr(ok2), ptr(first1), ptr(first2),
                                                ptr(sigma2), ctypes.byref(corr), _stream(device)))


def iterate_device(ws, corr, samples, n_iterations, prob, min_inliers, max_its_cap, flags, ransac, device=0):
    """mcs_sim3_solver_iterate_device; samples int32 [T, max_its_cap, 3] on the device."""
    _check(lib().mcs_sim3_solver_iterate_device(ws._h if ws is not None else None, ctypes.byref(corr),
                                                samples.data_ptr() if samples is not None else None,
                                                int(n_iterations), float(prob), int(min_inliers), int(max_its_cap),
                                                int(flags), ctypes.byref(ransac), _stream(device)))


def active_device(k1, k2, inlier, good1, good2, matches12, first2, active1, active2, device=0):
    """mcs_sim3_solver_active_device: active1 uint8 [T, n1], active2 uint8 [n_kp_total] are written."""
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_sim3_solver_active_device(ctypes.byref(k1), ctypes.byref(k2), ptr(inlier), ptr(good1), ptr(good2),
                                               ptr(matches12), ptr(first2), ptr(active1), ptr(active2),
                                               _stream(device)))


def sim3_solver(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first1, first2s, sigma2, samples, n_iterations,
                prob=0.99, min_inliers=6, max_its_cap=300, flags=INIT, state=None, good1=None, good2s=None, device=0):
    """Host entry (mcs_sim3_solver) -> dict with the arrays of mcs_sim3_corr and mcs_sim3_ransac by
    name and, when good1 / good2s are given, active1 [T, n1] and active2 (list per candidate).
    state: the dict of an earlier call, to go on from it (flags = 0)."""
    pk1, pp1, pk2, pp2, m12, o1, o2, f1, f2 = pack_call(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first1,
                                                        first2s)
    k1, p1, keep1 = host_sets(pk1, pp1)
    k2, p2, keep2 = host_sets(pk2, pp2)
    T, n1, n2 = len(kf2s), pk1["n_kp_total"], pk2["n_kp_total"]
    corr, ca = _np_struct(Sim3Corr, corr_shapes(T, n1))
    corr.n_targets, corr.cap, corr.n_cams = T, n1, k1.n_cams
    keys = [k for k, _, _ in _R_STATE]
    ran, ra = _np_struct(Sim3Ransac, ransac_shapes(T, n1, n_iterations),
                         None if state is None else {k: state[k] for k in keys})
    sig = np.ascontiguousarray(sigma2, np.float64)
    smp = np.ascontiguousarray(samples, np.int32).reshape(T, max_its_cap, 3)
    hand = good1 is not None
    g1 = np.ascontiguousarray(good1, np.uint8).reshape(n1) if hand else None
    g2 = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8).reshape(-1) for g in good2s])
                              if hand and T else np.zeros(0, np.uint8))
    a1, a2 = np.zeros((T, n1), np.uint8), np.zeros(max(n2, 1), np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None and hand else None  # noqa: E731
    _check(lib().mcs_sim3_solver(int(device), ctypes.byref(k1), ctypes.byref(p1), ctypes.byref(k2), ctypes.byref(p2),
                                 m12.ctypes.data, o1.ctypes.data, o2.ctypes.data, f1.ctypes.data, f2.ctypes.data,
                                 sig.ctypes.data, smp.ctypes.data, int(n_iterations), float(prob), int(min_inliers),
                                 int(max_its_cap), int(flags), ctypes.byref(corr), ctypes.byref(ran), ptr(g1), ptr(g2),
                                 ptr(a1), ptr(a2)))
    out = dict(ca, **ra)
    if hand:
        off = pk2["off"]
        out["active1"], out["active2"] = a1, [a2[off[k]:off[k + 1]].copy() for k in range(T)]
    return out


__all__ = ["Sim3Corr", "Sim3Ransac", "Workspace", "draw_samples", "corr_shapes", "ransac_shapes", "pack_call",
           "device_sets", "host_sets", "new_corr", "new_ransac", "prepare_device", "iterate_device", "active_device",
           "sim3_solver", "SET_PARAMS", "INIT", "McsError"]
