"""cORBmatcher::SearchBySim3 on the GPU (include/mcs_matcher.h): mutual projection matching of
one keyframe against a batch of loop candidates, each under its own Sim3 (reference
src/cORBmatcher.cpp:1721-1988, called at src/cLoopClosing.cpp:369).

  search_by_sim3(rig, kf1, pts1, kf2s, pts2s, active1, active2s, s12, R12, t12, th, th_high)
        host entry on NumPy -> (match1 [T, n1], match2 (list per candidate), matches12 [T, n1],
        n_found [T])
  search_by_sim3_device(ws, k1, p1, k2, p2, active1, active2, s12, R12, t12, th, th_high)
        the same on structs of device pointers and torch tensors, stream-ordered

rig      dict as mcs_amd.fuse: m_c, cam, mirror, grid_params, scale
keyframe dict as a Fuse target: kp_xy, kp_octave, kp_cam, desc, m_t; optional mask
points   dict per keyframe, one row per keypoint slot: pos [n, 3], dist [n, 2] (mfMinDistance,
         mfMaxDistance), desc uint8 [n, bytes] (the map point's descriptor); optional mask
active1  uint8 [T, n1], active2s: list of uint8 [n2_t]: pMP && !vbAlreadyMatched && !pMP->isBad()
There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib
from .fuse import _T_DTYPES, _T_INTS, FuseTargets, _device, _host, pack_targets


class Sim3Points(ctypes.Structure):
    """Mirror of mcs_sim3_points."""
    _fields_ = [("n", ctypes.c_int32)] + [(k, ctypes.c_void_p) for k in ("pos", "dist", "desc", "mask")]


_P_DTYPES = {"pos": np.float64, "dist": np.float64, "desc": np.uint8, "mask": np.uint8}


def th_high(nbytes, masked):
    """TH_HIGH_ of the cORBmatcher ctor (src/cORBmatcher.cpp:46-65)."""
    return int(np.floor(1.5 * nbytes)) if masked else 3 * nbytes


def pack_points(pts, nbytes):
    """The packed arrays of mcs_sim3_points for a list of per-keyframe point dicts (in the order
    of the keyframes of the set they belong to)."""
    n = sum(len(p["pos"]) for p in pts)
    masked = bool(pts) and pts[0].get("mask") is not None

    def cat(k, dt, w):
        rows = [np.asarray(p[k], dt).reshape(-1, w) for p in pts]
        return np.concatenate(rows) if rows else np.zeros((0, w), dt)
    return {"n": n, "pos": cat("pos", np.float64, 3), "dist": cat("dist", np.float64, 2),
            "desc": cat("desc", np.uint8, nbytes), "mask": cat("mask", np.uint8, nbytes) if masked else None}


def host_sets(pk, pp):
    """(FuseTargets, Sim3Points over the packed numpy arrays, the arrays to keep alive)."""
    ks, a = _host(FuseTargets, _T_INTS, _T_DTYPES, pk)
    ps, b = _host(Sim3Points, ("n",), _P_DTYPES, pp)
    return ks, ps, (a, b)


def device_sets(pk, pp, device=0):
    """(FuseTargets, Sim3Points of device pointers, the torch tensors that own them)."""
    ks, a = _device(FuseTargets, _T_INTS, _T_DTYPES, pk, device)
    ps, b = _device(Sim3Points, ("n",), _P_DTYPES, pp, device)
    return ks, ps, (a, b)


class Workspace(_Workspace):
    """mcs_sim3_workspace: device scratch for <= max_targets candidates of <= max_kp keypoints."""

    def __init__(self, max_targets, max_kp, device=0):
        super().__init__("mcs_sim3_workspace_create", "mcs_sim3_workspace_destroy", device, max_targets, max_kp)


def search_by_sim3_device(ws, k1, p1, k2, p2, active1, active2, s12, R12, t12, th, th_high, device=0, out=None):
    """Device entry.  k1 / k2: FuseTargets, p1 / p2: Sim3Points of device pointers; active1
    (uint8 [T, n1]), active2 (uint8 [n_kp_total]), s12 [T], R12 [T, 9], t12 [T, 3] (float64):
    torch tensors on the device -> (match1 [T, n1], match2 [n_kp_total], matches12 [T, n1],
    n_found [T]) int32 torch tensors, stream-ordered on torch's current stream."""
    import torch
    dev = "cuda:%d" % (ws.device if ws is not None else device)
    T, n1, n2 = k2.n_targets, k1.n_kp_total, k2.n_kp_total
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32, device=dev) for s in ((T, n1), (n2,), (T, n1), (T,)))
    m1, m2, m12, nf = out
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_search_by_sim3_device(ws._h if ws is not None else None, ctypes.byref(k1), ctypes.byref(p1),
                                           ctypes.byref(k2), ctypes.byref(p2), ptr(active1), ptr(active2),
                                           ptr(s12), ptr(R12), ptr(t12), float(th), int(th_high), ptr(m1), ptr(m2),
                                           ptr(m12), ptr(nf), torch.cuda.current_stream(dev).cuda_stream))
    return m1, m2, m12, nf


def pack_call(rig, kf1, pts1, kf2s, pts2s, active1, active2s, s12, R12, t12, nbytes, with_grid):
    """Packed keyframe sets, point sets and per-candidate arrays of one call."""
    T = len(kf2s)
    pk1, pk2 = pack_targets(rig, [kf1], nbytes, with_grid), pack_targets(rig, kf2s, nbytes, with_grid)
    pp1, pp2 = pack_points([pts1], nbytes), pack_points(pts2s, nbytes)
    n1 = pk1["n_kp_total"]
    a1 = np.ascontiguousarray(active1, np.uint8).reshape(T, n1)
    a2 = np.concatenate([np.asarray(a, np.uint8).reshape(-1) for a in active2s]) if T else np.zeros(0, np.uint8)
    return (pk1, pp1, pk2, pp2, a1, np.ascontiguousarray(a2),
            np.ascontiguousarray(s12, np.float64).reshape(T), np.ascontiguousarray(R12, np.float64).reshape(T, 9),
            np.ascontiguousarray(t12, np.float64).reshape(T, 3))


def search_by_sim3(rig, kf1, pts1, kf2s, pts2s, active1, active2s, s12, R12, t12, th, th_high, device=0,
                   nbytes=None):
    """Host entry (mcs_search_by_sim3) -> (match1 int32 [T, n1], match2: list of int32 [n2_t],
    matches12 int32 [T, n1], n_found int32 [T])."""
    nbytes = nbytes or int(np.asarray(kf1["desc"]).shape[1])
    pk1, pp1, pk2, pp2, a1, a2, s, R, t = pack_call(rig, kf1, pts1, kf2s, pts2s, active1, active2s, s12, R12, t12,
                                                    nbytes, False)
    k1, p1, keep1 = host_sets(pk1, pp1)
    k2, p2, keep2 = host_sets(pk2, pp2)
    T, n1, n2 = len(kf2s), pk1["n_kp_total"], pk2["n_kp_total"]
    m1, m2 = np.full((T, n1), -1, np.int32), np.full(max(n2, 1), -1, np.int32)
    m12, nf = np.full((T, n1), -1, np.int32), np.zeros(max(T, 1), np.int32)
    _check(lib().mcs_search_by_sim3(int(device), ctypes.byref(k1), ctypes.byref(p1), ctypes.byref(k2),
                                    ctypes.byref(p2), a1.ctypes.data, a2.ctypes.data, s.ctypes.data, R.ctypes.data,
                                    t.ctypes.data, float(th), int(th_high), m1.ctypes.data, m2.ctypes.data,
                                    m12.ctypes.data, nf.ctypes.data))
    off = pk2["off"]
    return m1, [m2[off[k]:off[k + 1]].copy() for k in range(T)], m12, nf[:T]


__all__ = ["Sim3Points", "Workspace", "pack_points", "pack_call", "host_sets", "device_sets", "search_by_sim3",
           "search_by_sim3_device", "th_high", "McsError"]
