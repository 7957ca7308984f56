"""cLocalMapping::CreateNewMapPoints on the GPU (include/mcs_newpoints.h): triangulate the matches
of SearchForTriangulationRaw and admit the new map points, neighbour by neighbour (reference
src/cLocalMapping.cpp:224-386, triangulate_point src/misc.cpp:26-51).

  create_new_map_points(rig, cur, neighbours, skip, kf2_first, E, has_mp, th_low, ...)
        host entry on NumPy -> dict: the created points, the updated flags, matches and verdicts
  pair_device(ws, kfs, i1, i2, n1, neighbour, matches12, kf2_first, has1, has2, verdict, out)
        the per-match loop of one neighbour on device pointers, stream-ordered
  create_device(ws, tri, kfs, n_kp, skip, kf2_first, E, has_mp, th_low, epi_thresh, ...)
        the whole neighbour loop (matcher -> pair kernels) on one stream

rig and keyframes are the dicts of mcs_amd.fuse (every keyframe with rays).  E float64
[T, C, C, 3, 3] is mcs_compute_e_rig per neighbour; has_mp a list of uint8 arrays, one per keyframe
(the current one first).  There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import MCS_ERR_CAPACITY, McsError, _Workspace, _check, lib
from .fuse import _T_DTYPES, _T_INTS, FuseTargets, _device, _host, pack_targets

NONE, CREATED, PARALLAX, BEHIND1, REPROJ1, BEHIND2, REPROJ2, DISTANCE = range(8)   # MCS_NP_*

_O_FIELDS = (("count", np.int32, 0), ("kp1", np.int32, 1), ("kp2", np.int32, 1), ("neighbour", np.int32, 1),
             ("pos", np.float64, 3), ("normal", np.float64, 3), ("min_dist", np.float64, 1),
             ("max_dist", np.float64, 1), ("desc", np.uint8, "b"), ("mask", np.uint8, "b"))


class NewPoints(ctypes.Structure):
    """Mirror of mcs_new_points."""
    _fields_ = [("cap", ctypes.c_int32)] + [(k, ctypes.c_void_p) for k, _, _ in _O_FIELDS]


def out_shapes(cap, nbytes, masked):
    """name -> (dtype, shape) of the buffers of mcs_new_points."""
    s = {}
    for k, dt, w in _O_FIELDS:
        if k == "mask" and not masked:
            continue
        s[k] = (dt, (1,) if w == 0 else (cap,) if w == 1 else (cap, nbytes if w == "b" else w))
    return s


class Workspace(_Workspace):
    """mcs_newpts_workspace: device scratch for a current keyframe of <= max_n1 keypoints."""

    def __init__(self, max_n1, device=0):
        super().__init__("mcs_newpts_workspace_create", "mcs_newpts_workspace_destroy", device, max_n1)


class TriWorkspace(_Workspace):
    """mcs_tri_workspace of the triangulation search the neighbour loop runs."""

    def __init__(self, max_n1, max_n2, device=0):
        super().__init__("mcs_tri_workspace_create", "mcs_tri_workspace_destroy", device, max_n1, max_n2)


def host_set(pk):
    """(FuseTargets over the packed numpy arrays, the arrays to keep alive)."""
    return _host(FuseTargets, _T_INTS, _T_DTYPES, pk)


def device_set(pk, device=0):
    """(FuseTargets of device pointers, the torch tensors that own them)."""
    return _device(FuseTargets, _T_INTS, _T_DTYPES, pk, device)


def new_out(cap, nbytes, masked, device=0, fill=0):
    """A NewPoints of fresh device tensors -> (NewPoints, tensors by name)."""
    import torch
    o, ts = NewPoints(), {}
    o.cap = cap
    for k, (dt, shp) in out_shapes(cap, nbytes, masked).items():
        shp = tuple(max(x, 1) for x in shp)
        t = torch.full(shp, fill, dtype=getattr(torch, np.dtype(dt).name), device="cuda:%d" % device)
        ts[k] = t
        setattr(o, k, t.data_ptr())
    return o, ts


def _stream(device):
    import torch
    return torch.cuda.current_stream("cuda:%d" % device).cuda_stream


def pair_device(ws, kfs, i1, i2, n1, neighbour, matches12, kf2_first, has1, has2, verdict, out, device=0):
    """mcs_new_points_pair_device on torch tensors, stream-ordered on torch's current stream."""
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_new_points_pair_device(ws._h if ws is not None else None, ctypes.byref(kfs), int(i1), int(i2),
                                            int(n1), int(neighbour), ptr(matches12), int(kf2_first), ptr(has1),
                                            ptr(has2), ptr(verdict), ctypes.byref(out), _stream(device)))


def create_device(ws, tri, kfs, n_kp, skip, kf2_first, E, has_mp, th_low, epi_thresh, out, matches12=None,
                  verdict=None, device=0):
    """mcs_create_new_map_points_device.  n_kp, skip, kf2_first: host sequences; E, has_mp, matches12,
    verdict: torch tensors on the device."""
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    nk = np.ascontiguousarray(n_kp, np.int32)
    sk, kf = np.ascontiguousarray(skip, np.uint8), np.ascontiguousarray(kf2_first, np.uint8)
    _check(lib().mcs_create_new_map_points_device(ws._h if ws is not None else None,
                                                  tri._h if tri is not None else None, ctypes.byref(kfs),
                                                  nk.ctypes.data, sk.ctypes.data, kf.ctypes.data, ptr(E), ptr(has_mp),
                                                  int(th_low), float(epi_thresh), ptr(matches12), ptr(verdict),
                                                  ctypes.byref(out), _stream(device)))


def create_new_map_points(rig, cur, neighbours, skip, kf2_first, E, has_mp, th_low, epi_thresh=1e-2, cap=None,
                          device=0, nbytes=None):
    """Host entry (mcs_create_new_map_points) -> dict: count, kp1, kp2, neighbour, pos, normal,
    min_dist, max_dist, desc, mask (None without masks) of the created points in creation order,
    has_mp (list per keyframe, updated), matches12 int32 [T, n1], verdict uint8 [T, n1] and
    capacity_exceeded (the first cap points are returned then)."""
    nbytes = nbytes or int(np.asarray(cur["desc"]).shape[1])
    kfs = [cur] + list(neighbours)
    pk = pack_targets(rig, kfs, nbytes, False)
    ks, keep = host_set(pk)
    T, n1, off = len(neighbours), len(cur["kp_xy"]), pk["off"]
    masked = pk["mask"] is not None
    cap = n1 * max(T, 1) if cap is None else int(cap)
    o, arrs = NewPoints(), {}
    o.cap = cap
    for k, (dt, shp) in out_shapes(cap, nbytes, masked).items():
        arrs[k] = np.zeros(shp, dt)
        setattr(o, k, arrs[k].ctypes.data)
    sk, kf = np.ascontiguousarray(skip, np.uint8).reshape(T), np.ascontiguousarray(kf2_first, np.uint8).reshape(T)
    Eh = np.ascontiguousarray(E, np.float64).reshape(T, -1)
    has = np.ascontiguousarray(np.concatenate([np.asarray(h, np.uint8).reshape(-1) for h in has_mp]))
    m12, vd = np.full((T, n1), -1, np.int32), np.zeros((T, n1), np.uint8)
    rc = lib().mcs_create_new_map_points(int(device), ctypes.byref(ks), sk.ctypes.data, kf.ctypes.data,
                                         Eh.ctypes.data, has.ctypes.data, int(th_low), float(epi_thresh),
                                         m12.ctypes.data, vd.ctypes.data, ctypes.byref(o))
    if rc != MCS_ERR_CAPACITY:
        _check(rc)
    n = min(int(arrs["count"][0]), cap)
    out = {k: (a[:n].copy() if k != "count" else int(a[0])) for k, a in arrs.items()}
    out.setdefault("mask", None)
    out.update(has_mp=[has[off[t]:off[t + 1]].copy() for t in range(T + 1)], matches12=m12, verdict=vd,
               capacity_exceeded=rc == MCS_ERR_CAPACITY)
    return out


__all__ = ["NewPoints", "Workspace", "TriWorkspace", "out_shapes", "host_set", "device_set", "new_out", "pair_device",
           "create_device", "create_new_map_points", "NONE", "CREATED", "PARALLAX", "BEHIND1", "REPROJ1", "BEHIND2",
           "REPROJ2", "DISTANCE", "McsError"]
