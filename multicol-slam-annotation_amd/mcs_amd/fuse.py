"""cORBmatcher::Fuse on the GPU (include/mcs_matcher.h): map-point fusion of local mapping and
loop closing, one query set of map points against a batch of target keyframes per call.

  fuse(rule, rig, targets, queries, ...)  ~ the projection / window / best-distance part of
        Fuse(pKF, curKF, vpMapPoints, th)   rule 0  (reference src/cORBmatcher.cpp:1265-1418)
        Fuse(pKF, vpMapPoints, th)          rule 1  (:1420-1567)
        Fuse(pKF, Scw, vpPoints, th)        rule 2  (:1570-1719)
      for every (target, query, camera) -> best_kp, best_dist, epi_ok   (host arrays)
  fuse_device(ws, rule, tset, qset, ...)  ~ the same on device pointers, stream-ordered
  fuse_select(rule, q_mp, best_kp, ...)   ~ the state-dependent tail of one target on the host
        (:1379-1415, :1536-1563, :1692-1715): action list, nFused, the target's end state

rig     dict: m_c [C, 4, 4], cam [C, 17] (c d e u0 v0 invP[12]), mirror uint8 [C, H, W],
        grid_params [C, 4], scale [L]
target  dict: kp_xy float32 [n, 2], kp_octave [n], kp_cam [n], desc uint8 [n, bytes], m_t [4, 4];
        optional mask [n, bytes]; rays [n, 3] for rule 0
queries dict: pos [nq, 3], dist [nq, 2] (mfMinDistance, mfMaxDistance), desc [nq, bytes];
        optional mask; rays [nq, 3] and m_t [4, 4] (curKF) for rule 0
There is no CPU fallback for the device part: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib
from .window import GRID_COLS, GRID_ROWS, grid_build

USE_DISTANCE = 1          # MCS_FUSE_USE_DISTANCE
ADD, REPLACE = 0, 1       # MCS_FUSE_ADD / MCS_FUSE_REPLACE
NO_DIST = 2 ** 31 - 1     # best_dist where no candidate was scanned (INT_MAX)


class FuseTargets(ctypes.Structure):
    """Mirror of mcs_fuse_targets."""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_targets", "n_kp_total", "n_cams", "bytes", "n_levels",
                                              "mirror_w", "mirror_h")] + \
               [(k, ctypes.c_void_p) for k in ("off", "kp_xy", "kp_octave", "kp_cam", "desc", "mask", "rays",
                                               "m_t", "m_c", "cam", "mirror", "grid_params", "scale",
                                               "cell_ptr", "cell_kp")]


class FuseQueries(ctypes.Structure):
    """Mirror of mcs_fuse_queries."""
    _fields_ = [("nq", ctypes.c_int32)] + \
               [(k, ctypes.c_void_p) for k in ("pos", "dist", "desc", "mask", "rays", "m_t")]


_T_DTYPES = {"off": np.int32, "kp_xy": np.float32, "kp_octave": np.int32, "kp_cam": np.int32,
             "desc": np.uint8, "mask": np.uint8, "rays": np.float64, "m_t": np.float64, "m_c": np.float64,
             "cam": np.float64, "mirror": np.uint8, "grid_params": np.float64, "scale": np.float64,
             "cell_ptr": np.int32, "cell_kp": np.int32}
_Q_DTYPES = {"pos": np.float64, "dist": np.float64, "desc": np.uint8, "mask": np.uint8,
             "rays": np.float64, "m_t": np.float64}


def cayley2hom(p):
    """cayley2hom (reference include/misc.h:134-162, :213-226): 6-vector -> 4x4, R = (1 / scale) * R."""
    c1, c2, c3 = (float(x) for x in p[:3])
    c1s, c2s, c3s = c1 * c1, c2 * c2, c3 * c3
    inv = 1 / (1.0 + c1s + c2s + c3s)
    R = [1 + c1s - c2s - c3s, 2 * (c1 * c2 - c3), 2 * (c1 * c3 + c2),
         2 * (c1 * c2 + c3), 1 - c1s + c2s - c3s, 2 * (c2 * c3 - c1),
         2 * (c1 * c3 - c2), 2 * (c2 * c3 + c1), 1 - c1s - c2s + c3s]
    T = np.eye(4)
    T[:3, :3] = np.array([r * inv for r in R]).reshape(3, 3)
    T[:3, 3] = p[3:6]
    return T


def pack_targets(rig, targets, nbytes, with_grid=True):
    """The packed arrays of mcs_fuse_targets for a list of target dicts."""
    n = [len(t["kp_xy"]) for t in targets]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    tot, T = int(off[-1]), len(targets)
    masked = [t.get("mask") is not None for t in targets]
    if masked and any(masked) != all(masked):
        raise ValueError("masks for every target or for none")
    with_rays = bool(targets) and all(t.get("rays") is not None for t in targets)
    mirror = np.ascontiguousarray(rig["mirror"], np.uint8)
    C = len(rig["m_c"])
    ncell = C * GRID_COLS * GRID_ROWS
    p = {"n_targets": T, "n_kp_total": tot, "n_cams": C, "bytes": int(nbytes), "n_levels": len(rig["scale"]),
         "mirror_w": mirror.shape[2], "mirror_h": mirror.shape[1], "off": off,
         "kp_xy": np.zeros((tot, 2), np.float32), "kp_octave": np.zeros(tot, np.int32),
         "kp_cam": np.zeros(tot, np.int32), "desc": np.zeros((tot, nbytes), np.uint8),
         "mask": np.zeros((tot, nbytes), np.uint8) if T and masked[0] else None,
         "rays": np.zeros((tot, 3)) if with_rays else None,
         "m_t": np.zeros((T, 16)), "m_c": np.asarray(rig["m_c"], np.float64).reshape(C, 16),
         "cam": np.asarray(rig["cam"], np.float64).reshape(C, 17), "mirror": mirror,
         "grid_params": np.asarray(rig["grid_params"], np.float64).reshape(C, 4),
         "scale": np.asarray(rig["scale"], np.float64),
         "cell_ptr": np.zeros((T, ncell + 1), np.int32) if with_grid else None,
         "cell_kp": np.zeros(max(tot, 1), np.int32) if with_grid else None}
    for k, t in enumerate(targets):
        o = int(off[k])
        p["kp_xy"][o:o + n[k]] = np.asarray(t["kp_xy"], np.float32).reshape(n[k], 2)
        p["kp_octave"][o:o + n[k]] = t["kp_octave"]
        p["kp_cam"][o:o + n[k]] = t["kp_cam"]
        p["desc"][o:o + n[k]] = np.asarray(t["desc"], np.uint8).reshape(n[k], nbytes)
        if p["mask"] is not None:
            p["mask"][o:o + n[k]] = np.asarray(t["mask"], np.uint8).reshape(n[k], nbytes)
        if with_rays:
            p["rays"][o:o + n[k]] = t["rays"]
        p["m_t"][k] = np.asarray(t["m_t"], np.float64).reshape(16)
        if with_grid:
            ptr, cells = grid_build(p["kp_xy"][o:o + n[k]], p["kp_cam"][o:o + n[k]], p["grid_params"])
            p["cell_ptr"][k] = ptr
            p["cell_kp"][o:o + len(cells)] = cells
    return p


def pack_queries(q, nbytes):
    nq = len(q["pos"])
    p = {"nq": nq, "pos": np.asarray(q["pos"], np.float64).reshape(nq, 3),
         "dist": np.asarray(q["dist"], np.float64).reshape(nq, 2),
         "desc": np.asarray(q["desc"], np.uint8).reshape(nq, nbytes),
         "mask": np.asarray(q["mask"], np.uint8).reshape(nq, nbytes) if q.get("mask") is not None else None,
         "rays": np.asarray(q["rays"], np.float64).reshape(nq, 3) if q.get("rays") is not None else None,
         "m_t": np.asarray(q["m_t"], np.float64).reshape(16) if q.get("m_t") is not None else None}
    return p


_T_INTS = ("n_targets", "n_kp_total", "n_cams", "bytes", "n_levels", "mirror_w", "mirror_h")


def _host(struct, ints, dtypes, p):
    s, keep = struct(*[p[k] for k in ints]), []
    for k, dt in dtypes.items():
        a = p.get(k)
        if a is not None:
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            setattr(s, k, a.ctypes.data)
    return s, keep


def _device(struct, ints, dtypes, p, device):
    import torch
    s, keep = struct(*[p[k] for k in ints]), {}
    for k, dt in dtypes.items():
        a = p.get(k)
        if a is None:
            continue
        t = torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to("cuda:%d" % device)
        keep[k] = t
        setattr(s, k, t.data_ptr())
    return s, keep


def host_sets(pt, pq):
    """(FuseTargets, FuseQueries over the packed numpy arrays, the arrays to keep alive)."""
    ts, k1 = _host(FuseTargets, _T_INTS, _T_DTYPES, pt)
    qs, k2 = _host(FuseQueries, ("nq",), _Q_DTYPES, pq)
    return ts, qs, (k1, k2)


def device_sets(pt, pq, device=0):
    """(FuseTargets, FuseQueries of device pointers, the torch tensors that own them)."""
    ts, k1 = _device(FuseTargets, _T_INTS, _T_DTYPES, pt, device)
    qs, k2 = _device(FuseQueries, ("nq",), _Q_DTYPES, pq, device)
    return ts, qs, (k1, k2)


class Workspace(_Workspace):
    """mcs_fuse_workspace: device scratch for batches of <= max_targets targets."""

    def __init__(self, max_targets, device=0):
        super().__init__("mcs_fuse_workspace_create", "mcs_fuse_workspace_destroy", device, max_targets)


def fuse_device(ws, rule, tset, qset, th, th_low, flags=0, q_skip=None, device=0, out=None):
    """Device entry on FuseTargets / FuseQueries of device pointers -> (best_kp int32,
    best_dist int32 [T, nq, C], epi_ok uint8 [T, nq, C] or None) torch tensors, stream-ordered
    on torch's current stream.  q_skip: torch uint8 [T, nq] on the device or None."""
    import torch
    dev = "cuda:%d" % (ws.device if ws is not None else device)
    shape = (tset.n_targets, qset.nq, tset.n_cams)
    if out is None:
        out = (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev),
               torch.empty(shape, dtype=torch.uint8, device=dev) if rule == 0 else None)
    bk, bd, ep = out
    _check(lib().mcs_fuse_device(ws._h if ws is not None else None, int(rule), int(flags), ctypes.byref(tset),
                                 ctypes.byref(qset), float(th), int(th_low),
                                 q_skip.data_ptr() if q_skip is not None else None, bk.data_ptr(),
                                 bd.data_ptr(), ep.data_ptr() if ep is not None else None,
                                 torch.cuda.current_stream(dev).cuda_stream))
    return bk, bd, ep


def fuse(rule, rig, targets, queries, th, th_low, flags=0, q_skip=None, device=0, nbytes=None):
    """Host entry (mcs_fuse): list of target dicts, query dict -> (best_kp, best_dist int32
    [T, nq, C], epi_ok uint8 [T, nq, C] (rule 0) or None)."""
    nbytes = nbytes or int(np.asarray(queries["desc"]).shape[1])
    pt, pq = pack_targets(rig, targets, nbytes, with_grid=False), pack_queries(queries, nbytes)
    ts, qs, keep = host_sets(pt, pq)
    shape = (ts.n_targets, qs.nq, ts.n_cams)
    bk, bd = np.full(shape, -1, np.int32), np.full(shape, NO_DIST, np.int32)
    ep = np.zeros(shape, np.uint8) if rule == 0 else None
    sk = np.ascontiguousarray(q_skip, np.uint8).reshape(shape[:2]) if q_skip is not None else None
    _check(lib().mcs_fuse(int(device), int(rule), int(flags), ctypes.byref(ts), ctypes.byref(qs), float(th),
                          int(th_low), sk.ctypes.data if sk is not None else None, bk.ctypes.data,
                          bd.ctypes.data, ep.ctypes.data if ep is not None else None))
    return bk, bd, ep


def fuse_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp):
    """mcs_fuse_select for one target.  mp_bad, mp_in_kf (uint8 [n_mp]) and kp_mp (int32 [n_kp])
    are updated in place -> (actions int32 [n, 4] (kind, query, keypoint, other_id), n_fused,
    requery ids)."""
    q_mp = np.ascontiguousarray(q_mp, np.int32)
    best_kp = np.ascontiguousarray(best_kp, np.int32)
    nq = len(q_mp)
    n_cams = best_kp.size // nq if nq else 1
    ep = np.ascontiguousarray(epi_ok, np.uint8) if epi_ok is not None else None
    for a, dt in ((mp_bad, np.uint8), (mp_in_kf, np.uint8), (kp_mp, np.int32)):
        if a.dtype != dt or not a.flags.c_contiguous:
            raise ValueError("state arrays must be contiguous uint8 / uint8 / int32 (updated in place)")
    cap = max(1, nq * n_cams)
    actions = np.zeros((cap, 4), np.int32)
    req = np.zeros(max(1, nq), np.int32)
    na, nf, nr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(lib().mcs_fuse_select(int(rule), nq, int(n_cams), q_mp.ctypes.data, best_kp.ctypes.data,
                                 ep.ctypes.data if ep is not None else None, len(mp_bad), mp_bad.ctypes.data,
                                 mp_in_kf.ctypes.data, len(kp_mp), kp_mp.ctypes.data, actions.ctypes.data, cap,
                                 ctypes.byref(na), ctypes.byref(nf), req.ctypes.data, ctypes.byref(nr)))
    return actions[:na.value].copy(), nf.value, req[:nr.value].copy()


__all__ = ["FuseTargets", "FuseQueries", "Workspace", "pack_targets", "pack_queries", "host_sets",
           "device_sets", "fuse", "fuse_device", "fuse_select", "cayley2hom", "USE_DISTANCE", "ADD",
           "REPLACE", "NO_DIST", "McsError"]
