"""cOptimizer::OptimizeSim3 on the GPU (include/mcs_matcher.h): the Sim3 refinement of one keyframe
against a batch of loop candidates, both LM rounds and the culls in one launch (reference
src/cOptimizerLoopStuff.cpp:63-270, called at src/cLoopClosing.cpp:372).

  optimize_sim3(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first2s, inv_sigma2_1, sigma2_2,
                s12, R12, t12, options=None, flags=0)
        host entry on NumPy -> dict: matches12 after the call and the arrays of mcs_sim3_opt_out
  optimize_sim3_device(ws, k1, p1, k2, p2, matches12, ok1, ok2, first2, inv_sigma2_1, sigma2_2,
                       s12, R12, t12, options)
        the same on structs of device pointers and torch tensors, stream-ordered; matches12 in-out
  merge_matches_device(bow12, inlier, new12)
        vpMapPointMatches of ComputeSim3 (src/cLoopClosing.cpp:354-369) on torch tensors

rig, keyframes and points are the dicts of mcs_amd.sim3_match; of the keyframes kp_xy, kp_octave,
kp_cam and m_t are read, of the points pos.  matches12 int32 [T, n1] holds the KF2 keypoint index
whose slot holds the matched point, -1 = none; first2s the first index of that point in KF2.
flags: OWN_CAMERA projects every edge with its own observation's camera instead of the crossed
lookup of the text.  There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib
from .fuse import pack_targets
from .sim3_match import device_sets, host_sets, pack_points

OWN_CAMERA = 1                  # MCS_SIM3OPT_OWN_CAMERA
MAX_ITS = 16                    # iterations per round the trial log holds

_O_FIELDS = (("n_in", np.int32, ()), ("n_corr", np.int32, ()), ("n_bad", np.int32, ()), ("n_undefined", np.int32, ()),
             ("s12", np.float64, ()), ("q12", np.float64, (4,)), ("R12", np.float64, (9,)), ("t12", np.float64, (3,)),
             ("iters", np.int32, (2,)), ("chi2", np.float64, (2,)), ("lambda", np.float64, (2,)),
             ("trials", np.int32, (2, MAX_ITS)), ("edge_chi2", np.float64, "n1"))


class Sim3OptOptions(ctypes.Structure):
    """Mirror of mcs_sim3_opt_options."""
    _fields_ = [("std_sim", ctypes.c_double), ("its_round1", ctypes.c_int32), ("its_clean", ctypes.c_int32),
                ("its_culled", ctypes.c_int32), ("terminate_max_iter", ctypes.c_int32),
                ("gain_threshold", ctypes.c_double), ("tau", ctypes.c_double), ("max_trials", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class Sim3OptOut(ctypes.Structure):
    """Mirror of mcs_sim3_opt_out."""
    _fields_ = [(k, ctypes.c_void_p) for k, _, _ in _O_FIELDS]


def default_options(flags=0, **kw):
    """mcs_sim3_opt_default_options, then the keyword overrides."""
    o = Sim3OptOptions()
    lib().mcs_sim3_opt_default_options(ctypes.byref(o))
    o.flags = int(flags)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise ValueError("no such option: %s" % k)
        setattr(o, k, v)
    return o


def out_shapes(T, n1):
    """name -> (dtype, shape) of the buffers of mcs_sim3_opt_out."""
    return {k: (dt, (T, n1, 2) if shp == "n1" else (T,) + shp) for k, dt, shp in _O_FIELDS}


class Workspace(_Workspace):
    """mcs_sim3_opt_workspace: device scratch for <= max_targets candidates and a KF1 of <= max_kp slots."""

    def __init__(self, max_targets, max_kp, device=0):
        super().__init__("mcs_sim3_opt_workspace_create", "mcs_sim3_opt_workspace_destroy", device, max_targets,
                         max_kp)


def pack_call(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first2s, nbytes=None):
    """Packed keyframe sets, point sets and the per-slot arrays of one call ->
    (pk1, pp1, pk2, pp2, matches12 [T, n1], ok1, ok2, first2)."""
    nbytes = nbytes or int(np.asarray(kf1["desc"]).shape[1])
    T = len(kf2s)
    pk1, pk2 = pack_targets(rig, [kf1], nbytes, False), pack_targets(rig, kf2s, nbytes, False)
    pp1, pp2 = pack_points([pts1], nbytes), pack_points(pts2s, nbytes)
    n1 = pk1["n_kp_total"]
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])  # noqa: E731
                                              if len(xs) else np.zeros(0, dt))
    return (pk1, pp1, pk2, pp2, np.ascontiguousarray(matches12, np.int32).reshape(T, n1).copy(),
            np.ascontiguousarray(ok1, np.uint8).reshape(n1), cat(ok2s, np.uint8), cat(first2s, np.int32))


def _stream(device):
    import torch
    return torch.cuda.current_stream("cuda:%d" % device).cuda_stream


def new_out(T, n1, device=0, edge_chi2=True, trials=True):
    """A Sim3OptOut of fresh device tensors -> (Sim3OptOut, tensors by name)."""
    import torch
    s, ts = Sim3OptOut(), {}
    for k, (dt, shp) in out_shapes(T, n1).items():
        if (k == "edge_chi2" and not edge_chi2) or (k == "trials" and not trials):
            continue
        ts[k] = torch.zeros(shp, dtype=getattr(torch, np.dtype(dt).name), device="cuda:%d" % device)
        setattr(s, k, ts[k].data_ptr())
    return s, ts


def optimize_sim3_device(ws, k1, p1, k2, p2, matches12, ok1, ok2, first2, inv_sigma2_1, sigma2_2, s12, R12, t12,
                         options=None, out=None, device=0):
    """mcs_optimize_sim3_device on torch tensors, stream-ordered on torch's current stream.
    matches12 int32 [T, n1] is rewritten in place.  out: (Sim3OptOut, tensors) of new_out, made when
    not given -> the tensors by name."""
    device = ws.device if ws is not None else device
    o = options if options is not None else default_options()
    if out is None:
        out = new_out(k2.n_targets, k1.n_kp_total, device)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_optimize_sim3_device(ws._h if ws is not None else None, ctypes.byref(k1), ctypes.byref(p1),
                                          ctypes.byref(k2), ctypes.byref(p2), ptr(matches12), ptr(ok1), ptr(ok2),
                                          ptr(first2), ptr(inv_sigma2_1), ptr(sigma2_2), ptr(s12), ptr(R12),
                                          ptr(t12), ctypes.byref(o), ctypes.byref(out[0]), _stream(device)))
    return out[1]


def merge_matches_device(bow12, inlier, new12, out=None, device=0):
    """mcs_sim3_merge_matches_device: bow12 / new12 int32 [T, n1], inlier uint8 [T, n1] on the device
    -> matches12 int32 [T, n1]: the BoW match where inlier, else new12 when >= 0, else -1."""
    import torch
    T, n1 = bow12.shape
    if out is None:
        out = torch.empty((T, n1), dtype=torch.int32, device=bow12.device)
    _check(lib().mcs_sim3_merge_matches_device(bow12.data_ptr(), inlier.data_ptr(), new12.data_ptr(), int(T), int(n1),
                                               out.data_ptr(), _stream(device)))
    return out


def optimize_sim3(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first2s, inv_sigma2_1, sigma2_2, s12, R12, t12,
                  options=None, flags=0, device=0):
    """Host entry (mcs_optimize_sim3) -> dict: matches12 [T, n1] after the call and the arrays of
    mcs_sim3_opt_out by name.  options: Sim3OptOptions, or a dict of overrides of the defaults."""
    pk1, pp1, pk2, pp2, m12, o1, o2, f2 = pack_call(rig, kf1, pts1, kf2s, pts2s, matches12, ok1, ok2s, first2s)
    k1, p1, keep1 = host_sets(pk1, pp1)
    k2, p2, keep2 = host_sets(pk2, pp2)
    T, n1 = len(kf2s), pk1["n_kp_total"]
    o = options if isinstance(options, Sim3OptOptions) else default_options(flags, **(options or {}))
    out, arrs = Sim3OptOut(), {}
    for k, (dt, shp) in out_shapes(T, n1).items():
        arrs[k] = np.zeros(shp, dt)
        setattr(out, k, arrs[k].ctypes.data)
    f64 = lambda a, shp: np.ascontiguousarray(a, np.float64).reshape(shp)  # noqa: E731
    is1, s2 = f64(inv_sigma2_1, -1), f64(sigma2_2, -1)
    s, R, t = f64(s12, T), f64(R12, (T, 9)), f64(t12, (T, 3))
    _check(lib().mcs_optimize_sim3(int(device), ctypes.byref(k1), ctypes.byref(p1), ctypes.byref(k2),
                                   ctypes.byref(p2), m12.ctypes.data, o1.ctypes.data, o2.ctypes.data,
                                   f2.ctypes.data, is1.ctypes.data, s2.ctypes.data, s.ctypes.data, R.ctypes.data,
                                   t.ctypes.data, ctypes.byref(o), ctypes.byref(out)))
    return dict(arrs, matches12=m12)


__all__ = ["Sim3OptOptions", "Sim3OptOut", "Workspace", "default_options", "out_shapes", "pack_call", "new_out",
           "device_sets", "host_sets", "optimize_sim3", "optimize_sim3_device", "merge_matches_device", "OWN_CAMERA",
           "MAX_ITS", "McsError"]
