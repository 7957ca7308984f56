"""Bundle adjustment binding (include/mcs_ba.h) + synthetic MultiCol BA problems.

Host mirror of cOptimizer::LocalBundleAdjustment (reference src/cOptimizer.cpp:489-908):
`local_ba(problem)` runs the GPU solver through mcs_local_ba; `optimize(problem, ...)` is one
initializeOptimization(0) + optimize(n) (the g2o call pair).


The synthetic problems and maps (make_problem, config_e_problem, ...) are in ba_synth.py and
re-exported here.
"""
import ctypes
import os
import threading
import weakref
from types import SimpleNamespace

import numpy as np

from .ba_synth import (HUBER_GLOBAL, cam_vec, cay2rot, config_e_problem, covisibles,  # noqa: F401
                       global_map_from_problem, make_global_problem, make_map, make_pose_problem,
                       make_problem, project, ring_rig, rot2cay, shard_points, shard_problem)

_D = ctypes.POINTER(ctypes.c_double)


class BAProblem(ctypes.Structure):
    _fields_ = [("n_poses", ctypes.c_int32), ("n_points", ctypes.c_int32),
                ("n_edges", ctypes.c_int32), ("n_cams", ctypes.c_int32),
                ("poses", ctypes.c_void_p), ("pose_fixed", ctypes.c_void_p),
                ("points", ctypes.c_void_p), ("mc", ctypes.c_void_p), ("cam", ctypes.c_void_p),
                ("edge_pose", ctypes.c_void_p), ("edge_point", ctypes.c_void_p),
                ("edge_cam", ctypes.c_void_p), ("edge_meas", ctypes.c_void_p),
                ("edge_info", ctypes.c_void_p), ("huber_delta", ctypes.c_double)]


class BAOptions(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int32), ("gain_threshold", ctypes.c_double),
                ("terminate_max_iter", ctypes.c_int32), ("max_trials", ctypes.c_int32),
                ("tau", ctypes.c_double)]

    def __init__(self, max_iterations=10, gain_threshold=1e-6, terminate_max_iter=15,
                 max_trials=10, tau=1e-5):
        super().__init__(max_iterations, gain_threshold, terminate_max_iter, max_trials, tau)


class BAReport(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("stop_flag", ctypes.c_int32),
                ("chi2_initial", ctypes.c_double), ("chi2_final", ctypes.c_double),
                ("lambda_final", ctypes.c_double), ("n_active_edges", ctypes.c_int32),
                ("n_active_poses", ctypes.c_int32), ("n_active_points", ctypes.c_int32),
                ("trace_chi2", ctypes.c_void_p), ("trace_cap", ctypes.c_int32)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_PROBLEM_FIELDS = (("poses", np.float64), ("pose_fixed", np.uint8), ("points", np.float64),
                   ("mc", np.float64), ("cam", np.float64), ("edge_pose", np.int32),
                   ("edge_point", np.int32), ("edge_cam", np.int32), ("edge_meas", np.float64),
                   ("edge_info", np.float64))


_STRUCT_CACHE = []   # (weakrefs to the arrays, huber_delta, BAProblem), most recent last
_STRUCT_CACHE_LOCK = threading.Lock()
_STRUCT_CACHE_SIZE = 2


def as_struct(pr):
    """numpy problem dict -> BAProblem (keeps references alive in the dict).  A dict whose
    arrays are the same objects as at an earlier call (values may have changed in place) gets
    that call's struct back: the addresses are the same, and reading ten array addresses cost
    ~30 us of a ~2.3 ms LocalBA call.  The cache holds weak references only, so a problem the
    caller drops is freed (a dead reference never matches: a new array at a reused address is
    a cache miss), and at most two entries."""
    arrs = tuple(pr[k] for k, _ in _PROBLEM_FIELDS)
    hd = float(pr["huber_delta"])
    with _STRUCT_CACHE_LOCK:
        for ent in _STRUCT_CACHE:
            if ent[1] == hd and all(r() is y for r, y in zip(ent[0], arrs)):
                return ent[2]
    addr = []
    for k, dt in _PROBLEM_FIELDS:
        a = pr[k]
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
            a = pr[k] = np.ascontiguousarray(a, dtype=dt)
        addr.append(a.__array_interface__["data"][0])
    s = BAProblem(len(pr["poses"]), len(pr["points"]), len(pr["edge_pose"]), len(pr["mc"]),
                  *addr, hd)
    refs = tuple(weakref.ref(pr[k]) for k, _ in _PROBLEM_FIELDS)
    with _STRUCT_CACHE_LOCK:
        _STRUCT_CACHE[:] = [e for e in _STRUCT_CACHE if all(r() is not None for r in e[0])]
        _STRUCT_CACHE.append((refs, hd, s))
        del _STRUCT_CACHE[:-_STRUCT_CACHE_SIZE]
    return s


# ---------------------------------------------------------------------------
# LocalBundleAdjustment graph assembly (mcs_local_ba_select, src/cOptimizer.cpp:503-769)
# ---------------------------------------------------------------------------
class LbaMap(ctypes.Structure):
    _fields_ = [("n_kf", ctypes.c_int32), ("kf_id", ctypes.c_void_p), ("kf_bad", ctypes.c_void_p),
                ("kf_mp_off", ctypes.c_void_p), ("kf_mp", ctypes.c_void_p),
                ("n_points", ctypes.c_int32), ("pt_bad", ctypes.c_void_p),
                ("pt_obs_off", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p)]


class LbaGraph(ctypes.Structure):
    _fields_ = [("local_kf", ctypes.c_void_p), ("n_local", ctypes.c_int32),
                ("fixed_kf", ctypes.c_void_p), ("n_fixed", ctypes.c_int32),
                ("pose_fixed", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("n_points", ctypes.c_int32), ("point_extra_obs", ctypes.c_void_p),
                ("edge_obs", ctypes.c_void_p), ("edge_pose", ctypes.c_void_p),
                ("edge_point", ctypes.c_void_p), ("n_edges", ctypes.c_int32),
                ("edge_cap", ctypes.c_int32)]


MCS_LBA_EMPTY = 1


def lba_map_struct(m):
    """numpy map dict (make_map) -> LbaMap (arrays kept alive in the dict)."""
    for k, dt in (("kf_id", np.int64), ("kf_bad", np.uint8), ("kf_mp_off", np.int32),
                  ("kf_mp", np.int32), ("pt_bad", np.uint8), ("pt_obs_off", np.int32),
                  ("obs_kf", np.int32)):
        m[k] = np.ascontiguousarray(m[k], dt)
    return LbaMap(len(m["kf_id"]), _p(m["kf_id"]), _p(m["kf_bad"]), _p(m["kf_mp_off"]),
                  _p(m["kf_mp"]), len(m["pt_bad"]), _p(m["pt_bad"]), _p(m["pt_obs_off"]),
                  _p(m["obs_kf"]))


def lba_graph_buffers(m):
    nk, npt, nobs = len(m["kf_id"]), len(m["pt_bad"]), len(m["obs_kf"])
    b = dict(local_kf=np.zeros(nk, np.int32), fixed_kf=np.zeros(nk, np.int32),
             pose_fixed=np.zeros(nk, np.uint8), points=np.zeros(npt, np.int32),
             point_extra_obs=np.zeros(npt, np.int32), edge_obs=np.zeros(max(1, nobs), np.int32),
             edge_pose=np.zeros(max(1, nobs), np.int32), edge_point=np.zeros(max(1, nobs), np.int32))
    g = LbaGraph(_p(b["local_kf"]), 0, _p(b["fixed_kf"]), 0, _p(b["pose_fixed"]), _p(b["points"]),
                 0, _p(b["point_extra_obs"]), _p(b["edge_obs"]), _p(b["edge_pose"]),
                 _p(b["edge_point"]), 0, nobs)
    return g, b


def lba_graph_result(rc, g, b):
    nl, nf, npt, ne = g.n_local, g.n_fixed, g.n_points, g.n_edges
    return dict(status=rc, local_kf=b["local_kf"][:nl].copy(), fixed_kf=b["fixed_kf"][:nf].copy(),
                pose_fixed=b["pose_fixed"][:nl + nf].copy(), points=b["points"][:npt].copy(),
                point_extra_obs=b["point_extra_obs"][:npt].copy(),
                edge_obs=b["edge_obs"][:ne].copy(), edge_pose=b["edge_pose"][:ne].copy(),
                edge_point=b["edge_point"][:ne].copy())


def local_ba_select(m, cur, covis):
    """mcs_local_ba_select: local / fixed keyframes, local points and edges of
    LocalBundleAdjustment for keyframe `cur` with covisibles `covis` (ordered)."""
    from . import lib
    st = lba_map_struct(m)
    cv = np.ascontiguousarray(covis, np.int32)
    g, b = lba_graph_buffers(m)
    rc = lib().mcs_local_ba_select(ctypes.byref(st), int(cur), _p(cv), len(cv), ctypes.byref(g))
    if rc < 0:
        from . import McsError, lib as _l
        raise McsError(rc, _l().mcs_last_error().decode())
    return lba_graph_result(rc, g, b)


def problem_from_graph(m, g, huber_delta=1.345 * 2):
    """mcs_ba_problem of one LocalBundleAdjustment call (vertices :585-711, edges :712-766):
    pose slots = local then fixed keyframes, points = local points, one edge per selected
    observation (measurement kp.pt, information invSigma2(octave))."""
    slots = np.concatenate([g["local_kf"], g["fixed_kf"]]).astype(np.int64)
    o = g["edge_obs"]
    return dict(poses=m["kf_pose"][slots].copy(), pose_fixed=g["pose_fixed"].copy(),
                points=m["pt_pos"][g["points"]].copy(), mc=m["mc"], cam=m["cam"],
                edge_pose=g["edge_pose"].astype(np.int32), edge_point=g["edge_point"].astype(np.int32),
                edge_cam=m["obs_cam"][o].astype(np.int32), edge_meas=m["obs_meas"][o].copy(),
                edge_info=m["obs_info"][o].copy(), huber_delta=huber_delta)


class GbaMap(ctypes.Structure):
    """Mirror of mcs_gba_map (include/mcs_ba.h)."""
    _fields_ = [("n_kf", ctypes.c_int32), ("kf_id", ctypes.c_void_p), ("kf_bad", ctypes.c_void_p),
                ("n_points", ctypes.c_int32), ("pt_id", ctypes.c_void_p), ("pt_bad", ctypes.c_void_p),
                ("pt_obs_off", ctypes.c_void_p), ("obs_kf", ctypes.c_void_p), ("n_cams", ctypes.c_int32)]


class GbaGraph(ctypes.Structure):
    """Mirror of mcs_gba_graph."""
    _fields_ = [("pose_kf", ctypes.c_void_p), ("pose_fixed", ctypes.c_void_p), ("n_poses", ctypes.c_int32),
                ("points", ctypes.c_void_p), ("point_vertex_id", ctypes.c_void_p), ("n_points", ctypes.c_int32),
                ("mc_vertex_id0", ctypes.c_int64), ("io_vertex_id0", ctypes.c_int64),
                ("kf_slot", ctypes.c_void_p), ("pt_slot", ctypes.c_void_p),
                ("edge_obs", ctypes.c_void_p), ("edge_pose", ctypes.c_void_p), ("edge_point", ctypes.c_void_p),
                ("n_edges", ctypes.c_int32), ("edge_cap", ctypes.c_int32), ("collision_id", ctypes.c_int64)]


class PoFrame(ctypes.Structure):
    """Mirror of mcs_po_frame."""
    _fields_ = [("n_keys", ctypes.c_int32), ("key_mp", ctypes.c_void_p), ("n_mp", ctypes.c_int32),
                ("pt_id", ctypes.c_void_p), ("n_cams", ctypes.c_int32)]


class PoGraph(ctypes.Structure):
    """Mirror of mcs_po_graph."""
    _fields_ = [("points", ctypes.c_void_p), ("point_vertex_id", ctypes.c_void_p), ("n_points", ctypes.c_int32),
                ("edge_obs", ctypes.c_void_p), ("edge_point", ctypes.c_void_p), ("n_edges", ctypes.c_int32),
                ("edge_cap", ctypes.c_int32)]


def global_ba_select(m, raise_on_error=True):
    """mcs_global_ba_select: the vertices and edges cOptimizer::BundleAdjustment builds from
    (vpKFs, vpMP) = the map dict's keyframes and points in list order (src/cOptimizer.cpp:101-234),
    and the write-back slots of :240-259.  m needs kf_id, kf_bad, pt_id, pt_bad, pt_obs_off,
    obs_kf and mc (n_cams)."""
    from . import lib, McsError
    for k, dt in (("kf_id", np.int64), ("kf_bad", np.uint8), ("pt_id", np.int64), ("pt_bad", np.uint8),
                  ("pt_obs_off", np.int32), ("obs_kf", np.int32)):
        m[k] = np.ascontiguousarray(m[k], dt)
    nk, npt, nobs = len(m["kf_id"]), len(m["pt_bad"]), len(m["obs_kf"])
    st = GbaMap(nk, _p(m["kf_id"]), _p(m["kf_bad"]), npt, _p(m["pt_id"]), _p(m["pt_bad"]),
                _p(m["pt_obs_off"]), _p(m["obs_kf"]), len(m["mc"]))
    b = dict(pose_kf=np.zeros(max(1, nk), np.int32), pose_fixed=np.zeros(max(1, nk), np.uint8),
             points=np.zeros(max(1, npt), np.int32), point_vertex_id=np.zeros(max(1, npt), np.int64),
             kf_slot=np.zeros(max(1, nk), np.int32), pt_slot=np.zeros(max(1, npt), np.int32),
             edge_obs=np.zeros(max(1, nobs), np.int32), edge_pose=np.zeros(max(1, nobs), np.int32),
             edge_point=np.zeros(max(1, nobs), np.int32))
    g = GbaGraph(_p(b["pose_kf"]), _p(b["pose_fixed"]), 0, _p(b["points"]), _p(b["point_vertex_id"]), 0,
                 -1, -1, _p(b["kf_slot"]), _p(b["pt_slot"]), _p(b["edge_obs"]), _p(b["edge_pose"]),
                 _p(b["edge_point"]), 0, nobs, -1)
    rc = lib().mcs_global_ba_select(ctypes.byref(st), ctypes.byref(g))
    if rc < 0 and raise_on_error:
        raise McsError(rc, lib().mcs_last_error().decode())
    npo, npp, ne = g.n_poses, g.n_points, g.n_edges
    return dict(status=rc, collision_id=g.collision_id, pose_kf=b["pose_kf"][:npo].copy(),
                pose_fixed=b["pose_fixed"][:npo].copy(), points=b["points"][:npp].copy(),
                point_vertex_id=b["point_vertex_id"][:npp].copy(), mc_vertex_id0=g.mc_vertex_id0,
                io_vertex_id0=g.io_vertex_id0, kf_slot=b["kf_slot"][:nk].copy(),
                pt_slot=b["pt_slot"][:npt].copy(), edge_obs=b["edge_obs"][:ne].copy(),
                edge_pose=b["edge_pose"][:ne].copy(), edge_point=b["edge_point"][:ne].copy())


def problem_from_gba_graph(m, g):
    """mcs_ba_problem of one BundleAdjustment call: poses = the keyframe vertices (mnId 0
    fixed), points = the point vertices, one edge per selected observation with measurement
    kp.pt, information I (:209) and Huber sqrt(5.991) (:161)."""
    o = g["edge_obs"]
    return dict(poses=np.ascontiguousarray(m["kf_pose"][g["pose_kf"]]), pose_fixed=g["pose_fixed"].copy(),
                points=np.ascontiguousarray(m["pt_pos"][g["points"]]), mc=m["mc"], cam=m["cam"],
                edge_pose=g["edge_pose"].astype(np.int32), edge_point=g["edge_point"].astype(np.int32),
                edge_cam=np.asarray(m["obs_cam"])[o].astype(np.int32),
                edge_meas=np.ascontiguousarray(np.asarray(m["obs_meas"])[o]), edge_info=np.ones(len(o)),
                huber_delta=HUBER_GLOBAL)


def global_ba_write_back(m, g, poses, points):
    """The reference's recovery loops (:242-259) over the select's slots: new keyframe poses
    and point positions for every list entry with a vertex (others keep their values)."""
    kp = np.array(m["kf_pose"], np.float64, copy=True)
    pp = np.array(m["pt_pos"], np.float64, copy=True)
    ks, ps = g["kf_slot"], g["pt_slot"]
    kp[ks >= 0] = poses[ks[ks >= 0]]
    pp[ps >= 0] = points[ps[ps >= 0]]
    return kp, pp


def pose_optimization_select(key_mp, pt_id, n_cams):
    """mcs_pose_optimization_select: PoseOptimization's point vertices (one per distinct
    mnId, first appearance) and edges (one per non-NULL keypoint), src/cOptimizer.cpp:364-430."""
    from . import lib, McsError
    km = np.ascontiguousarray(key_mp, np.int32)
    pid = np.ascontiguousarray(pt_id, np.int64)
    f = PoFrame(len(km), _p(km), len(pid), _p(pid), int(n_cams))
    b = dict(points=np.zeros(max(1, len(pid)), np.int32), point_vertex_id=np.zeros(max(1, len(pid)), np.int64),
             edge_obs=np.zeros(max(1, len(km)), np.int32), edge_point=np.zeros(max(1, len(km)), np.int32))
    g = PoGraph(_p(b["points"]), _p(b["point_vertex_id"]), 0, _p(b["edge_obs"]), _p(b["edge_point"]), 0, len(km))
    rc = lib().mcs_pose_optimization_select(ctypes.byref(f), ctypes.byref(g))
    if rc < 0:
        raise McsError(rc, lib().mcs_last_error().decode())
    return dict(points=b["points"][:g.n_points].copy(), point_vertex_id=b["point_vertex_id"][:g.n_points].copy(),
                edge_obs=b["edge_obs"][:g.n_edges].copy(), edge_point=b["edge_point"][:g.n_edges].copy())


# ---------------------------------------------------------------------------
# GPU solver binding
# ---------------------------------------------------------------------------
class Solver:
    """mcs_ba_ctx wrapper (device context reused across calls)."""

    def __init__(self, device=0):
        from . import lib, _check
        self._lib, self._check = lib(), _check
        h = ctypes.c_void_p()
        _check(self._lib.mcs_ba_create(int(device), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mcs_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _begin(pr, stop_flag=None, trace=0, reports=1):
        """What every solve starts with: the problem struct, working copies of the poses and
        points, the stop-flag cell (sf; sfp = its reference, None for a null flag) and the
        reports, each with a chi2 trace buffer when trace > 0."""
        sf = None if stop_flag is None else ctypes.c_int32(int(stop_flag))
        tr = [np.zeros(max(trace, 1), np.float64) for _ in range(reports)]
        return SimpleNamespace(
            s=as_struct(pr), poses=pr["poses"].copy(), points=pr["points"].copy(), sf=sf,
            sfp=None if sf is None else ctypes.byref(sf), trace=trace, tr=tr,
            rep=[BAReport(0, 0, 0, 0, 0, 0, 0, 0, _p(t) if trace else None, trace) for t in tr])

    @staticmethod
    def _end(c):
        """-> (the stop flag afterwards, or None; the filled part of every report's trace)"""
        return (None if c.sf is None else c.sf.value,
                [t[:min(c.trace, r.iterations)] for t, r in zip(c.tr, c.rep)])

    def optimize(self, pr, options=None, edge_level=None, stop_flag=None, trace=0):
        return self.optimize_sharded(pr, None, options, edge_level, stop_flag, trace)

    def optimize_sharded(self, pr, exchange, options=None, edge_level=None, stop_flag=None,
                         trace=0):
        """mcs_ba_optimize_sharded on this rank's problem (exchange None: mcs_ba_optimize)."""
        c = self._begin(pr, stop_flag, trace)
        lvl = np.zeros(len(pr["edge_pose"]), np.uint8) if edge_level is None else \
            np.ascontiguousarray(edge_level, np.uint8)
        chi = np.zeros(len(pr["edge_pose"]), np.float64)
        o = options or BAOptions()
        args = (self._h, ctypes.byref(c.s), ctypes.byref(o), _p(c.poses), _p(c.points), _p(lvl),
                _p(chi), c.sfp, ctypes.byref(c.rep[0]))
        if exchange is None:
            self._check(self._lib.mcs_ba_optimize(*args))
        else:
            self._check(self._lib.mcs_ba_optimize_sharded(*args, ctypes.byref(exchange.shard)))
        sf, (tr,) = self._end(c)
        return dict(poses=c.poses, points=c.points, edge_chi2=chi, report=c.rep[0], stop_flag=sf,
                    trace=tr)

    def global_ba(self, pr, pose_only=False, stop_flag=None, exchange=None, trace=0):
        """cOptimizer::BundleAdjustment (src/cOptimizer.cpp:73-261) on this rank's problem."""
        c = self._begin(pr, stop_flag, trace)
        sh = ctypes.byref(exchange.shard) if exchange is not None else None
        self._check(self._lib.mcs_global_ba(self._h, ctypes.byref(c.s), 1 if pose_only else 0,
                                            _p(c.poses), _p(c.points), c.sfp,
                                            ctypes.byref(c.rep[0]), sh))
        sf, (tr,) = self._end(c)
        return dict(poses=c.poses, points=c.points, report=c.rep[0], stop_flag=sf, trace=tr)

    def local_ba_ex(self, pr, extra_obs=None, stop_flag=0, point_write=True):
        """mcs_local_ba_ex: LocalBA rounds with the map-point bookkeeping (bad points, write-back
        mask).  extra_obs: observations of each point from bad keyframes (or None);
        stop_flag None = pbStopFlag NULL (g2o's auxiliary terminate flag)."""
        c = self._begin(pr, stop_flag, reports=2)
        n = len(pr["edge_pose"])
        inl = np.zeros(max(1, n), np.uint8)
        pw = np.zeros(max(1, len(c.points)), np.uint8) if point_write else None
        ex = None if extra_obs is None else np.ascontiguousarray(extra_obs, np.int32)
        wb = ctypes.c_int32()
        self._check(self._lib.mcs_local_ba_ex(
            self._h, ctypes.byref(c.s), None if ex is None else _p(ex), _p(c.poses), _p(c.points),
            _p(inl), None if pw is None else _p(pw), ctypes.byref(wb), c.sfp,
            ctypes.byref(c.rep[0]), ctypes.byref(c.rep[1])))
        out = dict(poses=c.poses, points=c.points, edge_inlier=inl[:n].copy(), write_back=wb.value,
                   stop_flag=self._end(c)[0], report1=c.rep[0], report2=c.rep[1])
        if point_write:
            out["point_write"] = pw[:len(c.points)].copy()
        return out

    def local_ba(self, pr, stop_flag=0):
        """mcs_local_ba: local_ba_ex without the extra observations and the write-back mask."""
        return self.local_ba_ex(pr, None, stop_flag, point_write=False)

    def pose_optimization(self, pr, trace=0):
        """cOptimizer::PoseOptimization (src/cOptimizer.cpp:264-486) via mcs_pose_optimization;
        pr holds one pose and fixed map points (make_pose_problem)."""
        c = self._begin(pr, None, trace, reports=2)
        pose = c.poses[0]
        n = len(pr["edge_pose"])
        out = np.zeros(max(n, 1), np.uint8)
        ngood = ctypes.c_int32()
        bad = ctypes.c_double()
        self._check(self._lib.mcs_pose_optimization(
            self._h, ctypes.byref(c.s), _p(pose), _p(out), ctypes.byref(ngood), ctypes.byref(bad),
            ctypes.byref(c.rep[0]), ctypes.byref(c.rep[1])))
        t1, t2 = self._end(c)[1]
        return dict(pose=pose, outlier=out[:n].copy(), n_good=ngood.value, bad_ratio=bad.value,
                    report1=c.rep[0], report2=c.rep[1], trace1=t1, trace2=t2)

    def linearize(self, pr):
        s = as_struct(pr)
        n = len(pr["edge_pose"])
        err = np.zeros((n, 2))
        jp = np.zeros((n, 2, 6))
        jl = np.zeros((n, 2, 3))
        self._check(self._lib.mcs_ba_linearize(self._h, ctypes.byref(s), _p(err), _p(jp), _p(jl)))
        return err, jp, jl

    def enable_timing(self, on=True):
        self._check(self._lib.mcs_ba_enable_timing(self._h, 1 if on else 0))

    def read_timing(self, reset=True):
        """-> (dict stage -> accumulated ms, iterations, trials, last reduced-system size n)."""
        ms = np.zeros(len(BA_STAGES))
        it, tr, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.mcs_ba_read_timing(self._h, _p(ms), ctypes.byref(it), ctypes.byref(tr),
                                                 ctypes.byref(n), 1 if reset else 0))
        return dict(zip(BA_STAGES, ms.tolist())), it.value, tr.value, n.value

    def read_host_timing(self, reset=True):
        """-> (dict host phase -> accumulated ms, optimize calls) (mcs_ba_read_host_timing)."""
        ms = np.zeros(len(BA_HOST_PHASES))
        n = ctypes.c_int32()
        self._check(self._lib.mcs_ba_read_host_timing(self._h, _p(ms), ctypes.byref(n),
                                                      1 if reset else 0))
        return dict(zip(BA_HOST_PHASES, ms.tolist())), n.value

    def read_solve_shape(self):
        """-> dict(n, T, band, pipelined) of the last call's reduced camera system
        (mcs_ba_read_solve_shape): band = the tile diagonals the factorisation ran on."""
        v = [ctypes.c_int32() for _ in range(4)]
        self._check(self._lib.mcs_ba_read_solve_shape(self._h, *[ctypes.byref(x) for x in v]))
        return dict(n=v[0].value, T=v[1].value, band=v[2].value, pipelined=bool(v[3].value))

    def set_ldlt_mode(self, mode):
        """Test hook (mcs_ba_set_ldlt_mode): 0 banded pipeline (default), 1 dense pipeline,
        2 one panel launch per step.  A later call the mode does not take raises McsError."""
        self._check(self._lib.mcs_ba_set_ldlt_mode(self._h, int(mode)))


# ---------------------------------------------------------------------------
# Global BA (config E) and point sharding
# ---------------------------------------------------------------------------
# (user, op, offset, count, hipStream_t of the library)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                ctypes.c_int64, ctypes.c_void_p)


class BAShard(ctypes.Structure):
    """Mirror of mcs_ba_shard (include/mcs_ba.h)."""
    _fields_ = [("rank", ctypes.c_int32), ("world", ctypes.c_int32), ("xchg", ctypes.c_void_p),
                ("xchg_cap", ctypes.c_int64), ("allreduce", ALLREDUCE_FN),
                ("user", ctypes.c_void_p), ("stream_ordered", ctypes.c_int32)]


class TorchExchange:
    """mcs_ba_shard backed by torch.distributed: the exchange buffer is a torch tensor on the
    rank's GPU and the callback all-reduces a slice of it (backend "nccl" = RCCL over xGMI).

    Default (stream_ordered = 0): the library drains its stream before each call and the
    callback returns only once the reduction is complete (the all-reduce is followed by a
    device synchronisation), which is correct whatever ProcessGroupNCCL does with streams.

    stream_ordered = 1 (opt-in: argument, or MCS_BA_STREAM_ORDERED=1): the callback issues the
    all-reduce with the library's stream as torch's current stream, so RCCL starts after the
    kernels that produced the slice and the library's next kernels wait for it on the device --
    no host synchronisation per exchange.  This relies on ProcessGroupNCCL making the external
    stream wait for the collective; it has run only on gloo and on the single-GPU ThreadExchange
    mock, never on real RCCL with world > 1, so it stays off until a 2-GPU run has shown ordered
    == unordered (identical poses and iteration counts).  A CPU buffer (gloo) is always reduced
    synchronously."""

    def __init__(self, n_poses, device, group=None, stream_ordered=None):
        import torch
        import torch.distributed as dist
        from . import lib
        self.torch, self.dist, self.group = torch, dist, group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        cap = int(lib().mcs_ba_xchg_doubles(int(n_poses)))
        self.buf = torch.zeros(cap, dtype=torch.float64, device=device)
        self._cb = ALLREDUCE_FN(self._allreduce)
        if stream_ordered is None:
            stream_ordered = os.environ.get("MCS_BA_STREAM_ORDERED", "0") == "1"
        self.ordered = bool(stream_ordered) and self.buf.is_cuda
        self.shard = BAShard(self.rank, self.world, self.buf.data_ptr(), cap, self._cb, None,
                             1 if self.ordered else 0)
        self._streams = {}
        self.calls = 0

    def _stream(self, handle):
        s = self._streams.get(handle)
        if s is None:
            s = self.torch.cuda.ExternalStream(handle, device=self.buf.device)
            self._streams[handle] = s
        return s

    def _allreduce(self, user, op, off, cnt, stream=None):
        try:
            t = self.buf[off:off + cnt]
            rop = self.dist.ReduceOp.SUM if op == 0 else self.dist.ReduceOp.MAX
            if self.ordered:
                # the NCCL process group orders the collective after the current stream's work
                # and makes the current stream wait for it (no host wait)
                with self.torch.cuda.stream(self._stream(stream)):
                    self.dist.all_reduce(t, op=rop, group=self.group)
            elif self.buf.is_cuda:
                # the library drained its stream; complete the reduction before returning
                self.dist.all_reduce(t, op=rop, group=self.group)
                self.torch.cuda.synchronize(self.buf.device)
            else:
                self.dist.all_reduce(t, op=rop, group=self.group)
            self.calls += 1
            return 0
        except Exception:   # never raise through the C stack
            return 1


def dense_ldlt_solve(S, b, device=0, tiled=False, path=None):
    """Device LDL^T solve of the reduced camera system (test hook) -> (x, zero_pivot).
    tiled=True forces the pad + per-step panel + backward kernels even for n <= 64 (path 1);
    path=2 forces the pipelined factorisation (one launch); path=3 the per-step panels with the
    one-workgroup backward substitution (every path above 96 tiles); default path 0 = what BA
    uses."""
    from . import lib, _check
    S = np.ascontiguousarray(S, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    n = S.shape[0]
    x = np.zeros(n)
    zp = ctypes.c_int32()
    if path is None:
        path = 1 if tiled else 0
    _check(lib().mcs_dense_ldlt_solve_ex(int(device), _p(S), n, _p(b), _p(x), ctypes.byref(zp),
                                         int(path)))
    return x, zp.value


def set_ldlt_wait_ticks(ticks):
    """Test hook: the pipelined LDL^T's hand-off wait bound (100 MHz ticks; <= 0 = default)."""
    from . import lib, _check
    _check(lib().mcs_ldlt_set_wait_ticks(int(ticks)))


BA_STAGES = ("linearize", "schur", "exchange", "solve", "update")
BA_HOST_PHASES = ("checks", "structure", "upload", "download", "lba_bookkeeping")
LDLT_BANDED, LDLT_DENSE, LDLT_PER_STEP = 0, 1, 2
