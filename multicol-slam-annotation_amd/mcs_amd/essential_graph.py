"""cOptimizer::OptimizeEssentialGraph on the GPU (include/mcs_essgraph.h): the Sim3 pose graph that
applies a loop correction to the map (reference src/cOptimizerLoopStuff.cpp:273-519, called at
src/cLoopClosing.cpp:648).

  select_edges(ids, parent, has_corrected, loops, cov, loop_connections, current, loop, min_weight=100)
        the edge list of :355-470 on the host -> (edges int32 [E, 3] = v0, v1, kind, counts [4])
  tile_band(n_kf, loop, edges)          the band of the system a host edge list gives
  optimize(Scw, Snc, loop, edges, point_pos, point_ref, point_bad, options=None)
        host entry on NumPy -> dict of the arrays of mcs_essgraph_out and the corrected points
  optimize_device(ws, Scw, Snc, loop, edges, point_pos, point_ref, point_bad, options, out=None)
        the same on torch tensors, stream-ordered on torch's current stream; point_pos in place
  resolve_point_refs_device(kf_id, corrected_by, corrected_ref, ref_kf, current_id)
        the keyframe index per point (:501-507) on torch tensors

  Plan(n_kf, loop, edges, max_edges=None, max_points=0, leaf_size=None, device=0)
        the block-sparse solver's plan for one edge list (any number of keyframes); .info, .arrays()
  optimize_planned_device(plan, Scw, Snc, edges, point_pos, point_ref, point_bad, options, out=None)
        optimize_device with the plan's solver
  optimize_sparse(Scw, Snc, loop, edges, ...)     optimize() with a plan made for the call

Keyframes come in ascending id order and none is bad.  A Sim3 is 8 doubles: s, qw qx qy qz,
tx ty tz.  Scw holds CorrectedSim3 where present, else Sim3(R, t, 1) of the inverse pose; Snc
NonCorrectedSim3 where present, else Scw.  A CSR argument is (ptr, idx) or (ptr, idx, weight).
There is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import McsError, _Workspace, _check, lib

MAX_ITERATIONS = 64

_O_FIELDS = (("sim3", np.float64, ("N", 8)), ("rot", np.float64, ("N", 9)), ("pose", np.float64, ("N", 16)),
             ("iterations", np.int32, (1,)), ("trials", np.int32, (MAX_ITERATIONS,)),
             ("chi2", np.float64, (MAX_ITERATIONS,)), ("lambda", np.float64, (1,)), ("edge_chi2", np.float64, ("E",)),
             ("status", np.int32, (1,)))


class EssGraphMap(ctypes.Structure):
    """Mirror of mcs_essgraph_map."""
    _fields_ = [("n_kf", ctypes.c_int32), ("kf_id", ctypes.c_void_p), ("parent", ctypes.c_void_p),
                ("has_corrected", ctypes.c_void_p), ("loop_ptr", ctypes.c_void_p), ("loop_idx", ctypes.c_void_p),
                ("cov_ptr", ctypes.c_void_p), ("cov_idx", ctypes.c_void_p), ("cov_weight", ctypes.c_void_p),
                ("lc_ptr", ctypes.c_void_p), ("lc_idx", ctypes.c_void_p), ("lc_weight", ctypes.c_void_p),
                ("current_index", ctypes.c_int32), ("loop_index", ctypes.c_int32), ("min_weight", ctypes.c_int32)]


class EssGraphOptions(ctypes.Structure):
    """Mirror of mcs_essgraph_options."""
    _fields_ = [("iterations", ctypes.c_int32), ("terminate_max_iter", ctypes.c_int32),
                ("gain_threshold", ctypes.c_double), ("lambda0", ctypes.c_double), ("max_trials", ctypes.c_int32),
                ("tile_band", ctypes.c_int32)]


class EssGraphOut(ctypes.Structure):
    """Mirror of mcs_essgraph_out."""
    _fields_ = [(k, ctypes.c_void_p) for k, _, _ in _O_FIELDS]


def default_options(**kw):
    """mcs_essgraph_default_options, then the keyword overrides."""
    o = EssGraphOptions()
    lib().mcs_essgraph_default_options(ctypes.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise ValueError("no such option: %s" % k)
        setattr(o, k, v)
    return o


def out_shapes(N, E):
    """name -> (dtype, shape) of the buffers of mcs_essgraph_out."""
    dim = {"N": N, "E": E}
    return {k: (dt, tuple(dim.get(s, s) for s in shp)) for k, dt, shp in _O_FIELDS}


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def select_edges(ids, parent, has_corrected, loops, cov, loop_connections, current, loop, min_weight=100):
    """mcs_essgraph_select_edges -> (edges int32 [E, 3], counts int32 [4])."""
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    N = len(ids)
    keep = [ids, _i32(parent), np.ascontiguousarray(has_corrected, np.uint8).reshape(-1)]
    for csr in (loops, cov, loop_connections):
        keep += [_i32(a) for a in csr]
    if len(keep) != 3 + 2 + 3 + 3 or any(len(a) != N for a in keep[:3]):
        raise ValueError("select_edges: loops = (ptr, idx); cov, loop_connections = (ptr, idx, weight)")
    m = EssGraphMap(N, *[a.ctypes.data for a in keep], int(current), int(loop), int(min_weight))
    n, counts = ctypes.c_int32(0), np.zeros(4, np.int32)
    rc = lib().mcs_essgraph_select_edges(ctypes.byref(m), None, 0, ctypes.byref(n), counts.ctypes.data)
    if rc not in (0, -2):
        _check(rc)
    edges = np.zeros((n.value, 3), np.int32)
    _check(lib().mcs_essgraph_select_edges(ctypes.byref(m), edges.ctypes.data, n.value, ctypes.byref(n),
                                           counts.ctypes.data))
    return edges, counts


def tile_band(n_kf, loop, edges):
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
    return int(lib().mcs_essgraph_tile_band(int(n_kf), int(loop), e.ctypes.data, len(e)))


def supported(n_kf, band=0):
    """True when the solver takes n_kf keyframes at this tile band (size arithmetic only)."""
    return lib().mcs_essgraph_supported(int(n_kf), int(band)) == 0


class Workspace(_Workspace):
    """mcs_essgraph_workspace: device scratch for <= max_kf keyframes, max_edges edges, max_points points."""

    def __init__(self, max_kf, max_edges, max_points, device=0):
        super().__init__("mcs_essgraph_workspace_create", "mcs_essgraph_workspace_destroy", device, max_kf, max_edges,
                         max_points)


def _stream(device):
    import torch
    return torch.cuda.current_stream("cuda:%d" % device).cuda_stream


def new_out(N, E, device=0, edge_chi2=True):
    """An EssGraphOut of fresh device tensors -> (EssGraphOut, tensors by name)."""
    import torch
    s, ts = EssGraphOut(), {}
    for k, (dt, shp) in out_shapes(N, E).items():
        if k == "edge_chi2" and not edge_chi2:
            continue
        ts[k] = torch.zeros(shp, dtype=getattr(torch, np.dtype(dt).name), device="cuda:%d" % device)
        setattr(s, k, ts[k].data_ptr())
    return s, ts


def resolve_point_refs_device(kf_id, corrected_by, corrected_ref, ref_kf, current_id, out=None, device=0):
    """mcs_essgraph_resolve_point_refs_device on int64 torch tensors -> int32 [P]."""
    import torch
    P = int(corrected_by.shape[0])
    if out is None:
        out = torch.empty(P, dtype=torch.int32, device=kf_id.device)
    _check(lib().mcs_essgraph_resolve_point_refs_device(int(kf_id.shape[0]), kf_id.data_ptr(), P,
                                                        corrected_by.data_ptr(), corrected_ref.data_ptr(),
                                                        ref_kf.data_ptr(), int(current_id), out.data_ptr(),
                                                        _stream(device)))
    return out


def optimize_device(ws, Scw, Snc, loop, edges, point_pos, point_ref, point_bad, options=None, out=None, device=0):
    """mcs_optimize_essential_graph_device on torch tensors, stream-ordered.  point_pos float64
    [P, 3] is corrected in place.  options.tile_band must cover the edges (tile_band()).  out:
    (EssGraphOut, tensors) of new_out, made when not given -> the tensors by name; read `status`."""
    device = ws.device if ws is not None else device
    o = options if options is not None else default_options()
    N, E = int(Scw.shape[0]), int(edges.shape[0])
    P = int(point_pos.shape[0]) if point_pos is not None else 0
    if out is None:
        out = new_out(N, E, device)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_optimize_essential_graph_device(ws._h if ws is not None else None, N, ptr(Scw), ptr(Snc),
                                                     int(loop), E, ptr(edges), P, ptr(point_pos), ptr(point_ref),
                                                     ptr(point_bad), ctypes.byref(o), ctypes.byref(out[0]),
                                                     _stream(device)))
    return out[1]


def optimize(Scw, Snc, loop, edges, point_pos=None, point_ref=None, point_bad=None, options=None, device=0):
    """Host entry (mcs_optimize_essential_graph) -> dict: the arrays of mcs_essgraph_out by name and
    `points`, the corrected positions.  options: EssGraphOptions, or a dict of overrides; its
    tile_band is derived from the edges when left 0."""
    Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8)
    Snc = np.ascontiguousarray(Snc, np.float64).reshape(-1, 8)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
    N, E = len(Scw), len(edges)
    pos = np.ascontiguousarray(point_pos if point_pos is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3).copy()
    P = len(pos)
    ref = np.ascontiguousarray(point_ref if point_ref is not None else np.zeros(0), np.int32).reshape(-1)
    bad = np.ascontiguousarray(point_bad if point_bad is not None else np.zeros(0), np.uint8).reshape(-1)
    if len(Snc) != N or len(ref) != P or len(bad) != P:
        raise ValueError("optimize: Scw / Snc and the point arrays must agree in length")
    o = options if isinstance(options, EssGraphOptions) else default_options(**(options or {}))
    if o.tile_band == 0 and 0 <= int(loop) < N:
        o.tile_band = tile_band(N, loop, edges)
    out, arrs = EssGraphOut(), {}
    for k, (dt, shp) in out_shapes(N, E).items():
        arrs[k] = np.zeros(shp, dt)
        setattr(out, k, arrs[k].ctypes.data)
    _check(lib().mcs_optimize_essential_graph(int(device), N, Scw.ctypes.data, Snc.ctypes.data, int(loop), E,
                                              edges.ctypes.data if E else None, P, pos.ctypes.data if P else None,
                                              ref.ctypes.data if P else None, bad.ctypes.data if P else None,
                                              ctypes.byref(o), ctypes.byref(out)))
    return dict(arrs, points=pos)


class PlanOptions(ctypes.Structure):
    """Mirror of mcs_essgraph_plan_options."""
    _fields_ = [("leaf_size", ctypes.c_int32)]


class PlanInfo(ctypes.Structure):
    """Mirror of mcs_essgraph_plan_info."""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_kf", "loop_index", "free_blocks", "leaf_size", "supernodes", "levels",
                                              "max_supernode_columns", "solver_launches_per_trial",
                                              "launches_per_trial")] + \
               [(k, ctypes.c_int64) for k in ("a_blocks", "l_blocks", "panel_blocks", "flops_per_factor",
                                              "device_bytes")] + [("digest", ctypes.c_uint64)]


class PlanArrays(ctypes.Structure):
    """Mirror of mcs_essgraph_plan_arrays."""
    _fields_ = [("perm", ctypes.c_void_p), ("col0", ctypes.c_void_p), ("row_ptr", ctypes.c_void_p),
                ("rows", ctypes.c_void_p), ("n_rows", ctypes.c_int32), ("parent", ctypes.c_void_p),
                ("level", ctypes.c_void_p), ("block_off", ctypes.c_void_p), ("a_block", ctypes.c_void_p)]


class Plan:
    """mcs_essgraph_plan: the block-sparse LDL^T planned on the host for one edge list, with the
    device storage of its calls.  edges int32 [E, 3] on the host.  device < 0: a host-only plan
    (info and arrays).  .info: dict of mcs_essgraph_plan_info, with `fill` = l_blocks / a_blocks."""

    def __init__(self, n_kf, loop, edges, max_edges=None, max_points=0, leaf_size=None, device=0):
        e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        o = PlanOptions()
        lib().mcs_essgraph_plan_default_options(ctypes.byref(o))
        if leaf_size is not None:
            o.leaf_size = int(leaf_size)
        h = ctypes.c_void_p()
        _check(lib().mcs_essgraph_plan_create(int(device), int(n_kf), int(loop), e.ctypes.data if len(e) else None, len(e),
                                              len(e) if max_edges is None else int(max_edges), int(max_points),
                                              ctypes.byref(o), ctypes.byref(h)))
        self._h, self.device, self.n_kf, self.loop = h, int(device), int(n_kf), int(loop)
        i = PlanInfo()
        _check(lib().mcs_essgraph_plan_get_info(h, ctypes.byref(i)))
        self.info = {k: int(getattr(i, k)) for k, _ in PlanInfo._fields_}
        self.info["fill"] = self.info["l_blocks"] / max(1, self.info["a_blocks"])

    def arrays(self):
        """Copies of the plan's host arrays (mcs_essgraph_plan_arrays) by name."""
        a = PlanArrays()
        _check(lib().mcs_essgraph_plan_get_arrays(self._h, ctypes.byref(a)))
        S, n = self.info["supernodes"], self.info["free_blocks"]

        def arr(ptr, count, ct, dt):
            if count == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), (count,)).astype(dt, copy=True)
        i32 = lambda ptr, count: arr(ptr, count, ctypes.c_int32, np.int32)  # noqa: E731
        return dict(perm=i32(a.perm, n), col0=i32(a.col0, S + 1), row_ptr=i32(a.row_ptr, S + 1),
                    rows=i32(a.rows, a.n_rows), parent=i32(a.parent, S), level=i32(a.level, S),
                    block_off=i32(a.block_off, S + 1),
                    a_block=arr(a.a_block, self.info["panel_blocks"], ctypes.c_uint8, np.uint8))

    def close(self):
        if getattr(self, "_h", None):
            lib().mcs_essgraph_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def optimize_planned_device(plan, Scw, Snc, edges, point_pos, point_ref, point_bad, options=None, out=None, loop=None):
    """mcs_optimize_essential_graph_planned_device on torch tensors, stream-ordered; as
    optimize_device, with the plan's solver (options.tile_band is ignored).  loop defaults to the
    plan's."""
    o = options if options is not None else default_options()
    N, E = int(Scw.shape[0]), int(edges.shape[0])
    P = int(point_pos.shape[0]) if point_pos is not None else 0
    if out is None:
        out = new_out(N, E, plan.device)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _check(lib().mcs_optimize_essential_graph_planned_device(plan._h, N, ptr(Scw), ptr(Snc),
                                                             plan.loop if loop is None else int(loop), E, ptr(edges), P,
                                                             ptr(point_pos), ptr(point_ref), ptr(point_bad),
                                                             ctypes.byref(o), ctypes.byref(out[0]),
                                                             _stream(plan.device)))
    return out[1]


def optimize_sparse(Scw, Snc, loop, edges, point_pos=None, point_ref=None, point_bad=None, options=None, device=0):
    """mcs_optimize_essential_graph_sparse: optimize() through a plan made for the call; any number
    of keyframes the plan's limits take."""
    Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8)
    Snc = np.ascontiguousarray(Snc, np.float64).reshape(-1, 8)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
    N, E = len(Scw), len(edges)
    pos = np.ascontiguousarray(point_pos if point_pos is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3).copy()
    P = len(pos)
    ref = np.ascontiguousarray(point_ref if point_ref is not None else np.zeros(0), np.int32).reshape(-1)
    bad = np.ascontiguousarray(point_bad if point_bad is not None else np.zeros(0), np.uint8).reshape(-1)
    if len(Snc) != N or len(ref) != P or len(bad) != P:
        raise ValueError("optimize_sparse: Scw / Snc and the point arrays must agree in length")
    o = options if isinstance(options, EssGraphOptions) else default_options(**(options or {}))
    out, arrs = EssGraphOut(), {}
    for k, (dt, shp) in out_shapes(N, E).items():
        arrs[k] = np.zeros(shp, dt)
        setattr(out, k, arrs[k].ctypes.data)
    _check(lib().mcs_optimize_essential_graph_sparse(int(device), N, Scw.ctypes.data, Snc.ctypes.data, int(loop), E,
                                                     edges.ctypes.data if E else None, P, pos.ctypes.data if P else None,
                                                     ref.ctypes.data if P else None, bad.ctypes.data if P else None,
                                                     ctypes.byref(o), ctypes.byref(out)))
    return dict(arrs, points=pos)


__all__ = ["Plan", "PlanOptions", "PlanInfo", "PlanArrays", "optimize_planned_device", "optimize_sparse",
           "EssGraphMap", "EssGraphOptions", "EssGraphOut", "Workspace", "default_options", "out_shapes", "select_edges",
           "tile_band", "supported", "new_out", "resolve_point_refs_device", "optimize_device", "optimize",
           "MAX_ITERATIONS", "McsError"]
