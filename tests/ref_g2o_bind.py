"""ctypes binding of oracle/_ref/libg2o_ref.so: the reference's own g2o behind
oracle/ref_g2o_driver.cpp.  Test infrastructure only; the library exists only where the
reference checkout was there to build it from (`available()`), and nothing on a GPU reads it.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libg2o_ref.so")

_P = C.c_void_p
_lib = None


def available():
    return os.path.exists(REF_LIB)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_LIB)
        L.ref_g2o_create.restype = _P
        L.ref_g2o_create.argtypes = [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P]
        L.ref_g2o_create_ex.restype = _P
        L.ref_g2o_create_ex.argtypes = [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32]
        L.ref_g2o_round.restype = C.c_int
        L.ref_g2o_round.argtypes = [_P, _P, C.c_int32, _P, _P, _P, _P, _P]
        L.ref_g2o_destroy.restype = None
        L.ref_g2o_destroy.argtypes = [_P]
        L.ref_g2o_refused_vertices.restype = C.c_int32
        L.ref_g2o_refused_vertices.argtypes = [_P]
        L.ref_g2o_last_trials.restype = C.c_int32
        L.ref_g2o_last_trials.argtypes = [_P, C.c_int32]
        L.ref_g2o_optimize.restype = C.c_int
        L.ref_g2o_optimize.argtypes = [_P] * 8 + [C.c_int32, _P, _P]
        L.ref_g2o_linear_solve.restype = C.c_int
        L.ref_g2o_linear_solve.argtypes = [C.c_int32, _P, _P, _P, _P, _P]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(_P) if a is not None else None


class Graph:
    """One SparseOptimizer over `pr` (ref_g2o_create); `round()` = setLevel +
    initializeOptimization(0) + optimize(n).  has_stop_flag False = pbStopFlag NULL;
    dense_solver = BlockSolverX over LinearSolverDense, PoseOptimization's choice."""

    def __init__(self, pr, options=None, points_fixed=False, has_stop_flag=True, pose_id=None,
                 point_id=None, dense_solver=False):
        from mcs_amd import ba
        self.pr = pr
        self._s = ba.as_struct(pr)
        self.o = options or ba.BAOptions()
        self.poses = np.ascontiguousarray(pr["poses"], np.float64).copy()
        self.points = np.ascontiguousarray(pr["points"], np.float64).copy()
        self.has_flag = bool(has_stop_flag)
        pi = None if pose_id is None else np.ascontiguousarray(pose_id, np.int64)
        qi = None if point_id is None else np.ascontiguousarray(point_id, np.int64)
        self._h = lib().ref_g2o_create_ex(C.byref(self._s), C.byref(self.o), _p(self.poses),
                                          _p(self.points), int(bool(points_fixed)),
                                          int(self.has_flag), _p(pi), _p(qi), int(bool(dense_solver)))
        self.refused = lib().ref_g2o_refused_vertices(self._h)

    def round(self, n_iter, edge_level=None, stop_flag=0, trace=32):
        from mcs_amd import ba
        n = len(self.pr["edge_pose"])
        lvl = None if edge_level is None else np.ascontiguousarray(edge_level, np.uint8)
        chi = np.zeros(max(n, 1))
        tr = np.zeros(trace)
        rep = ba.BAReport(0, 0, 0, 0, 0, 0, 0, 0, _p(tr), trace)
        sf = C.c_int32(int(stop_flag)) if self.has_flag else None
        ret = lib().ref_g2o_round(self._h, _p(lvl), int(n_iter), None if sf is None else C.byref(sf),
                                  C.byref(rep), _p(self.poses), _p(self.points), _p(chi))
        nt = lib().ref_g2o_last_trials(None, 0)
        trials = np.zeros(max(nt, 1), np.int32)
        lib().ref_g2o_last_trials(_p(trials), nt)
        return dict(ret=ret, poses=self.poses.copy(), points=self.points.copy(), edge_chi2=chi[:n].copy(),
                    report=rep, stop_flag=None if sf is None else sf.value,
                    trace=tr[:min(trace, rep.iterations)].copy(), trials=trials[:nt].copy())

    def close(self):
        if self._h:
            lib().ref_g2o_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def optimize(pr, options=None, edge_level=None, stop_flag=None, trace=32, points_fixed=False,
             pose_id=None, point_id=None):
    """ref_g2o_optimize: the arguments and results of oracle_bind.ba_optimize, plus the ids."""
    from mcs_amd import ba
    s = ba.as_struct(pr)
    o = options or ba.BAOptions()
    poses = np.ascontiguousarray(pr["poses"], np.float64).copy()
    points = np.ascontiguousarray(pr["points"], np.float64).copy()
    n = len(pr["edge_pose"])
    lvl = None if edge_level is None else np.ascontiguousarray(edge_level, np.uint8)
    chi = np.zeros(max(n, 1))
    tr = np.zeros(trace)
    rep = ba.BAReport(0, 0, 0, 0, 0, 0, 0, 0, _p(tr), trace)
    sf = None if stop_flag is None else C.c_int32(int(stop_flag))
    pi = None if pose_id is None else np.ascontiguousarray(pose_id, np.int64)
    qi = None if point_id is None else np.ascontiguousarray(point_id, np.int64)
    ret = lib().ref_g2o_optimize(C.byref(s), C.byref(o), _p(poses), _p(points), _p(lvl), _p(chi),
                                 None if sf is None else C.byref(sf), C.byref(rep),
                                 int(bool(points_fixed)), _p(pi), _p(qi))
    nt = lib().ref_g2o_last_trials(None, 0)
    trials = np.zeros(max(nt, 1), np.int32)
    lib().ref_g2o_last_trials(_p(trials), nt)
    return dict(ret=ret, poses=poses, points=points, edge_chi2=chi[:n].copy(), report=rep,
                stop_flag=None if sf is None else sf.value,
                trace=tr[:min(trace, rep.iterations)].copy(), trials=trials[:nt].copy())


def linear_solve(S, b):
    """LinearSolverEigen<6x6>::solve on the upper block triangle of the dense symmetric S
    (blocks that are entirely zero are left out, as a SparseBlockMatrix would not hold them;
    diagonal blocks are always present) -> (x, solve()'s bool)."""
    S = np.ascontiguousarray(S, np.float64)
    nb = S.shape[0] // 6
    rows, cols, blocks = [], [], []
    for c in range(nb):
        for r in range(c + 1):
            blk = S[6 * r:6 * r + 6, 6 * c:6 * c + 6]
            if r == c or np.any(blk != 0):
                rows.append(r)
                cols.append(c)
                blocks.append(blk)
    rows = np.asarray(rows, np.int32)
    cols = np.asarray(cols, np.int32)
    blocks = np.ascontiguousarray(np.stack(blocks), np.float64)
    bb = np.ascontiguousarray(b, np.float64)
    x = np.zeros(6 * nb)
    ok = lib().ref_g2o_linear_solve(len(rows), _p(rows), _p(cols), _p(blocks), _p(bb), _p(x))
    assert ok >= 0
    return x, bool(ok)
