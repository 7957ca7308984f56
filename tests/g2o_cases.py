"""The cases of tests/golden/g2o_optimize_ref.npz: how each problem is made, how the oracle and
the product run it, and how a run is compared with what the reference's g2o recorded.

Shared by the generator (tests/golden/gen_g2o_optimize_ref.py: the `measured_*` keys are
`compare(oracle run, g2o run)`) and tests/test_g2o_optimize_ref.py.

A run is a dict of
  discrete fields (must be equal): it, stop, active, ret [per round], and the sets a kind has
    (edge_inlier / point_write / write_back, outlier / n_good);
  continuous fields: trace (the rounds' chi2 traces one after the other), lam and chi2 [per
    round], poses, points.

Bounds (the project's GPU-against-oracle ones, tests/test_ba.py, test_global_ba.py,
test_pose_opt.py): trace, chi2 and lambda rel 1e-6; poses abs 1e-6 (1e-8 for the single 6x6
system of a pose-only run); points with >= 3 observations 1e-5 of the point's scale
max(1, |X|).  The recorded oracle-against-g2o differences must sit 10x inside them.
"""
import ctypes as C
import hashlib

import numpy as np

TRACE = 32
BOUNDS = dict(trace=1e-6, chi2=1e-6, lam=1e-6, poses=1e-6, poses_pose_only=1e-8, points=1e-5)
MARGIN = 10.0

LOCAL_KW = dict(n_local=3, n_fixed=1, n_points=300, target_edges=2000, seed=5, outlier_frac=0.02,
                noise_scale=0.05, pose_noise=(1e-3, 1e-3), point_noise=1e-3)
GLOBAL_KW = dict(n_kf=24, n_points=3000, target_edges=24000, ncams=8, seed=1)
GBAND_KW = dict(n_kf=33, n_points=800, target_edges=5000, step=0.6, max_range=3.0, ncams=8, seed=1)
PCONV_KW = dict(seed=5, outlier_frac=0.0, noise_scale=0.05, pose_noise=(1e-4, 1e-4))

# name -> (kind, what makes the problem); kinds: opt (one optimize(10) with a caller's flag),
# local (LocalBundleAdjustment's two rounds, caller's flag), global (optimize(15), caller's
# flag; pose_only fixes the points), pose (PoseOptimization's two rounds, flag NULL)
CASES = {
    "L": ("opt", "make_problem(**LOCAL_KW)"),
    "Lperm": ("opt", "L with the pose ids reversed and the point ids shuffled (seed 11)"),
    "C": ("local", "make_problem(seed=1)"),
    "G": ("global", "make_global_problem(**GLOBAL_KW)"),
    "Gpose": ("global", "make_global_problem(**GLOBAL_KW), points fixed"),
    "Gband": ("global", "make_global_problem(**GBAND_KW): BANDED_CASES['K33'], band 2 of T = 3"),
    "P0": ("pose", "make_pose_problem(seed=0)"),
    "Pconv": ("pose", "make_pose_problem(**PCONV_KW)"),
    "S": ("opt", "structure_problem(): 50 hand-picked edges"),
    "Soff": ("opt", "structure_problem() with every edge at level 1"),
}
POSE_ONLY = ("Gpose", "P0", "Pconv")
_PROBLEMS = {}


def structure_problem():
    """<= 50 edges over 2 fixed + 3 free poses that hold: a free pose (4) whose edges are all at
    level 1, a point (0) seen only by fixed poses, a point (1) with a single edge, and one
    (pose, point) pair twice.  -> (problem, edge_level)."""
    from mcs_amd import ba
    pr = ba.make_problem(n_local=3, n_fixed=2, n_points=16, target_edges=10 ** 6, seed=3,
                         outlier_frac=0.0, noise_scale=0.3, pose_noise=(1e-3, 1e-2),
                         point_noise=1e-2)
    ep, eq = pr["edge_pose"], pr["edge_point"]
    keep = []
    for q in range(len(pr["points"])):
        es = np.where(eq == q)[0]
        if q == 0:
            es = np.array([es[ep[es] == 0][0], es[ep[es] == 1][0]])
        elif q == 1:
            es = es[ep[es] == 2][:1]
        else:   # three poses per point, taken in turn
            es = np.array([es[ep[es] == (q + j) % 5][0] for j in range(3)], int)
        keep.extend(es.tolist())
    keep = np.array(sorted(keep)[:49])
    dup = keep[(ep[keep] == 2) & (eq[keep] > 1)][0]
    out = dict(pr)
    for k in ("edge_pose", "edge_point", "edge_cam", "edge_info"):
        out[k] = np.concatenate([pr[k][keep], pr[k][[dup]]])
    out["edge_meas"] = np.concatenate([pr["edge_meas"][keep], pr["edge_meas"][[dup]] + 0.5])
    level = (out["edge_pose"] == 4).astype(np.uint8)
    ep, eq = out["edge_pose"], out["edge_point"]
    assert len(ep) <= 50 and level.sum() >= 1
    assert (eq == 0).sum() >= 1 and np.all(out["pose_fixed"][ep[eq == 0]] == 1)
    assert (eq == 1).sum() == 1
    assert len(set(zip(ep.tolist(), eq.tolist()))) == len(ep) - 1
    return out, level


def problem(name):
    """-> (problem dict, edge_level or None); built once, never written to."""
    from mcs_amd import ba
    if name not in _PROBLEMS:
        lvl = None
        if name in ("L", "Lperm"):
            pr = ba.make_problem(**LOCAL_KW)
        elif name == "C":
            pr = ba.make_problem(seed=1)
        elif name in ("G", "Gpose"):
            pr = ba.make_global_problem(**GLOBAL_KW)
        elif name == "Gband":
            pr = ba.make_global_problem(**GBAND_KW)
        elif name == "P0":
            pr = ba.make_pose_problem(seed=0)
        elif name == "Pconv":
            pr = ba.make_pose_problem(**PCONV_KW)
        else:
            pr, lvl = structure_problem()
            if name == "Soff":
                lvl = np.ones_like(lvl)
        _PROBLEMS[name] = (pr, lvl)
    return _PROBLEMS[name]


def perm_ids(pr, seed=11):
    """Lperm's vertex ids: poses reversed, points shuffled behind them (Mc / IO follow)."""
    n, m = len(pr["poses"]), len(pr["points"])
    pose_id = np.arange(n)[::-1].astype(np.int64)
    point_id = (n + np.random.default_rng(seed).permutation(m)).astype(np.int64)
    return pose_id, point_id


def problem_sha(pr, lvl=None):
    h = hashlib.sha256()
    for k in ("poses", "pose_fixed", "points", "mc", "cam", "edge_pose", "edge_point", "edge_cam",
              "edge_meas", "edge_info"):
        h.update(np.ascontiguousarray(pr[k]).tobytes())
    h.update(np.float64(pr["huber_delta"]).tobytes())
    if lvl is not None:
        h.update(np.ascontiguousarray(lvl, np.uint8).tobytes())
    return h.hexdigest()


def _ret(rep):
    return -1 if rep.n_active_poses + rep.n_active_points == 0 else rep.iterations


def _rounds(reps, traces, **more):
    reps = list(reps)
    out = dict(it=np.array([r.iterations for r in reps], np.int32),
               stop=np.array([r.stop_flag for r in reps], np.int32),
               active=np.array([[r.n_active_edges, r.n_active_poses, r.n_active_points] for r in reps],
                               np.int32),
               ret=np.array([_ret(r) for r in reps], np.int32),
               lam=np.array([r.lambda_final for r in reps]),
               chi2=np.array([[r.chi2_initial, r.chi2_final] for r in reps]),
               trace=np.concatenate([np.asarray(t, np.float64)[:r.iterations] for r, t in zip(reps, traces)]))
    out.update(more)
    return out


def _reports(n):
    from mcs_amd import ba
    tr = [np.zeros(TRACE) for _ in range(n)]
    reps = [ba.BAReport(0, 0, 0, 0, 0, 0, 0, 0, t.ctypes.data_as(C.c_void_p), TRACE) for t in tr]
    return reps, tr


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(name, solver=None):
    """Run case `name` on the oracle (solver None) or on the product (a ba.Solver)."""
    from mcs_amd import ba, _check
    from tests import oracle_bind as ob
    kind = CASES[name][0]
    pr, lvl = problem(name)
    s = ba.as_struct(pr)
    poses = np.ascontiguousarray(pr["poses"], np.float64).copy()
    points = np.ascontiguousarray(pr["points"], np.float64).copy()
    n = len(pr["edge_pose"])
    L = ob._ba_sigs() if solver is None else solver._lib
    sf = C.c_int32(0)

    def call(oname, gname, *args):
        if solver is None:
            f = getattr(L, oname)
            f.restype = C.c_int
            rc = f(*args)
            assert rc == 0, (oname, rc)
        else:
            _check(getattr(L, gname)(solver._h, *args))

    if kind == "opt":
        (rep,), (tr,) = _reports(1)
        o = ba.BAOptions()
        lv = np.zeros(n, np.uint8) if lvl is None else np.ascontiguousarray(lvl, np.uint8)
        chi = np.zeros(n)
        call("oracle_ba_optimize", "mcs_ba_optimize", C.byref(s), C.byref(o), _p(poses), _p(points),
             _p(lv), _p(chi), C.byref(sf), C.byref(rep))
        return _rounds([rep], [tr], poses=poses, points=points)
    if kind == "global":
        (rep,), (tr,) = _reports(1)
        po = C.c_int32(1 if name == "Gpose" else 0)
        if solver is None:
            call("oracle_global_ba", None, C.byref(s), po, _p(poses), _p(points), C.byref(sf),
                 C.byref(rep))
        else:
            call(None, "mcs_global_ba", C.byref(s), po, _p(poses), _p(points), C.byref(sf),
                 C.byref(rep), None)
        return _rounds([rep], [tr], poses=poses, points=points)
    if kind == "local":
        reps, tr = _reports(2)
        inl = np.zeros(n, np.uint8)
        pw = np.zeros(len(points), np.uint8)
        wb = C.c_int32()
        call("oracle_local_ba_ex", "mcs_local_ba_ex", C.byref(s), None, _p(poses), _p(points), _p(inl),
             _p(pw), C.byref(wb), C.byref(sf), C.byref(reps[0]), C.byref(reps[1]))
        return _rounds(reps, tr, poses=poses, points=points, edge_inlier=inl, point_write=pw,
                       write_back=np.int32(wb.value))
    reps, tr = _reports(2)
    pose = poses[0].copy()
    out = np.zeros(n, np.uint8)
    bad = C.c_double()
    if solver is None:
        f = L.oracle_pose_optimization
        f.restype = C.c_int
        ngood = f(C.byref(s), _p(pose), _p(out), C.byref(bad), C.byref(reps[0]), C.byref(reps[1]))
    else:
        ng = C.c_int32()
        _check(L.mcs_pose_optimization(solver._h, C.byref(s), _p(pose), _p(out), C.byref(ng),
                                       C.byref(bad), C.byref(reps[0]), C.byref(reps[1])))
        ngood = ng.value
    return _rounds(reps, tr, poses=pose[None].copy(), points=points, outlier=out,
                   n_good=np.int32(ngood))


DISCRETE = ("it", "stop", "active", "ret", "edge_inlier", "point_write", "write_back", "outlier",
            "n_good")


def well_constrained(name):
    pr, _ = problem(name)
    return np.bincount(pr["edge_point"], minlength=len(pr["points"])) >= 3


def compare(name, got, ref, scale=1.0):
    """Differences of run `got` from run `ref` (dicts or the fixture's `name/` keys).
    -> (list of discrete fields that differ, dict of measured figures, dict of the bounds,
    each divided by `scale`)."""
    bad = [k for k in DISCRETE if k in ref and not np.array_equal(np.asarray(got[k]), np.asarray(ref[k]))]
    m = {}
    if len(ref["trace"]) and len(got["trace"]) == len(ref["trace"]):
        m["trace"] = float(np.abs(got["trace"] / ref["trace"] - 1).max())
    act = np.asarray(ref["ret"]) > 0
    if act.any() and np.array_equal(got["ret"], ref["ret"]):
        m["chi2"] = float(np.abs(np.asarray(got["chi2"])[act] / np.asarray(ref["chi2"])[act] - 1).max())
        m["lam"] = float(np.abs(np.asarray(got["lam"])[act] / np.asarray(ref["lam"])[act] - 1).max())
    m["poses"] = float(np.abs(np.asarray(got["poses"]) - np.asarray(ref["poses"])).max())
    wc = well_constrained(name)
    if name in POSE_ONLY:
        m["points"] = float(np.abs(np.asarray(got["points"]) - np.asarray(ref["points"])).max())
    elif wc.any():
        P, Q = np.asarray(got["points"])[wc], np.asarray(ref["points"])[wc]
        m["points"] = float((np.abs(P - Q).max(axis=1) / np.maximum(1.0, np.linalg.norm(Q, axis=1))).max())
    b = {k: (0.0 if k == "points" and name in POSE_ONLY else
             BOUNDS["poses_pose_only" if k == "poses" and name in POSE_ONLY else k]) / scale for k in m}
    return bad, m, b


def from_fixture(z, name):
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def check(name, got, ref, scale=1.0, label=""):
    """Print every figure, then assert: discrete fields equal, continuous ones inside bound / scale."""
    bad, m, b = compare(name, got, ref, scale)
    print("%s %s: it %s stop %s active %s | " % (label, name, np.asarray(got["it"]).tolist(),
                                                 np.asarray(got["stop"]).tolist(),
                                                 np.asarray(got["active"]).tolist()) +
          " ".join("%s %.3g (bound %.1g)" % (k, m[k], b[k]) for k in m))
    assert not bad, "%s: discrete fields differ: %s" % (name, bad)
    assert len(got["trace"]) == len(ref["trace"])
    for k in m:
        assert m[k] <= b[k], "%s: %s differs by %.3g, bound %.3g" % (name, k, m[k], b[k])
    return m


# ------------------------------------------------------------------------------ linear solver
LIN_SIZES = (6, 60, 66, 132)


def lin_system(n, zero_block=None, seed=0):
    """Block-banded SPD system of 6x6 blocks (two block diagonals beside the main one);
    zero_block = k: block row and column k are exactly zero, so whatever the elimination order
    a pivot of that block is exactly 0."""
    rng = np.random.default_rng(1000 * n + seed)
    nb = n // 6
    S = np.zeros((n, n))
    for i in range(nb):
        for j in range(max(0, i - 2), i):
            B = rng.uniform(-1, 1, (6, 6))
            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
            S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
        A = rng.normal(size=(6, 6))
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = A @ A.T + 30.0 * np.eye(6)
    b = rng.normal(size=n)
    if zero_block is not None:
        k = slice(6 * zero_block, 6 * zero_block + 6)
        S[k, :] = 0.0
        S[:, k] = 0.0
    return S, b


# name -> (n, zero_block): the four SPD sizes (one tile: 6, 60; tiled: 66, 132), a zero block
# row and column in the middle of a tiled system and at the head of a one-tile one
LIN_CASES = {"n6": (6, None), "n60": (60, None), "n66": (66, None), "n132": (132, None),
             "n66zero": (66, 4), "n60zero": (60, 0), "n132zero": (132, 13)}


def lin_coupled_zero(n, k):
    """lin_system(n) with only the diagonal block k zeroed: the off-diagonal blocks stay, so
    whether a pivot becomes exactly 0 depends on the elimination order (the matrix is
    indefinite; no reduced camera system looks like this)."""
    S, b = lin_system(n)
    S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = 0.0
    return S, b


# name -> (n, block): recorded as facts about SimplicialLDLT's fill-reducing order only
LIN_ORDER_CASES = {"n66head": (66, 0), "n66mid": (66, 4), "n132mid": (132, 21)}
