"""optimize() against the reference's own g2o, built from its sources.

tests/golden/g2o_optimize_ref.npz holds what the reference's SparseOptimizer + BlockSolver_6_3 +
LinearSolverEigen + OptimizationAlgorithmLevenberg + SparseOptimizerTerminateAction +
RobustKernelHuber compute (oracle/ref_g2o.mk builds them from the reference checkout into
oracle/_ref/libg2o_ref.so; oracle/ref_g2o_driver.cpp supplies additive vertices and an edge
whose error and Jacobian are oracle_ba_edge, the one seam that stays pinned elsewhere) on the
cases of tests/g2o_cases.py: LocalBA-size optimize(10) under two vertex-id orders, config C's two
rounds, GlobalBA dense / pose-only / banded, PoseOptimization with the terminate action's
auxiliary flag carried into round 2, a 46-edge graph of structural corner cases, and
LinearSolverEigen::solve on block-banded systems with and without an exactly zero block.

Discrete fields (iterations, stop flags, active counts, optimize()'s return value, the
outlier / inlier / write-back sets, solve()'s bool) must be equal.  Continuous fields use the
bounds the project already holds the product to against the oracle (g2o_cases.BOUNDS; LDL^T
rel 1e-10); the oracle itself must sit 10x inside them.  The `-m gpu` tests read
the committed fixture only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import g2o_cases as gc
from tests import ref_g2o_bind as rg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "g2o_optimize_ref.npz")
LDLT_REL = 1e-10
_Z = {}


def _fix():
    if "z" not in _Z:
        _Z["z"] = np.load(FIXTURE)
    return _Z["z"]


def _no_pivot_ldlt_has_zero_pivot(S):
    """LDL^T in the natural order without pivoting (what ldlt.hip runs): an exact zero pivot?"""
    A = np.array(S, np.float64)
    n = len(A)
    for j in range(n):
        if A[j, j] == 0.0:
            return True
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j]) / A[j, j]
    return False


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", list(gc.CASES))
def test_oracle_reproduces_g2o(name):
    z = _fix()
    pr, lvl = gc.problem(name)
    assert str(z[name + "/sha"]) == gc.problem_sha(pr, lvl), "the case's inputs changed"
    m = gc.check(name, gc.run(name), gc.from_fixture(z, name), scale=gc.MARGIN, label="oracle")
    for k, v in m.items():   # what the generator measured is what this run measures
        assert abs(float(z["measured_%s_%s" % (name, k)]) - v) <= 1e-3 * gc.BOUNDS["poses_pose_only"]


def test_fixture_cases_are_what_they_claim():
    z = _fix()
    c = gc.from_fixture(z, "C")
    assert c["it"].tolist()[0] == 10 and c["it"][1] > 0 and int(c["write_back"]) == 1
    assert 0 < int((c["edge_inlier"] == 0).sum()) < len(c["edge_inlier"])
    assert int(c["trials"].max()) > 1, "no LM trial was ever rejected"
    for name in ("P0", "Pconv"):   # the auxiliary flag stopped round 1 and round 2 did nothing
        p = gc.from_fixture(z, name)
        assert p["stop"].tolist() == [1, 1] and p["it"][0] >= 1 and p["it"][1] == 0
        assert p["ret"].tolist() == [int(p["it"][0]), 0]
    assert int(gc.from_fixture(z, "P0")["outlier"].sum()) > 0
    from tests.test_global_ba import BANDED_CASES, _band_of
    kw = dict(gc.GBAND_KW)
    assert {k: kw[k] for k in BANDED_CASES["K33"][0]} == BANDED_CASES["K33"][0]
    T, band = _band_of(gc.problem("Gband")[0])
    assert band < T and (T, band) == BANDED_CASES["K33"][1:]
    assert all(v[1] >= T for v in BANDED_CASES.values()), "K33 is no longer the smallest"


def test_structure_case_counts():
    """What g2o's own containers report for the corner cases: a point seen only by fixed poses
    is active (its edges are not allVerticesFixed), a free pose whose edges are all at level 1
    is not, and with every edge disabled optimize() returns -1 and moves nothing."""
    z = _fix()
    pr, lvl = gc.problem("S")
    s = gc.from_fixture(z, "S")
    ep, eq = pr["edge_pose"][lvl == 0], pr["edge_point"][lvl == 0]
    free = np.unique(ep[pr["pose_fixed"][ep] == 0])
    assert 4 not in ep and pr["pose_fixed"][4] == 0
    assert s["active"].tolist() == [[int((lvl == 0).sum()), len(free), len(np.unique(eq))]]
    assert len(np.unique(eq)) == len(pr["points"]) and s["ret"].tolist() == [int(s["it"][0])]
    assert np.array_equal(s["poses"][4], pr["poses"][4])
    assert not np.array_equal(s["points"][0], pr["points"][0])   # moved, though only fixed poses see it
    off = gc.from_fixture(z, "Soff")
    assert off["ret"].tolist() == [-1] and off["active"].tolist() == [[0, 0, 0]]
    assert np.array_equal(off["poses"], pr["poses"]) and np.array_equal(off["points"], pr["points"])


def test_lperm_against_l():
    """The same problem under another vertex-id order (another Hessian order inside g2o)."""
    z = _fix()
    gc.check("L", gc.from_fixture(z, "Lperm"), gc.from_fixture(z, "L"), scale=gc.MARGIN, label="Lperm vs")
    assert np.array_equal(z["Lperm/trials"], z["L/trials"])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_measured_differences_leave_room(name):
    z = _fix()
    keys = [k for k in z.files if k.startswith("measured_%s_" % name)]
    assert keys
    for k in keys:
        f = k.rsplit("_", 1)[1]
        b = gc.BOUNDS["poses_pose_only" if f == "poses" and name in gc.POSE_ONLY else f]
        if f == "points" and name in gc.POSE_ONLY:
            b = 0.0
        assert float(z[k]) * gc.MARGIN <= b, (k, float(z[k]), b)


@pytest.mark.parametrize("name", list(gc.LIN_CASES))
def test_linear_solver_record(name):
    """LinearSolverEigen's recorded answer against numpy, and its bool against the natural-order
    LDL^T's zero pivot (ldlt.hpp: "an exact zero pivot fails the solve")."""
    z = _fix()
    S, b = gc.lin_system(*gc.LIN_CASES[name])
    ok = bool(z["lin/%s/ok" % name])
    assert ok == (gc.LIN_CASES[name][1] is None)
    assert ok == (not _no_pivot_ldlt_has_zero_pivot(S))
    if ok:
        ref = np.linalg.solve(S, b)
        rel = np.abs(z["lin/%s/x" % name] - ref).max() / np.abs(ref).max()
        print("lin", name, "g2o against numpy rel %.3g" % rel)
        assert rel <= LDLT_REL / gc.MARGIN


def test_linear_solver_order_dependence_is_recorded():
    """A zero diagonal block that stays coupled: SimplicialLDLT's answer follows its
    fill-reducing order, not the natural one (n132mid fails there, succeeds in natural order)."""
    z = _fix()
    got = {k: bool(z["lin_order/%s/ok" % k]) for k in gc.LIN_ORDER_CASES}
    assert got == {"n66head": False, "n66mid": True, "n132mid": False}
    nat = {k: not _no_pivot_ldlt_has_zero_pivot(gc.lin_coupled_zero(*v)[0])
           for k, v in gc.LIN_ORDER_CASES.items()}
    assert nat == {"n66head": False, "n66mid": True, "n132mid": True}


@pytest.mark.skipif(not rg.available(), reason="oracle/_ref/libg2o_ref.so is not built")
def test_fixture_regenerates_from_reference_g2o(tmp_path):
    """Where the reference checkout was there to build from, the generator re-derives the fixture
    from the reference's compiled g2o: discrete fields equal, continuous ones rel 1e-12."""
    out = tmp_path / "g.npz"
    gen = os.path.join(GOLDEN, "gen_g2o_optimize_ref.py")
    subprocess.check_call([sys.executable, gen, "--out", str(out)], timeout=600,
                          stdout=subprocess.DEVNULL)
    q, z = np.load(out), _fix()
    assert sorted(q.files) == sorted(z.files)
    bitwise, worst = True, 0.0
    for k in q.files:
        a, b = q[k], z[k]
        if k.startswith("measured_"):
            assert abs(float(a) - float(b)) <= 1e-3 * gc.BOUNDS["poses_pose_only"], k
        elif a.dtype.kind in "fc":
            assert a.shape == b.shape, k
            if a.size:
                d = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
                worst = max(worst, d)
                assert d <= 1e-12, (k, d)
        else:
            assert np.array_equal(a, b), k
        bitwise &= a.tobytes() == b.tobytes()
    print("regenerated from libg2o_ref.so: %d keys, bitwise %s, worst rel %.3g" % (
        len(q.files), bitwise, worst))


# ------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gc.CASES))
def test_gpu_entry_points_match_g2o(gpu, name):
    """mcs_ba_optimize (L, Lperm, S, Soff), mcs_local_ba_ex (C), mcs_global_ba (G, Gpose, Gband;
    default = banded LDL^T mode) and mcs_pose_optimization (P0, Pconv) against the record."""
    from mcs_amd import ba
    gc.check(name, gc.run(name, ba.Solver()), gc.from_fixture(_fix(), name), label="gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["G", "Gpose", "Gband"])
def test_gpu_global_ba_dense_mode_matches_g2o(gpu, name):
    from mcs_amd import ba
    S = ba.Solver()
    S.set_ldlt_mode(ba.LDLT_DENSE)
    gc.check(name, gc.run(name, S), gc.from_fixture(_fix(), name), label="gpu dense")


@pytest.mark.gpu
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", list(gc.LIN_CASES))
def test_gpu_dense_ldlt_matches_linear_solver_eigen(gpu, name, path):
    """mcs_dense_ldlt_solve on what BA uses (path 0: one fused tile up to n = 64, the pipelined
    tiles above) and on the pad + per-step panels (path 1) against LinearSolverEigen's recorded
    solution; the zero-pivot flag is set exactly where solve() returned false."""
    from mcs_amd import ba
    z = _fix()
    S, b = gc.lin_system(*gc.LIN_CASES[name])
    x, zp = ba.dense_ldlt_solve(S, b, path=path)
    ok = bool(z["lin/%s/ok" % name])
    assert (zp != 0) == (not ok)
    if ok:
        ref = z["lin/%s/x" % name]
        rel = np.abs(x - ref).max() / np.abs(ref).max()
        print("gpu lin", name, "path", path, "against LinearSolverEigen rel %.3g" % rel)
        assert rel <= LDLT_REL


# --------------------------------------------------- the reference text driving the reference g2o
# localba_g2o_ref.npz / globalba_g2o_ref.npz: gen_localba_ref.py / gen_globalba_ref.py --g2o, i.e.
# the translated LocalBundleAdjustment / BundleAdjustment / PoseOptimization text with every
# optimize() run by libg2o_ref.so under the vertex ids the text assigned.  They hold what a run
# produced; the inputs are those of localba_ref.npz / globalba_ref.npz.
TEXT = {"localba": ("localba_ref.npz", "localba_g2o_ref.npz", "gen_localba_ref.py"),
        "globalba": ("globalba_ref.npz", "globalba_g2o_ref.npz", "gen_globalba_ref.py")}
# float keys an optimisation moves -> bound (abs for poses, of the row's scale for points)
TEXT_BOUNDS = {"est_poses": gc.BOUNDS["poses"], "pose_write": gc.BOUNDS["poses"],
               "pose_out": gc.BOUNDS["poses_pose_only"], "est_points": gc.BOUNDS["points"],
               "point_write": gc.BOUNDS["points"]}


class _Merged(dict):
    files = property(lambda self: list(self))


def _text(which):
    if which not in _Z:
        base = dict(np.load(os.path.join(GOLDEN, TEXT[which][0]), allow_pickle=False))
        g2o = dict(np.load(os.path.join(GOLDEN, TEXT[which][1]), allow_pickle=False))
        _Z[which] = (base, g2o, _Merged({**base, **g2o}))
    return _Z[which]


def _text_names(which, first):
    g2o = np.load(os.path.join(GOLDEN, TEXT[which][1]), allow_pickle=False)
    return sorted({k.split("_")[0] for k in g2o.files if k[0] in first and k[1].isdigit()})


def _text_diff(a, b, key):
    """Largest difference of a moved float key, in the terms of its bound."""
    kind = key.split("_", 1)[1]
    if kind in ("pose_write", "point_write"):   # leading column: the keyframe / point written
        assert np.array_equal(a[:, 0], b[:, 0]), key
        a, b = a[:, 1:], b[:, 1:]
    if not a.size:
        return 0.0
    d = np.abs(a - b)
    if kind in ("est_points", "point_write"):
        d = d.max(axis=1) / np.maximum(1.0, np.linalg.norm(b.reshape(len(b), -1), axis=1))
    return float(d.max())


@pytest.mark.parametrize("which", list(TEXT))
def test_text_over_g2o_against_text_over_oracle(which):
    """The same translated text with the oracle's rounds and with the reference's own g2o:
    every discrete record equal (vertices, edges and their final levels, each optimize()'s
    iterations and flags, erased observations, bad points, the entries written back, outliers,
    return values), the written estimates 10x inside the bounds."""
    base, g2o, _ = _text(which)
    assert set(g2o) <= set(base) and len(g2o) > 100
    worst = {}
    for k, v in g2o.items():
        kind = k.split("_", 1)[1] if "_" in k else k
        if kind in TEXT_BOUNDS:
            assert v.shape == base[k].shape, k
            d = _text_diff(v, base[k], k)
            worst[kind] = max(worst.get(kind, 0.0), d)
            assert d * gc.MARGIN <= TEXT_BOUNDS[kind], (k, d)
        else:
            assert np.array_equal(v, base[k]), k
    print(which, "text over g2o against text over the oracle:",
          " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert len(worst) >= 3


@pytest.mark.skipif(not (rg.available() and os.path.isdir("/root/reference")),
                    reason="needs oracle/_ref/libg2o_ref.so and the reference checkout")
@pytest.mark.parametrize("which", list(TEXT))
def test_text_over_g2o_regenerates(which, tmp_path):
    out = tmp_path / "t.npz"
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, TEXT[which][2]), "--g2o", "--out", str(out)],
                          timeout=900, stdout=subprocess.DEVNULL)
    q, z = np.load(out), _text(which)[1]
    assert sorted(q.files) == sorted(z)
    bitwise = True
    for k in q.files:
        kind = k.split("_", 1)[1] if "_" in k else k
        if kind in TEXT_BOUNDS and q[k].size:
            assert np.abs(q[k] - z[k]).max() <= 1e-12 * max(1.0, np.abs(z[k]).max()), k
        else:
            assert np.array_equal(q[k], z[k]), k
        bitwise &= q[k].tobytes() == z[k].tobytes()
    print("%s regenerated through libg2o_ref.so: %d keys, bitwise %s" % (TEXT[which][1], len(q.files), bitwise))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _text_names("localba", "s"))
def test_gpu_local_ba_matches_text_over_g2o(gpu, name, monkeypatch):
    """tests/test_localba_ref.py's GPU comparison, held against the g2o-driven record."""
    from tests import test_localba_ref as TL
    monkeypatch.setitem(TL._Z, "z", _text("localba")[2])
    TL.test_gpu_local_ba_matches_reference_text(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _text_names("globalba", "g"))
def test_gpu_global_ba_matches_text_over_g2o(gpu, name, monkeypatch):
    from tests import test_globalba_ref as TG
    monkeypatch.setattr(TG, "_fix", lambda: _text("globalba")[2])
    TG.test_gpu_global_ba_matches_reference_text(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _text_names("globalba", "p"))
def test_gpu_pose_optimization_matches_text_over_g2o(gpu, name, monkeypatch):
    from tests import test_globalba_ref as TG
    monkeypatch.setattr(TG, "_fix", lambda: _text("globalba")[2])
    TG.test_gpu_pose_optimization_matches_reference_text(gpu, name)
    z = _text("globalba")[2]      # the pose-only bound of tests/test_pose_opt.py on top
    g = TG._po_select(z, name + "_")
    from mcs_amd import ba
    r = ba.Solver().pose_optimization(TG._po_problem(z, name + "_", g))
    d = np.abs(r["pose"] - z[name + "_pose_out"]).max()
    print("gpu text-over-g2o", name, "pose %.3g" % d)
    assert d < gc.BOUNDS["poses_pose_only"]
