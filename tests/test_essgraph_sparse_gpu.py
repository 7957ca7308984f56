"""OptimizeEssentialGraph through a plan (include/mcs_essgraph.h: mcs_essgraph_plan_create,
mcs_optimize_essential_graph_planned_device; csrc/essential_graph_sparse.hpp), the block-sparse
LDL^T: every case of tests/essgraph_cases.py against tests/golden/essgraph_ref.npz by the fixture's
own rule (essgraph_cases.compare, unchanged), the sparse solve against the dense one on the device,
identical bits from run to run and from a permuted edge list, a second call that allocates nothing,
the status word for what a plan refuses, and K_cov1000: a map above the dense entries' 878
keyframes against tests/golden/essgraph_sparse_ref.npz (the reference's own g2o,
tests/golden/gen_essgraph_sparse_ref.py)."""
import os

import numpy as np
import pytest

from tests import essgraph_cases as ec
from tests import essgraph_sparse_cases as sc
from tests import test_essgraph_gpu as tg

pytestmark = pytest.mark.gpu
_SPARSE = {}


def _es():
    from mcs_amd import essential_graph
    return essential_graph


def sparse_fixture():
    if "fix" not in _SPARSE:
        _SPARSE["fix"] = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                              "essgraph_sparse_ref.npz"))
    return _SPARSE["fix"]


def k_case():
    if "K" not in _SPARSE:
        _SPARSE["K"] = sc.make_sparse_case("K_cov1000")
    return _SPARSE["K"]


class Planned:
    """A case on the device (test_essgraph_gpu.Device) and a plan for its edge list."""

    def __init__(self, case, edges=None, leaf=None, plan=None, max_points=None):
        self.dev = tg.Device(case, edges, band=0)
        self.plan = plan if plan is not None else _es().Plan(
            case["N"], case["loop"], self.dev.edges_np, max_points=case["P"] if max_points is None else max_points,
            leaf_size=leaf)

    def run(self, out=None, edges=None, ref=None):
        import torch
        d = self.dev
        pos = d.pos.clone()
        ts = _es().optimize_planned_device(self.plan, d.Scw, d.Snc, d.edges if edges is None else edges, pos,
                                           d.ref if ref is None else ref, d.bad, d.opts, out=out, loop=d.case["loop"])
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in ts.items()}
        r["points"] = pos.cpu().numpy()
        return r


LEAVES = [(n, None) for n in ec.CASES] + [(n, leaf) for leaf in (4, 16) for n in ("C_cov40", "H_cov130")]


@pytest.mark.parametrize("name,leaf", LEAVES)
def test_planned_entry_equals_the_reference_g2o(gpu, name, leaf):
    case = tg.get_case(name)
    p = Planned(case, leaf=leaf)
    print(name, leaf, p.plan.info)
    r = p.run()
    assert r["status"][0] == 0
    ec.compare(tg.fixture(), name, tg.as_result(r))
    if "opts" in ec.CASES[name]:                         # the one-trial cases: the host replica's tighter tier
        ec.compare(tg.fixture(), "host_" + name, tg.as_result(r))
    n_it = r["iterations"][0]
    assert (r["trials"][n_it:] == 0).all() and (r["chi2"][n_it:] == 0).all() and r["lambda"][0] > 0
    if name == "C_cov40":                                # rejects and re-damping on one factor pattern
        assert r["trials"][:n_it].tolist() == [1, 4, 4, 1, 4, 1]
    if name == "E_consistent":                           # rho = 0: one rejected trial, nothing moves, to the bit
        assert r["trials"][0] == 1 and np.array_equal(r["sim3"], case["Scw"])
        keep = case["bad"] == 0
        assert np.array_equal(r["points"][keep], case["pos"][keep])
    bad = case["bad"] != 0
    assert np.array_equal(r["points"][bad], case["pos"][bad])


@pytest.mark.parametrize("name", ["G_mid100", "H_cov130"])
def test_sparse_solve_equals_the_dense_one_on_the_device(gpu, name):
    """The rule of test_banded_solve_equals_the_dense_one: the same systems, another elimination
    order; 1e-9 of the field's scale bounds what that can leave."""
    case = tg.get_case(name)
    sparse, dense = Planned(case).run(), tg.Device(case).run()
    assert sparse["status"][0] == 0 and dense["status"][0] == 0 and dense["iterations"][0] == 1
    assert np.array_equal(sparse["trials"], dense["trials"]) and sparse["iterations"][0] == dense["iterations"][0]
    for k in ("sim3", "pose", "points", "chi2", "edge_chi2"):
        d = np.abs(sparse[k] - dense[k]).max()
        print(name, "sparse - dense", k, d)
        assert d <= 1e-9 * max(1.0, np.abs(dense[k]).max()), k


def test_identical_bits_from_two_runs_a_permuted_list_and_no_allocation(gpu):
    import torch
    es = _es()
    case = tg.get_case("I_dense300")
    p = Planned(case)
    want = p.run()
    assert want["status"][0] == 0 and want["iterations"][0] == 1
    tg.same_bits(want, p.run())
    perm = np.random.default_rng(5).permutation(len(p.dev.edges_np))
    got = p.run(edges=tg.up(p.dev.edges_np[perm], np.int32))
    tg.same_bits(want, got, skip=("edge_chi2",))
    assert want["edge_chi2"][perm].tobytes() == got["edge_chi2"].tobytes()
    again = Planned(case, edges=p.dev.edges_np[perm])                # planned from the permuted list: the same plan
    assert again.plan.info["digest"] == p.plan.info["digest"]
    tg.same_bits(want, again.run(edges=p.dev.edges))
    again.plan.close()
    d = p.dev
    out = es.new_out(case["N"], len(d.edges_np))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    pos = d.pos.clone()
    free1 = torch.cuda.mem_get_info()[0]
    es.optimize_planned_device(p.plan, d.Scw, d.Snc, d.edges, pos, d.ref, d.bad, d.opts, out=out)
    free2 = torch.cuda.mem_get_info()[0]               # before any synchronisation: nothing was allocated
    torch.cuda.synchronize()
    assert free2 == free1 <= free0
    assert out[1]["sim3"].cpu().numpy().tobytes() == want["sim3"].tobytes()
    p.plan.close()


def untouched(r, case, what):
    assert r["status"][0] == -1, what
    assert np.array_equal(r["points"], case["pos"]), what
    for k in ("sim3", "rot", "pose", "chi2", "edge_chi2", "iterations", "trials", "lambda"):
        assert (r[k] == 7).all(), (what, k)


def sevens(N, E):
    out = _es().new_out(N, E)
    for t in out[1].values():
        t.fill_(7)
    return out


def test_a_plan_refuses_another_map(gpu):
    """A plan made for J_n300 is given A_ring6: MCS_ERR_ARG in the status word, nothing else written."""
    big, small = tg.get_case("J_n300"), tg.get_case("A_ring6")
    plan = Planned(big).plan
    p = Planned(small, plan=plan)
    untouched(p.run(out=sevens(small["N"], len(p.dev.edges_np))), small, "another map")
    import mcs_amd
    few = _es().Plan(small["N"], small["loop"], p.dev.edges_np, max_points=0)      # counts above the plan's
    with pytest.raises(mcs_amd.McsError) as e:
        Planned(small, plan=few).run()
    assert e.value.code == mcs_amd.MCS_ERR_ARG


def test_what_the_plan_does_not_hold_is_reported_and_nothing_is_touched(gpu):
    case = tg.get_case("G_mid100")
    p = Planned(case)
    held = {(min(a, b), max(a, b)) for a, b, _ in p.dev.edges_np.tolist()}
    assert (3, 90) not in held and (40, 41) in held
    for what in ("pair", "fill", "ref", "v0"):
        edges, ref = p.dev.edges_np.copy(), ec.point_refs(case).copy()
        if what == "pair":
            edges[5, :2] = (3, 90)                       # two free keyframes far apart: no block at all
        elif what == "fill":
            edges[5, :2] = (40, 47)                      # not a pair of the list (neighbours reach 6), fill or not
            assert (40, 47) not in held
        elif what == "ref":
            ref[int(np.flatnonzero(case["bad"] == 0)[0])] = case["N"] + 3
        else:
            edges[3, 0] = case["N"]
        r = p.run(out=sevens(case["N"], len(edges)), edges=tg.up(edges, np.int32), ref=tg.up(ref, np.int32))
        untouched(r, case, what)
    ok = p.run()                                         # the plan is intact afterwards
    assert ok["status"][0] == 0
    ec.compare(tg.fixture(), "G_mid100", tg.as_result(ok))


def test_a_map_beyond_the_dense_cap_equals_the_reference_g2o(gpu):
    """K_cov1000, one trial: 1000 keyframes, 13 592 edges.  The dense entries refuse it as before;
    the planned entry and the host form over a plan hold the fixture's rule."""
    import mcs_amd
    es = _es()
    case, fix = k_case(), sparse_fixture()
    assert ec.digest(case) == str(fix["K_cov1000_sha256"]), "the seeded inputs are not those of the fixture"
    edges, counts = es.select_edges(case["ids"], case["parent"], case["has_corr"], (case["loop_ptr"], case["loop_idx"]),
                                    (case["cov_ptr"], case["cov_idx"], case["cov_w"]),
                                    (case["lc_ptr"], case["lc_idx"], case["lc_w"]), case["cur"], case["loop"],
                                    case["min_weight"])
    assert np.array_equal(edges, fix["K_cov1000_edges"]) and np.array_equal(counts, fix["K_cov1000_counts"])
    assert not es.supported(1000)
    with pytest.raises(mcs_amd.McsError) as e:
        es.optimize(case["Scw"], case["Snc"], case["loop"], edges, case["pos"], ec.point_refs(case), case["bad"],
                    options=case["opts"])
    assert e.value.code == mcs_amd.MCS_ERR_UNSUPPORTED
    p = Planned(case, edges=edges)
    print(p.plan.info)
    r = p.run()
    assert r["status"][0] == 0
    ec.compare(fix, "K_cov1000", tg.as_result(r))
    if "host_K_cov1000_sim3" in fix:
        ec.compare(fix, "host_K_cov1000", tg.as_result(r))
    host = es.optimize_sparse(case["Scw"], case["Snc"], case["loop"], edges, case["pos"], ec.point_refs(case),
                              case["bad"], options=case["opts"])
    for k in r:
        assert host[k].tobytes() == r[k].tobytes(), k
    p.plan.close()


def _demo(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "essgraph_sparse_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(root, "tests", "cpp", "essgraph_sparse_demo.cpp"),
                           "-I", os.path.join(root, "include"), "-L", lib, "-lmcs_amd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def _run_demo(exe, case, solver, tmp_path):
    import subprocess
    path = str(tmp_path / (case["name"] + ".txt"))
    ec.write_case_file(case, path)
    out = subprocess.run([exe, path, solver], capture_output=True, text=True, timeout=60)
    rows = [ln.split() for ln in out.stdout.splitlines()]
    head = {r[0]: r[1] for r in rows if r and r[0] in ("sparse", "iterations", "edges", "error")}
    pose = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "pose"])
    pts = [r for r in rows if r[0] == "points"]
    return out.returncode, head, pose, (np.array([float(x) for x in pts[0][1:]]).reshape(-1, 3) if pts else None)


def test_adapter_solver_argument(gpu, tmp_path):
    """mcs::OptimizeEssentialGraph of host/mcs_multicol.hpp: Auto is the dense solver wherever it
    takes the map and the plan above the cap; Sparse and Dense are what they say."""
    exe = _demo(tmp_path)
    small, fix = tg.get_case("C_cov40"), tg.fixture()
    want = {}
    for solver, sparse in (("auto", "0"), ("dense", "0"), ("sparse", "1")):
        rc, head, pose, pts = _run_demo(exe, small, solver, tmp_path)
        assert rc == 0 and head["sparse"] == sparse, (solver, head)
        assert int(head["iterations"]) == int(fix["C_cov40_iterations"]) and int(head["edges"]) == len(fix["C_cov40_edges"])
        assert np.abs(pose - fix["C_cov40_pose"]).max() <= ec.tolerance(fix, "C_cov40", "pose")
        assert np.abs(pts - fix["C_cov40_points"]).max() <= ec.tolerance(fix, "C_cov40", "points")
        want[solver] = (pose, pts)
    assert want["auto"][0].tobytes() == want["dense"][0].tobytes() and want["auto"][1].tobytes() == want["dense"][1].tobytes()
    big, sfix = k_case(), sparse_fixture()
    rc, head, pose, pts = _run_demo(exe, big, "auto", tmp_path)
    assert rc == 0 and head["sparse"] == "1" and int(head["iterations"]) == 1, head
    assert np.abs(pose - sfix["K_cov1000_pose"]).max() <= ec.tolerance(sfix, "K_cov1000", "pose")
    assert np.abs(pts - sfix["K_cov1000_points"]).max() <= ec.tolerance(sfix, "K_cov1000", "points")
    rc, head, _, _ = _run_demo(exe, big, "dense", tmp_path)                 # the dense entry's limit stays
    assert rc == 1 and "error" in head
