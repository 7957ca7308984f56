"""OptimizeEssentialGraph without a GPU: Sim3::log / Sim3(update) of csrc/essential_graph_math.hpp
against the reference's own (tests/golden/essgraph_ref.npz, written by gen_essgraph_ref.py through
tests/cpp/essgraph_g2o_driver.cpp), the edge selection against the edge lists the text's loops
produce, hand-made selection cases, and the argument errors of the entries, which all come before
any device use."""
import os
import subprocess

import numpy as np
import pytest

from tests import essgraph_cases as ec
from tests import ref_g2o_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "essgraph_ref.npz")
NEW_SYMBOLS = ("mcs_essgraph_select_edges", "mcs_essgraph_default_options", "mcs_essgraph_tile_band",
               "mcs_essgraph_supported", "mcs_essgraph_workspace_create", "mcs_essgraph_workspace_destroy",
               "mcs_essgraph_resolve_point_refs_device", "mcs_optimize_essential_graph_device",
               "mcs_optimize_essential_graph")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("essgraph") / "essgraph_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "essgraph_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def _es():
    from mcs_amd import essential_graph
    return essential_graph


def select(case, **kw):
    c = dict(case, **kw)
    return _es().select_edges(c["ids"], c["parent"], c["has_corr"], (c["loop_ptr"], c["loop_idx"]),
                              (c["cov_ptr"], c["cov_idx"], c["cov_w"]), (c["lc_ptr"], c["lc_idx"], c["lc_w"]),
                              c["cur"], c["loop"], c["min_weight"])


def _W_cond(row):
    """cond(W) of Sim3::log's last solve in the theta -> 0, sigma != 0 branch, W = A [w]x + B [w]x^2 + C I."""
    s, (w, x, y, z) = row[0], row[1:5]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    sg = np.log(s)
    om = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    A, B, C = ((sg - 1) * s + 1) / sg ** 2, ((0.5 * sg * sg - sg + 1) * s) / sg ** 3, (s - 1) / sg
    return np.linalg.cond(A * Om + B * Om @ Om + C * np.eye(3))


def test_sim3_log_and_exp_equal_the_reference_on_both_sides_of_each_threshold(host, fix, tmp_path):
    logs, exps = ec.log_exp_inputs()
    import hashlib
    assert hashlib.sha256(logs.tobytes() + exps.tobytes()).hexdigest() == str(fix["list_sha256"])
    path = str(tmp_path / "list.txt")
    ec.write_list_file(path, logs, exps)
    lo, ex = ec.parse_list(subprocess.check_output([host, "list", path], text=True))
    want_lo, want_ex = fix["list_log"], fix["list_exp"]
    branches = set()
    worst = 0.0
    for i, row in enumerate(logs):
        sg, th = np.log(row[0]), 2 * np.arccos(min(1.0, abs(row[1])))
        small_s, small_t = abs(sg) < 1e-5, 1 - np.cos(th) < 1e-5
        branches.add((small_s, small_t))
        scale = max(1.0, np.abs(want_lo[i]).max())
        # 1e-12 relative to the row; in the 1 / sigma^3 branch upsilon is the solution of a 3 x 3
        # system whose condition number reaches 1e10 there (B theta^2 against C), and two correct
        # evaluations of it differ by up to cond(W) ulp: the bound is 16 cond(W) 2^-52
        tol = 1e-12 * scale
        if not small_s and small_t:
            tol = max(tol, 16 * _W_cond(row) * 2.0 ** -52 * scale)
        d = np.abs(lo[i] - want_lo[i]).max()
        worst = max(worst, d / tol)
        assert d <= tol, (i, row, lo[i], want_lo[i], tol)
    assert len(branches) == 4, "the list must reach all four branches of log"
    for i in range(len(exps)):
        scale = max(1.0, np.abs(want_ex[i]).max())
        assert np.abs(ex[i] - want_ex[i]).max() <= 1e-12 * scale, (i, exps[i], ex[i], want_ex[i])
    print("worst log difference / tolerance", worst)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_select_edges_equals_the_loops_of_the_text(built, fix, name):
    case = ec.make_case(name)
    assert ec.digest(case) == str(fix[name + "_sha256"]), "the seeded inputs are not those of the fixture"
    edges, counts = select(case)
    assert np.array_equal(edges, fix[name + "_edges"])
    assert np.array_equal(counts, fix[name + "_counts"])


def test_host_program_selects_the_same_edges(host, fix, tmp_path):
    case = ec.make_case("C_cov40")
    path = str(tmp_path / "c.txt")
    ec.write_case_file(case, path)
    r = ec.parse_results(subprocess.check_output([host, "edges", path], text=True))
    assert np.array_equal(r["edges"], fix["C_cov40_edges"]) and np.array_equal(r["counts"], fix["C_cov40_counts"])


def test_one_trial_cases_enter_the_paths_they_are_named_for(built, fix):
    ONE_TRIAL = [n for n in ec.CASES if "opts" in ec.CASES[n]]
    tiles = lambda n: (7 * (ec.CASES[n]["N"] - 1) + 63) // 64  # noqa: E731
    E = {n: len(fix[n + "_edges"]) for n in ONE_TRIAL}
    assert ONE_TRIAL == ["G_mid100", "H_cov130", "J_n300", "I_dense300"]
    assert [tiles(n) for n in ONE_TRIAL] == [11, 15, 33, 33]                    # every earlier case has at most 5
    assert all(256 < E[n] for n in ONE_TRIAL) and E["I_dense300"] > 16384 >= E["J_n300"]
    assert [min(64, (E[n] + 255) // 256) for n in ONE_TRIAL] == [3, 3, 35, 64]  # chi2 partials
    loop = ec.CASES["G_mid100"]["loop"]
    assert 0 < 7 * loop // 64 < tiles("G_mid100") - 1                           # the fixed keyframe in a middle tile
    assert ec.CASES["J_n300"]["N"] > 256 and ec.CASES["J_n300"]["P"] > 256
    assert fix["H_cov130_counts"].tolist()[:3] == [4, 129, 1]                   # loop connections, tree, earlier loop
    es = _es()
    band = {n: es.tile_band(ec.CASES[n]["N"], ec.CASES[n].get("loop", 0), fix[n + "_edges"]) for n in ONE_TRIAL}
    assert band == {"G_mid100": 2, "H_cov130": 15, "J_n300": 5, "I_dense300": 8}, band      # H: every tile filled
    for n in ONE_TRIAL:
        assert fix[n + "_trials"].tolist() == [1] and fix[n + "_chi2"][0] < fix[n + "_chi2_initial"]
        assert fix["host_" + n + "_trials"].tolist() == [1]
        for f in ec.REALS:                      # the second tier is the tighter one
            assert fix["measured_host_%s_%s" % (n, f)] < fix["measured_%s_%s" % (n, f)], (n, f)


def _tiny(cov, lc, loops=None, parent=None, has_corr=None, cur=3, loop=0, ids=(10, 20, 30, 40)):
    N = len(ids)
    cp, cf = ec._csr(cov)
    lp, lf = ec._csr(lc)
    op, of = ec._csr(loops or [[] for _ in range(N)])
    return dict(ids=np.array(ids, np.int64), parent=np.array(parent if parent is not None else [-1] * N, np.int32),
                has_corr=np.array(has_corr if has_corr is not None else [0] * N, np.uint8),
                loop_ptr=op, loop_idx=np.array(of, np.int32),
                cov_ptr=cp, cov_idx=np.array([c for c, _ in cf], np.int32), cov_w=np.array([w for _, w in cf], np.int32),
                lc_ptr=lp, lc_idx=np.array([c for c, _ in lf], np.int32), lc_w=np.array([w for _, w in lf], np.int32),
                cur=cur, loop=loop, min_weight=100)


def test_select_edges_weights_99_100_101(built):
    e, c = select(_tiny(cov=[[], [(0, 99)], [(0, 100)], [(0, 101)]], lc=[[], [], [], []]))
    assert e.tolist() == [[2, 0, 0], [3, 0, 0]] and c.tolist() == [0, 0, 0, 2]
    e, c = select(_tiny(cov=[[(1, 150)], [], [], []], lc=[[], [], [], []]))      # only id_n < id_i adds it
    assert len(e) == 0
    e, c = select(_tiny(cov=[[]] * 4, lc=[[], [(2, 99)], [(0, 100)], [(1, 101), (2, 5)]]))
    assert e.tolist() == [[2, 0, 0], [3, 1, 0]] and c.tolist() == [2, 0, 0, 0]


def test_select_edges_current_loop_pair_is_exempt_from_the_weight(built):
    e, c = select(_tiny(cov=[[]] * 4, lc=[[], [], [], [(0, 1)]]))
    assert e.tolist() == [[3, 0, 0]]
    e, c = select(_tiny(cov=[[]] * 4, lc=[[(3, 1)], [], [(0, 1)], []]))           # (loop, current) and others are not
    assert len(e) == 0


def test_select_edges_keeps_duplicate_pairs_and_marks_the_table(built):
    m = _tiny(cov=[[], [(0, 150)], [], [(0, 120), (2, 100)]], lc=[[], [], [], [(0, 1)]], loops=[[3], [], [], [0]],
              parent=[-1, 0, 1, 2], has_corr=[0, 0, 0, 1])
    e, c = select(m)
    # loop connection; then per keyframe: parent, earlier loop edges, covisibles -- insertedEdges is never consulted
    assert e.tolist() == [[3, 0, 0], [1, 0, 0], [1, 0, 0], [2, 1, 0], [3, 2, 1], [3, 0, 1], [3, 0, 1], [3, 2, 1]]
    assert c.tolist() == [1, 3, 1, 3]
    es = _es()
    assert es.tile_band(4, 0, e) == 1 and es.tile_band(40, 0, [[39, 1, 0]]) == 5 and es.tile_band(40, 0, [[39, 0, 0]]) == 2


def test_select_edges_argument_errors(built):
    import mcs_amd
    good = _tiny(cov=[[]] * 4, lc=[[]] * 4)
    for kw in (dict(cur=4), dict(loop=-1), dict(ids=np.array([10, 20, 20, 40], np.int64)),
               dict(parent=np.array([-1, 0, 1, 7], np.int32)), dict(cov_idx=np.array([9], np.int32),
                                                                    cov_w=np.array([100], np.int32),
                                                                    cov_ptr=np.array([0, 1, 1, 1, 1], np.int32))):
        with pytest.raises(mcs_amd.McsError) as err:
            select(good, **kw)
        assert err.value.code == mcs_amd.MCS_ERR_ARG, kw


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES and hasattr(mcs_amd.lib(), s), s


def test_entry_argument_errors_come_before_any_device_use(built):
    import mcs_amd
    es = _es()
    case = ec.make_case("A_ring6")
    edges = np.load(FIX)["A_ring6_edges"]
    args = (case["Scw"], case["Snc"], case["loop"], edges, case["pos"], ec.point_refs(case), case["bad"])
    for a, kw in ((args, dict(options=dict(iterations=65))), (args, dict(options=dict(iterations=-1))),
                  (args, dict(options=dict(max_trials=0))), (args, dict(options=dict(max_trials=65))),
                  (args[:2] + (6,) + args[3:], {}), (args[:2] + (-1,) + args[3:], {}),
                  (args[:3] + (np.array([[1, 1, 0]], np.int32),) + args[4:], {})):
        with pytest.raises(mcs_amd.McsError) as e:
            es.optimize(*a, **kw)
        assert e.value.code == mcs_amd.MCS_ERR_ARG, kw
    # above the solver's limit: size arithmetic alone, nothing is allocated
    big = np.tile(case["Scw"][:1], (2000, 1))
    with pytest.raises(mcs_amd.McsError) as e:
        es.optimize(big, big, 0, np.array([[1, 0, 0]], np.int32))
    assert e.value.code == mcs_amd.MCS_ERR_UNSUPPORTED
    assert es.supported(878) and not es.supported(879) and es.supported(10)
    # the device entry checks the same before it touches its pointers
    o, out = es.default_options(iterations=99), es.EssGraphOut()
    status = np.zeros(1, np.int32)
    out.status = status.ctypes.data
    rc = mcs_amd.lib().mcs_optimize_essential_graph_device(None, 6, case["Scw"].ctypes.data, case["Snc"].ctypes.data, 0,
                                                           0, None, 0, None, None, None, ctypes_ref(o), ctypes_ref(out),
                                                           None)
    assert rc == mcs_amd.MCS_ERR_ARG
    if mcs_amd.device_count() < 1:
        with pytest.raises(mcs_amd.McsError) as e:
            es.optimize(*args)
        assert e.value.code == mcs_amd.MCS_ERR_NO_DEVICE


def ctypes_ref(x):
    import ctypes
    return ctypes.byref(x)


REF_G2O = os.path.join(os.environ.get("MCS_REFERENCE", "/root/reference"), "ThirdParty", "g2o", "g2o", "types", "sim3.h")


@pytest.mark.skipif(not (ref_g2o_bind.available() and os.path.exists(REF_G2O)),
                    reason="needs oracle/_ref/libg2o_ref.so and the reference checkout's g2o headers")
def test_fixture_regenerates_from_the_reference_g2o(fix, tmp_path):
    from tests.golden import gen_essgraph_ref as gen
    exe = gen.build_driver(str(tmp_path))
    case = ec.make_case("B_ring12")
    runs = gen.run_reference(exe, case, str(tmp_path))
    for f in ec.INTS + ec.REALS:
        assert np.array_equal(np.asarray(runs[0][f]), fix["B_ring12_" + f]), f
    spread = gen.check_and_measure("B_ring12", runs)
    for f in ec.REALS:
        assert spread[f] == float(fix["measured_B_ring12_" + f]), f
    # a one-trial case: the reference runs, the generator's conditions, and the host replica's keys
    name = "G_mid100"
    case = ec.make_case(name)
    runs = gen.run_reference(exe, case, str(tmp_path))
    for f in ec.INTS + ec.REALS:
        assert np.array_equal(np.asarray(runs[0][f]), fix["%s_%s" % (name, f)]), f
    spread = gen.check_and_measure(name, runs)
    for f in ec.REALS:
        assert spread[f] == float(fix["measured_%s_%s" % (name, f)]), f
    assert gen.one_trial(case) and gen.check_one_trial(name, case, runs, spread) >= 0.9
    hruns = gen.run_host(gen.build_host(str(tmp_path)), case, str(tmp_path))
    hspread = gen.spread_of(hruns)
    for f in ("iterations", "trials") + ec.REALS:
        assert np.array_equal(np.asarray(hruns[0][f]), fix["host_%s_%s" % (name, f)]), f
    for f in ec.REALS:
        assert hspread[f] == float(fix["measured_host_%s_%s" % (name, f)]), f
