"""tests/cpp/essgraph_sparse_host.cpp: the planner and the per-supernode arithmetic of the
block-sparse essential-graph solver (csrc/essential_graph_sparse_math.hpp, the functions the device
kernels run) on the CPU in the plan's launch order, against a dense LDL^T of the same seeded SPD
block matrix.  The bound c n 2^-52 cond is the program's own and is stated at its head; the
program computes the condition number.  Then a matrix with an exact zero pivot, and the same
program under ASan / UBSan, run stand-alone."""
import os
import subprocess

import pytest

from tests import essgraph_sparse_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ("A_ring6", "C_cov40", "G_mid100", "H_cov130", "J_n300")


def _build(path, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra,
                           os.path.join(ROOT, "tests", "cpp", "essgraph_sparse_host.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("essgraph_sparse_host") / "essgraph_sparse_host"))


def graph_file(name, tmp_path):
    edges, N, loop = sc.graph(name)
    path = str(tmp_path / (name + ".graph"))
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (N, loop, len(edges)))
        for r in edges:
            f.write("%d %d %d\n" % tuple(r))
    return path


@pytest.mark.parametrize("leaf", [0, 4, 16])
@pytest.mark.parametrize("name", GRAPHS)
def test_sparse_solve_equals_the_dense_one_within_the_stated_bound(host, tmp_path, name, leaf):
    r = subprocess.run([host, "solve", graph_file(name, tmp_path), str(leaf), "11"], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    last = dict(zip(r.stdout.splitlines()[-1].split()[::2], r.stdout.splitlines()[-1].split()[1::2]))
    assert float(last["residual"]) <= float(last["bound"]) and float(last["cond"]) > 1.0


@pytest.mark.parametrize("name", ["A_ring6", "H_cov130"])
def test_an_exact_zero_pivot_sets_the_flag(host, tmp_path, name):
    r = subprocess.run([host, "zero", graph_file(name, tmp_path), "4", "11"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flag 1" in r.stdout.splitlines()


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = _build(str(tmp_path / "essgraph_sparse_host_san"), ("-g", "-fsanitize=address,undefined",
                                                              "-fno-sanitize-recover=all"))
    for name, leaf in (("A_ring6", 0), ("C_cov40", 4), ("G_mid100", 16), ("H_cov130", 4)):
        for mode in ("solve", "zero"):
            r = subprocess.run([exe, mode, graph_file(name, tmp_path), str(leaf), "3"], capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
