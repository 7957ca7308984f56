"""mcs::OptimizeSim3 of the C++ host mirror (multicol-slam-annotation_amd/host/mcs_multicol.hpp):
tests/cpp/sim3opt_demo.cpp compiles against the adapter header without a GPU, and on the GPU the
adapter reproduces A_clean (a recovered Sim3) and D_below3 (the `< 3` return: nIn = 0, matches
nulled, Sim3 untouched) of tests/golden/sim3opt_ref.npz."""
import os
import subprocess

import numpy as np
import pytest

from tests import sim3opt_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "sim3opt_ref.npz")


def build_demo(tmp_path):
    lib = os.path.join(ROOT, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "sim3opt_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "sim3opt_demo.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib, "-lmcs_amd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_demo_compiles_against_adapter_header(built, tmp_path):
    assert os.path.exists(build_demo(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A_clean", "D_below3"])
def test_adapter_reproduces_the_fixture(gpu, tmp_path, name):
    fix = np.load(FIX)
    case = sc.make_case(name)
    path = str(tmp_path / "case.txt")
    sc.write_case_file(case, path)
    out = subprocess.run([build_demo(tmp_path), path], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    assert int(lines["n_in"][0]) == fix[name + "_n_in"][0]
    assert np.array_equal(np.array(lines["matches"], np.int32), fix[name + "_matches12"][0])
    v = np.array([float(x) for x in lines["sim3"]])
    s, R, t = v[0], v[1:10].reshape(3, 3), v[10:13]
    if fix[name + "_n_in"][0] == 0:                  # returned before the recover: the input, bit for bit
        assert s == case["s12"][0] and np.array_equal(R.reshape(9), case["R12"][0]) and np.array_equal(t, case["t12"][0])
        return
    assert abs(s - fix[name + "_s"][0]) <= sc.tolerance(fix, name, "s", 0)
    assert np.abs(t - fix[name + "_t"][0]).max() <= sc.tolerance(fix, name, "t", 0)
    w, x, y, z = fix[name + "_q"][0]
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.abs(R - Rq).max() <= 4 * sc.tolerance(fix, name, "q", 0)    # R is quadratic in q: |dR| <= 4 |dq|
