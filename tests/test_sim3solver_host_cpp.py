"""mcs::Sim3Solver of the C++ host mirror (multicol-slam-annotation_amd/host/mcs_multicol.hpp) and
the draw helper as a program of its own.

Without a GPU: tests/cpp/sim3solver_draws.cpp includes csrc/sim3_draws.hpp alone (no library), checks
it against a literal array restatement and prints triples for given draws, which must equal
np_draw_samples.  On the GPU: tests/cpp/sim3solver_demo.cpp runs the loop shape of
cLoopClosing::ComputeSim3 (iterate(50) per visit, one more visit after a success) through the
adapter; the program prints the sample triples the adapter drew, and every visit must
equal the replay of the acceptance rule over the restatement's counts."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_sim3solver_ref import CAP, get_case, np_draw_samples, np_max_its, np_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def draws_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("s3s_draws") / "sim3solver_draws")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "sim3solver_draws.cpp"),
                           "-o", exe])
    return exe


def test_draw_program_self_check(draws_exe):
    out = subprocess.run([draws_exe, "self"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    tag, triples, repeats, past = out.stdout.split()
    assert tag == "ok" and int(triples) == 16000 and int(repeats) > 100 and int(past) > 100


def test_draw_program_equals_the_restatement(draws_exe):
    rng = np.random.default_rng(3)
    for n in (3, 5, 15, 50):
        d = rng.integers(0, n, (40, 3))
        out = subprocess.run([draws_exe, str(n)] + [str(x) for x in d.ravel()], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        got = np.array([ln.split() for ln in out.stdout.splitlines()], np.int32)
        assert np.array_equal(got, np_draw_samples(n, d))
    out = subprocess.run([draws_exe, "5", "0", "5", "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1


def build_demo(tmp_path):
    lib = os.path.join(ROOT, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "sim3solver_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "sim3solver_demo.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib, "-lmcs_amd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_demo_compiles_against_adapter_header(built, tmp_path):
    assert os.path.exists(build_demo(tmp_path))


def write_inputs(d, case, t):
    d.mkdir()

    def put(fname, a, dt):
        np.ascontiguousarray(a, dt).tofile(str(d / (fname + ".bin")))
    rig = case["rig"]
    for k in ("m_c", "cam", "scale"):
        put(k, rig[k], np.float64)
    put("sigma2", case["sigma2"], np.float64)
    for p, kf, pts, ok in (("k1_", case["kf1"], case["pts1"], case["ok1"]),
                           ("k2_", case["kf2s"][t], case["pts2s"][t], case["ok2s"][t])):
        put(p + "kp_octave", kf["kp_octave"], np.int32)
        put(p + "kp_cam", kf["kp_cam"], np.int32)
        put(p + "m_t", kf["m_t"], np.float64)
        put(p + "mp_pos", pts["pos"], np.float64)
        put(p + "has", np.ones(len(ok)), np.uint8)
        put(p + "bad", 1 - np.asarray(ok), np.uint8)
    put("matches12", case["matches12"][t], np.int32)
    put("first1", case["first1"], np.int32)
    put("first2", case["first2s"][t], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [0, 1, 2])
def test_adapter_runs_the_compute_sim3_loop(gpu, tmp_path, t):
    case = dict(get_case("t3_mixed"))
    N = case["rows"][t]["n"]
    exe = build_demo(tmp_path)
    write_inputs(tmp_path / "in", case, t)
    out = subprocess.run([exe, str(tmp_path / "in"), "77"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    get = lambda k: [ln[1:] for ln in lines if ln[0] == k]  # noqa: E731
    assert int(get("N")[0][0]) == N and int(get("max_its")[0][0]) == np_max_its(N)[0]
    # the triples the adapter drew (std::mt19937 through mcs_sim3_draw_samples), as the program prints them
    smp = np.array(get("samples")[0], np.int32).reshape(CAP, 3)
    assert ((smp >= 0) & (smp < N)).all() and len(np.unique(smp)) > min(N, 10) - 1
    case["samples"] = case["samples"].copy()
    case["samples"][t] = smp
    visits = [[int(x) for x in v] for v in get("visit")]
    state, first, want_visits = None, None, []
    while True:
        s = np_solve(case, t, 50, state)
        assert all(c[1].sum() == 0 for c in s["checks"])          # no decision within the margin
        want_visits.append([int(s["success"]), int(s["no_more"]), s["counts"][s["khit"]] if s["success"] else 0, s["iterations"]])
        if s["success"] and first is None:
            first = s
        if s["no_more"] or (state is not None and state.get("extra")):
            break
        state = dict(iterations=s["iterations"], best=s["best"], max_its=s["max_its"], extra=s["success"])
    # the device's hypotheses differ from eigh's by rounding only (stage A), far inside the margin
    assert visits == want_visits
    if first is not None:
        inl = np.zeros(len(case["kf1"]["kp_xy"]), np.uint8)
        inl[case["rows"][t]["idx1"][first["checks"][first["khit"]][0]]] = 1
        assert np.array_equal(np.array(get("inliers")[0], np.uint8), inl)
