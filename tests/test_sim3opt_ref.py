"""OptimizeSim3 (reference src/cOptimizerLoopStuff.cpp:63-270) without a GPU: csrc/sim3_opt_math.hpp
over csrc/lm_control.hpp as the stand-alone program tests/cpp/sim3opt_host.cpp, against
tests/golden/sim3opt_ref.npz, which the reference's own g2o produced
(tests/golden/gen_sim3opt_ref.py).

Integers and sets are exact: the kept slots, n_corr, n_bad, the nulled matches, n_in, n_undefined,
the iteration counts of both rounds and the LM trials of every iteration.  Reals (s, q up to sign,
t, the round chi2, edge_chi2) agree to max(8 x the spread the reference shows between the
difference steps 0.5e-9, 1e-9 and 2e-9 of its numeric Jacobian, 1e-9 of the field's scale): the
analytic Jacobian and another summation order sit at the scale of that scatter, not inside it.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import ref_g2o_bind
from tests import sim3opt_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "sim3opt_ref.npz")
NEW_SYMBOLS = ["mcs_sim3_opt_default_options", "mcs_sim3_opt_workspace_create", "mcs_sim3_opt_workspace_destroy",
               "mcs_optimize_sim3_device", "mcs_sim3_merge_matches_device", "mcs_optimize_sim3"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3opt") / "sim3opt_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "sim3opt_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def run_host(host, case, tmp_path):
    path = str(tmp_path / (case["name"] + ".txt"))
    sc.write_case_file(case, path)
    return sc.parse_results(subprocess.check_output([host, "run", path], text=True), case["matches12"].shape[1])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_program_equals_the_reference_g2o(host, fix, tmp_path, name):
    case = sc.make_case(name)
    assert sc.digest(case) == str(fix[name + "_sha256"]), "the seeded inputs are not those of the fixture"
    sc.compare(fix, name, run_host(host, case, tmp_path))


def test_cases_cover_what_their_names_say(fix):
    assert fix["A_clean_n_corr"][0] == 40 and fix["A_clean_n_bad"][0] == 0
    assert fix["B_outliers_n_corr"][0] == 130 and fix["B_outliers_n_bad"][0] >= 20
    assert fix["C_batch_n_corr"].tolist() == [0, 2, 3, 70]
    assert fix["C_batch_n_in"][1] == 0 and fix["C_batch_n_in"][2] == 3          # the `< 3` return and the exact minimum
    assert fix["D_below3_n_corr"][0] - fix["D_below3_n_bad"][0] < 3 and fix["D_below3_n_in"][0] == 0
    assert fix["F_gainstop_iters"][0, 1] == 0 and fix["I_round2_iters"][0, 1] > 0
    assert fix["H_undefined_n_undefined"][0] == 6
    assert fix["G_own_camera_n_bad"][0] != fix["B_outliers_n_bad"][0]
    # the cases named for the kernel's rounds of 256 slots / 256 rows, on the fixture alone
    rows = {}
    for name in ("J_rounds", "K_batch_wide", "L_round2_wide"):
        for t in range(len(fix[name + "_n_corr"])):
            kept = ~np.isnan(fix[name + "_edge_chi2"][t][:, 0])
            assert kept.sum() == fix[name + "_n_corr"][t]
            culled = kept & (fix[name + "_matches12"][t] < 0)
            rows[name, t] = (np.flatnonzero(kept), (np.cumsum(kept) - 1)[culled])
    for name, t, rounds in (("J_rounds", 0, 2), ("K_batch_wide", 0, 3), ("K_batch_wide", 1, 3), ("L_round2_wide", 0, 2)):
        slots = rows[name, t][0]
        assert len(slots) > 256, (name, t)
        for r in range(rounds):                 # kept slots in every round of 256, so `base` carries a row offset
            assert ((slots >= 256 * r) & (slots < 256 * (r + 1))).any(), (name, t, r)
    assert fix["J_rounds_n_bad"][0] > 0 and fix["J_rounds_n_undefined"][0] == 6
    case = sc.make_case("J_rounds")
    undef = np.array(case["undefined"][0])
    assert (undef < 256).any() and (undef >= 256).any()
    skipped = np.flatnonzero((case["matches12"][0] >= 0) & np.isnan(fix["J_rounds_edge_chi2"][0][:, 0]))
    skipped = np.setdiff1d(skipped, undef)      # the four skip rules: matched, defined and not kept
    assert len(skipped) == 4 and (skipped >= 256).all(), skipped
    assert fix["K_batch_wide_n_corr"].tolist() == [300, 257, 0, 5] and fix["K_batch_wide_n_bad"][0] > 0
    assert fix["K_batch_wide_n_in"][2] == 0 and (fix["K_batch_wide_iters"][2] == 0).all()
    assert fix["K_batch_wide_n_corr"][3] - fix["K_batch_wide_n_bad"][3] < 3 and fix["K_batch_wide_n_in"][3] == 0
    assert sc.make_case("K_batch_wide")["matches12"].shape == (4, 520)          # three slot rounds, the last partial
    assert fix["L_round2_wide_iters"][0, 1] > 0
    culled = rows["L_round2_wide", 0][1]        # pairs taken out in both rounds of 256 rows of the cull loop
    assert (culled < 256).any() and (culled >= 256).any(), culled
    assert fix["L_round2_wide_n_in"][0] > 256   # round 2 iterates over more live rows than one round
    for name in sc.CASES:                       # a Sim3 returned before the recover is the input
        case = sc.make_case(name)
        for t in range(len(case["kf2s"])):
            if fix[name + "_n_corr"][t] - fix[name + "_n_bad"][t] < 3:
                assert fix[name + "_s"][t] == case["s12"][t] and np.array_equal(fix[name + "_t"][t], case["t12"][t])


def test_crossed_cameras_differ_from_own_in_every_case():
    for name in sc.CASES:
        case = sc.make_case(name)
        n = 0
        for t, kf2 in enumerate(case["kf2s"]):
            for i in np.nonzero(case["matches12"][t] >= 0)[0]:
                i2 = int(case["first2s"][t][case["matches12"][t][i]])
                n += 0 <= i2 < len(case["kf1"]["kp_cam"]) and case["kf1"]["kp_cam"][i2] != case["kf1"]["kp_cam"][i]
        assert n >= 1, name


def test_analytic_jacobian_against_central_differences(host, tmp_path):
    """1 000 random (S, X, camera) draws.  The central difference at 1e-6 of a pixel value near
    700 (ulp 1.1e-13, a few ulp of evaluation error) carries about 1e-12 / 2e-6 = 5e-7 of absolute
    noise plus a truncation term of 1e-12 f''' / 6, on entries of 1e2 to 1e3: 1e-6 relative to the
    largest entry of the edge's block (at least 1) bounds both with room."""
    path = str(tmp_path / "rig.txt")
    sc.write_case_file(sc.make_case("D_below3"), path)
    out = subprocess.check_output([host, "jac", path, "7", "1000"], text=True).split()
    print("worst relative error", out[1])
    assert out[0] == "jac" and float(out[1]) < 1e-6


def test_sim3_round_trips_on_both_sides_of_each_eps_branch(host):
    """S S^-1 = 1, (S^-1)^-1 = S, S (S^-1 x) = x and (S S) x = S (S x) for sigma and theta on both
    sides of eps = 1e-5: below theta = eps the text's R = I + W + W^2 is a rotation to
    theta^2 / 2 <= 5e-11 only, hence 1e-9.  exp(-u) = exp(u)^-1 holds to eps |upsilon| only,
    because the branches below eps take the limits of A, B and C while s stays exp(sigma):
    upsilon is 0.37 long, hence 1e-5.  The branch |sigma| >= eps, 0 < theta < eps is left out of
    that identity: its B (sim3.h:116) grows like 1 / sigma^3, as written."""
    out = subprocess.check_output([host, "exp"], text=True).split()
    print("worst errors", out[1:])
    assert out[0] == "exp" and float(out[1]) < 1e-9 and float(out[2]) < 1e-5


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES and hasattr(mcs_amd.lib(), s), s


def test_host_entry_argument_errors_and_no_device(built):
    import mcs_amd
    from mcs_amd import sim3_opt
    case = sc.make_case("D_below3")
    tail = (case["inv_sigma2_1"], case["sigma2_2"], case["s12"], case["R12"], case["t12"])
    for kw in (dict(options=dict(its_round1=99)), dict(options=dict(max_trials=0)), dict(options=dict(std_sim=0.0)),
               dict(flags=8)):
        with pytest.raises(mcs_amd.McsError) as e:      # all argument errors come before any device use
            sim3_opt.optimize_sim3(*sc.call_args(case), *tail, **kw)
        assert e.value.code == mcs_amd.MCS_ERR_ARG, kw
    if mcs_amd.device_count() < 1:
        with pytest.raises(mcs_amd.McsError) as e:
            sim3_opt.optimize_sim3(*sc.call_args(case), *tail)
        assert e.value.code == mcs_amd.MCS_ERR_NO_DEVICE


REF_G2O = os.path.join(os.environ.get("MCS_REFERENCE", "/root/reference"), "ThirdParty", "g2o", "g2o", "types", "sim3.h")


@pytest.mark.skipif(not (ref_g2o_bind.available() and os.path.exists(REF_G2O)),
                    reason="needs oracle/_ref/libg2o_ref.so and the reference checkout's g2o headers")
def test_fixture_regenerates_from_the_reference_g2o(fix, tmp_path):
    from tests.golden import gen_sim3opt_ref as gen
    exe = gen.build_driver(str(tmp_path))
    case = sc.make_case("E_skips")
    runs = gen.run_reference(exe, case, str(tmp_path))
    for f in gen.INTS + gen.REALS:
        want = fix["E_skips_" + f]
        have = np.stack([np.asarray(r[f]) for r in runs[0]])
        assert np.array_equal(have, want, equal_nan=have.dtype.kind == "f"), f
    spread = gen.check_and_measure("E_skips", runs)
    for f in gen.REALS:
        assert np.array_equal(spread[f], fix["measured_E_skips_" + f]), f
