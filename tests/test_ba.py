"""Bundle adjustment: oracle self-checks (CPU) and GPU parity vs the oracle (tolerance).

Reference: EdgeProjectXYZ2MCS (src/g2o_MultiCol_vertices_edges.cpp:32-129), g2o LM + Schur
(ThirdParty/g2o/g2o/core), cOptimizer::LocalBundleAdjustment (src/cOptimizer.cpp:489-908).
Tolerances: Jacobian rel 1e-9 (vs central differences: 1e-6, FD-limited);
GPU vs oracle per-edge error/Jacobian rel 1e-9; robust chi2 per iteration rel 1e-6;
final poses abs 1e-6, points abs 1e-5 (well-constrained points).
"""
import numpy as np
import pytest

from tests import oracle_bind as ob


@pytest.fixture(scope="module")
def problem():
    from mcs_amd import ba
    return ba.make_problem(seed=0)


@pytest.fixture(scope="module")
def small_problem():
    from mcs_amd import ba
    return ba.make_problem(n_local=4, n_fixed=1, n_points=300, target_edges=2000, seed=3)


def _fd_jac(pr, e, h=1e-6):
    k, p, c = pr["edge_pose"][e], pr["edge_point"][e], pr["edge_cam"][e]
    args = lambda dp, dx: (pr["poses"][k] + dp, pr["points"][p] + dx, pr["mc"][c], pr["cam"][c],
                           pr["edge_meas"][e])
    nj = np.zeros((2, 6))
    nl = np.zeros((2, 3))
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        nj[:, i] = (ob.ba_edge(*args(d, 0))[0] - ob.ba_edge(*args(-d, 0))[0]) / (2 * h)
    for i in range(3):
        d = np.zeros(3)
        d[i] = h
        nl[:, i] = (ob.ba_edge(*args(0, d))[0] - ob.ba_edge(*args(0, -d))[0]) / (2 * h)
    return nj, nl


def test_oracle_jacobian_matches_central_differences(problem):
    for e in range(0, len(problem["edge_pose"]), 997):
        k, p, c = problem["edge_pose"][e], problem["edge_point"][e], problem["edge_cam"][e]
        _, jp, jl = ob.ba_edge(problem["poses"][k], problem["points"][p], problem["mc"][c],
                               problem["cam"][c], problem["edge_meas"][e])
        nj, nl = _fd_jac(problem, e)
        assert np.abs(jp - nj).max() <= 1e-6 * max(1.0, np.abs(nj).max())
        assert np.abs(jl - nl).max() <= 1e-6 * max(1.0, np.abs(nl).max())


def test_oracle_zero_residual_at_ground_truth(problem):
    # measurement = noiseless projection -> zero error
    pr = dict(problem)
    for e in range(0, len(pr["edge_pose"]), 1500):
        k, p, c = pr["edge_pose"][e], pr["edge_point"][e], pr["edge_cam"][e]
        err0, _, _ = ob.ba_edge(pr["gt_poses"][k], pr["gt_points"][p], pr["mc"][c], pr["cam"][c],
                                np.zeros(2))
        err, _, _ = ob.ba_edge(pr["gt_poses"][k], pr["gt_points"][p], pr["mc"][c], pr["cam"][c],
                               -err0)
        assert np.abs(err).max() < 1e-9


def test_oracle_lm_monotone_and_converges(small_problem):
    r = ob.ba_optimize(small_problem, trace=20)
    tr = r["trace"]
    assert r["report"].chi2_final < r["report"].chi2_initial
    assert (np.diff(tr) <= 1e-9 * tr[:-1]).all()   # accepted steps never increase chi2


def test_oracle_local_ba_semantics(small_problem):
    L = ob.local_ba(small_problem, stop_flag=0)
    assert L["report1"].iterations >= 1
    if L["write_back"]:
        assert L["report2"].n_active_edges == int(L["edge_inlier"].sum()) or \
            L["report2"].n_active_edges >= int(L["edge_inlier"].sum())
    # a stop flag raised before the call aborts everything (:771-773)
    L2 = ob.local_ba(small_problem, stop_flag=1)
    assert L2["write_back"] == 0 and np.array_equal(L2["poses"], small_problem["poses"])


def test_oracle_converged_problem_sets_stop_flag():
    from mcs_amd import ba
    pr = ba.make_problem(n_local=3, n_fixed=1, n_points=200, target_edges=1200, seed=5,
                         outlier_frac=0.0, noise_scale=0.0, pose_noise=(1e-4, 1e-4), point_noise=1e-4)
    r = ob.ba_optimize(pr, stop_flag=0)
    # the terminate action ends a converged optimisation by writing the caller's flag
    assert r["stop_flag"] == 1 or r["report"].iterations == 10


@pytest.mark.gpu
def test_gpu_linearize_matches_oracle(gpu, problem):
    from mcs_amd import ba
    S = ba.Solver()
    err, jp, jl = S.linearize(problem)
    for e in range(0, len(problem["edge_pose"]), 313):
        k, p, c = problem["edge_pose"][e], problem["edge_point"][e], problem["edge_cam"][e]
        oe, ojp, ojl = ob.ba_edge(problem["poses"][k], problem["points"][p], problem["mc"][c],
                                  problem["cam"][c], problem["edge_meas"][e])
        assert np.allclose(err[e], oe, rtol=1e-9, atol=1e-9)
        assert np.allclose(jp[e], ojp, rtol=1e-9, atol=1e-9 * np.abs(ojp).max())
        assert np.allclose(jl[e], ojl, rtol=1e-9, atol=1e-9 * np.abs(ojl).max())


def _well_constrained(pr, min_obs=3):
    cnt = np.bincount(pr["edge_point"], minlength=len(pr["points"]))
    return cnt >= min_obs


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "configC"])
def test_gpu_optimize_matches_oracle(gpu, which, problem, small_problem):
    from mcs_amd import ba
    pr = small_problem if which == "small" else problem
    S = ba.Solver()
    g = S.optimize(pr, trace=20)
    o = ob.ba_optimize(pr, trace=20)
    assert g["report"].iterations == o["report"].iterations
    assert g["report"].n_active_poses == o["report"].n_active_poses
    assert np.allclose(g["trace"], o["trace"], rtol=1e-6)
    assert abs(g["report"].chi2_final - o["report"].chi2_final) <= 1e-6 * o["report"].chi2_final
    assert np.abs(g["poses"] - o["poses"]).max() < 1e-6
    wc = _well_constrained(pr)
    assert np.abs(g["points"][wc] - o["points"][wc]).max() < 1e-5
    _check_two_obs_points(pr, g, o)


def _check_two_obs_points(pr, g, o, inlier=None):
    """Points seen twice: a 3x3 Hll of two rank-2 blocks is the worst-conditioned part of the
    system, so rounding-level differences (fixed-order device sums vs the oracle's sums) reach
    them amplified.  Bound: 1e-5 of the point's own scale (its distance from the origin)."""
    ep = pr["edge_point"] if inlier is None else pr["edge_point"][inlier.astype(bool)]
    two = np.bincount(ep, minlength=len(pr["points"])) == 2
    two &= np.bincount(pr["edge_point"], minlength=len(pr["points"])) == 2
    if not two.any():
        return
    scale = np.maximum(1.0, np.linalg.norm(o["points"][two], axis=1))
    rel = np.abs(g["points"][two] - o["points"][two]).max(axis=1) / scale
    assert rel.max() < 1e-5, "2-observation points: max relative difference %.3g" % rel.max()


@pytest.mark.gpu
def test_gpu_optimize_bitwise_reproducible(gpu, small_problem):
    from mcs_amd import ba
    S = ba.Solver()
    a = S.optimize(small_problem)
    b = S.optimize(small_problem)
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])


@pytest.mark.gpu
def test_gpu_local_ba_matches_oracle(gpu, problem):
    from mcs_amd import ba
    S = ba.Solver()
    g = S.local_ba(problem)
    o = ob.local_ba(problem)
    assert g["write_back"] == o["write_back"]
    assert g["report1"].iterations == o["report1"].iterations
    assert g["report2"].iterations == o["report2"].iterations
    assert np.array_equal(g["edge_inlier"], o["edge_inlier"])
    assert np.abs(g["poses"] - o["poses"]).max() < 1e-6
    wc = _well_constrained(problem)
    assert np.abs(g["points"][wc] - o["points"][wc]).max() < 1e-5
    _check_two_obs_points(problem, g, o, inlier=o["edge_inlier"])


@pytest.mark.gpu
def test_gpu_stop_flag_semantics(gpu, small_problem):
    from mcs_amd import ba
    S = ba.Solver()
    g = S.local_ba(small_problem, stop_flag=1)
    assert g["write_back"] == 0 and np.array_equal(g["poses"], small_problem["poses"])
    pr = ba.make_problem(n_local=3, n_fixed=1, n_points=200, target_edges=1200, seed=5,
                         outlier_frac=0.0, noise_scale=0.0, pose_noise=(1e-4, 1e-4), point_noise=1e-4)
    r = S.optimize(pr, stop_flag=0)
    o = ob.ba_optimize(pr, stop_flag=0)
    assert r["stop_flag"] == o["stop_flag"] and r["report"].iterations == o["report"].iterations


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["configC", "culled", "duplicate_groups", "small"])
def test_gpu_device_schur_structure_matches_host(gpu, case, problem, small_problem):
    """The Schur pair lists and k_schur work items the product builds on the device are
    entry-for-entry those of the host restatement of BlockSolver::buildStructure
    (block_solver.hpp:143-295 via ba_structure.hpp build_pairs_host): block pointers, every
    (e1, e2) pair in (point, e1, e2) order inside its block, every work item."""
    import ctypes
    from mcs_amd import ba, lib
    pr = dict(small_problem if case == "small" else problem)
    level = None
    if case == "culled":   # LocalBA round 2: some edges at level 1
        rng = np.random.default_rng(3)
        level = (rng.random(len(pr["edge_pose"])) < 0.1).astype(np.uint8)
    if case == "duplicate_groups":   # a point observed twice by one pose (multi-edge groups)
        k = 40
        for key in ("edge_pose", "edge_point", "edge_cam"):
            pr[key] = np.concatenate([pr[key], pr[key][:k]])
        pr["edge_meas"] = np.concatenate([pr["edge_meas"], pr["edge_meas"][:k] + 0.5])
        pr["edge_info"] = np.concatenate([pr["edge_info"], pr["edge_info"][:k]])
    s = ba.as_struct(pr)
    solver = ba.Solver()
    lv = None if level is None else level.ctypes.data_as(ctypes.c_void_p)
    bad = lib().mcs_ba_check_structure(solver._h, ctypes.byref(s), lv)
    assert bad == 0, bad


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "configC"])
def test_gpu_device_driven_lm_matches_host_driven(gpu, which, problem, small_problem):
    """The device-driven LM loop (timing off: k_build_trial, k_edges_end with the LM decision in
    its last-arriving workgroup) against the host-driven loop (timing on: k_build +
    k_point_trial, k_edges + host decision).  The trial chi2 is summed in another order, so
    values agree to rounding, decisions exactly."""
    from mcs_amd import ba
    pr = small_problem if which == "small" else problem
    D = ba.Solver()
    H = ba.Solver()
    H.enable_timing(True)
    for fn in ("local_ba", "optimize"):
        d = getattr(D, fn)(pr)
        h = getattr(H, fn)(pr)
        for rk in (("report1", "report2") if fn == "local_ba" else ("report",)):
            assert d[rk].iterations == h[rk].iterations
            assert abs(d[rk].chi2_final - h[rk].chi2_final) <= 1e-9 * h[rk].chi2_final
        if fn == "local_ba":
            assert np.array_equal(d["edge_inlier"], h["edge_inlier"])
            assert d["write_back"] == h["write_back"]
        assert np.abs(d["poses"] - h["poses"]).max() < 1e-9
        assert np.abs(d["points"] - h["points"]).max() < 1e-7


@pytest.mark.gpu
def test_gpu_long_trace_selects_host_driven_loop(gpu, small_problem):
    """The driver selection by trace length: a caller asking for more than the device loop's 64
    trace entries of a run allowed more than 64 iterations gets the host-driven loop, one asking
    for 64 the device-driven one.  Same controller, so the same decisions; the trial sums are
    added in another order, so values agree to rounding."""
    from mcs_amd import ba
    S = ba.Solver()
    o = ba.BAOptions(max_iterations=80)
    h = S.optimize(small_problem, options=o, trace=80)
    d = S.optimize(small_problem, options=o, trace=64)
    hr, dr = h["report"], d["report"]
    assert hr.iterations == dr.iterations and hr.stop_flag == dr.stop_flag
    assert (hr.n_active_edges, hr.n_active_poses, hr.n_active_points) == \
        (dr.n_active_edges, dr.n_active_poses, dr.n_active_points)
    assert abs(dr.chi2_final - hr.chi2_final) <= 1e-9 * hr.chi2_final
    assert len(h["trace"]) == hr.iterations and len(d["trace"]) == dr.iterations
    assert hr.iterations > 0
    m = min(len(h["trace"]), len(d["trace"]))
    assert np.all(np.abs(d["trace"][:m] - h["trace"][:m]) <= 1e-9 * np.abs(h["trace"][:m]))


@pytest.mark.gpu
def test_gpu_local_ba_bitwise_reproducible(gpu, problem):
    """Device-driven LocalBA twice: the arrival counter and every sum order are fixed, so the
    results are the same bits."""
    from mcs_amd import ba
    S = ba.Solver()
    a = S.local_ba(problem)
    b = S.local_ba(problem)
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])
    assert np.array_equal(a["edge_inlier"], b["edge_inlier"])


def _pose_leaves_problem():
    """Config-C-style small problem whose last local pose keeps 12 edges, all moved ~2000 px:
    round 1's culling (cOptimizer.cpp:798-817) removes every one of them, so that pose leaves the
    system of round 2 (g2o's initializeOptimization drops a vertex without active edges)."""
    from mcs_amd import ba
    pr = dict(ba.make_problem(n_local=4, n_fixed=1, n_points=300, target_edges=2000, seed=3))
    rng = np.random.default_rng(0)
    k = int(np.nonzero(pr["pose_fixed"] == 0)[0][-1])
    ek = np.nonzero(pr["edge_pose"] == k)[0]
    m = np.ones(len(pr["edge_pose"]), bool)
    m[ek[12:]] = False
    for key in ("edge_pose", "edge_point", "edge_cam", "edge_meas", "edge_info"):
        pr[key] = pr[key][m]
    ek = np.nonzero(pr["edge_pose"] == k)[0]
    pr["edge_meas"] = pr["edge_meas"].copy()
    pr["edge_meas"][ek] += rng.uniform(-2000.0, 2000.0, (len(ek), 2))
    return pr, k


def test_oracle_pose_leaves_after_culling():
    pr, k = _pose_leaves_problem()
    o = ob.local_ba(pr)
    assert o["report1"].n_active_poses == 4 and o["report2"].n_active_poses == 3
    assert o["edge_inlier"][pr["edge_pose"] == k].sum() == 0 and o["write_back"] == 1


@pytest.mark.gpu
def test_gpu_local_ba_pose_leaves_after_culling(gpu):
    """The device-culled LocalBA (k_lba_cull / k_lba_compact between the rounds) finds that an
    active pose lost every edge and runs round 2 from scratch on the host's copy of round 1's
    state: the same rounds, inlier set and write-back as the oracle and as the host-culled flow
    (timing on).  The left pose is fitted to 12 outliers only, so its estimate is compared
    loosely; every other pose and the well-constrained points as in the config-C test."""
    from mcs_amd import ba
    pr, k = _pose_leaves_problem()
    g = ba.Solver().local_ba(pr)
    H = ba.Solver()
    H.enable_timing(True)
    h = H.local_ba(pr)
    o = ob.local_ba(pr)
    for r in (g, h):
        assert r["report2"].n_active_poses == 3
        assert r["write_back"] == o["write_back"]
        assert r["report1"].iterations == o["report1"].iterations
        assert r["report2"].iterations == o["report2"].iterations
        assert np.array_equal(r["edge_inlier"], o["edge_inlier"])
    keep = np.arange(len(pr["poses"])) != k
    assert np.abs(g["poses"][keep] - o["poses"][keep]).max() < 1e-6
    assert np.abs(g["poses"][k] - o["poses"][k]).max() < 1e-3
    wc = _well_constrained(pr)
    assert np.abs(g["points"][wc] - o["points"][wc]).max() < 1e-5
    assert np.abs(g["poses"] - h["poses"]).max() < 1e-6


def _outlier_points_problem():
    """_pose_leaves_problem with eight points (three or more edges each, none on the leaving
    pose) whose every measurement is moved ~2000 px.  Round 1 culls their edges until the point
    goes bad; an extra observation keeps the point alive one edge longer, so the inlier flags
    depend on extra_obs, and the points end with at most one edge: not written back."""
    pr, k = _pose_leaves_problem()
    n = len(pr["points"])
    cnt = np.bincount(pr["edge_point"], minlength=n)
    on_k = np.zeros(n, bool)
    on_k[pr["edge_point"][pr["edge_pose"] == k]] = True
    sel = np.isin(pr["edge_point"], np.nonzero((cnt >= 3) & ~on_k)[0][:8])
    pr["edge_meas"][sel] += np.random.default_rng(1).uniform(-2000.0, 2000.0, (int(sel.sum()), 2))
    return pr


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["pose_leaves", "outlier_points"])
def test_gpu_local_ba_ex_flows_agree_on_write_back_mask(gpu, which):
    """local_ba_ex with extra observations on every third point, through the device-culled flow
    (which falls back to a host round 2 here: a pose leaves), the host-culled flow (timing on) and
    the oracle: the same point_write mask, inlier flags, write-back and iteration counts.

    On _pose_leaves_problem the oracle writes every point back (point_write is all ones) and
    its results do not depend on extra_obs, whatever the modulus: point_write cannot, because a
    point is bad only once fewer than two of its edges are left, which alone clears its flag.
    The second case adds points that are outliers as a whole: there the oracle's point_write
    has 10 zeros among 300 and extra_obs changes 4 inlier flags (modulus 3 kept)."""
    from mcs_amd import ba
    pr = _pose_leaves_problem()[0] if which == "pose_leaves" else _outlier_points_problem()
    extra_obs = (np.arange(len(pr["points"])) % 3 == 0).astype(np.int32)
    o = ob.local_ba_ex(pr, extra_obs)
    if which == "outlier_points":
        assert 0 < o["point_write"].sum() < len(o["point_write"])
        assert not np.array_equal(o["edge_inlier"], ob.local_ba_ex(pr, None)["edge_inlier"])
    g = ba.Solver().local_ba_ex(pr, extra_obs)
    H = ba.Solver()
    H.enable_timing(True)
    h = H.local_ba_ex(pr, extra_obs)
    for r in (g, h):
        assert np.array_equal(r["point_write"], o["point_write"])
        assert np.array_equal(r["edge_inlier"], o["edge_inlier"])
        assert r["write_back"] == o["write_back"]
        assert r["report1"].iterations == o["report1"].iterations
        assert r["report2"].iterations == o["report2"].iterations


@pytest.mark.gpu
def test_gpu_local_ba_multi_tile_matches_oracle(gpu):
    """LocalBA with 14 local keyframes: 84 pose unknowns, so the reduced system spans two 64x64
    tiles (pipelined LDL^T, k_schur_fin launches) while the culling runs on the device; the same
    rounds, inlier set and write-back as the oracle and as the host-culled flow (timing on)."""
    from mcs_amd import ba
    pr = ba.make_problem(n_local=14, n_fixed=2, n_points=800, target_edges=6000, seed=4)
    g = ba.Solver().local_ba(pr)
    H = ba.Solver()
    H.enable_timing(True)
    h = H.local_ba(pr)
    o = ob.local_ba(pr)
    assert g["report1"].n_active_poses == 14
    for r in (g, h):
        assert r["write_back"] == o["write_back"]
        assert r["report1"].iterations == o["report1"].iterations
        assert r["report2"].iterations == o["report2"].iterations
        assert np.array_equal(r["edge_inlier"], o["edge_inlier"])
    assert np.abs(g["poses"] - o["poses"]).max() < 1e-6
    wc = _well_constrained(pr)
    assert np.abs(g["points"][wc] - o["points"][wc]).max() < 1e-5
    assert np.abs(g["poses"] - h["poses"]).max() < 1e-8
