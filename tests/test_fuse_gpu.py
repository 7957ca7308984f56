"""cORBmatcher::Fuse on the device (mcs_fuse, mcs_fuse_device; reference src/cORBmatcher.cpp
:1265-1719) against the NumPy restatement of tests/test_fuse_ref.py, at the kernel's edge shapes.

All comparisons are exact (integers and bytes, best_dist as an integer) over every (target,
query, camera) triple.  The inputs keep the 1e-9 margin of tests/test_fuse_ref.py on every
decision that depends on atan (asserted on each input), so a last-ulp difference between the
device's atan and libm's cannot flip one; everything else is the same correctly rounded
operations in the same order on both sides."""
import ctypes

import numpy as np
import pytest

from tests.test_fuse_ref import (INT_MAX, MARGIN, SCENARIOS, check_sequence_against_text, load_scenario, build_fuse_demo, make_case, make_queries, make_rig,
                                 make_target, np_fuse_candidates, np_fuse_select, np_fuse_sequence, np_grid,
                                 th_low)

pytestmark = pytest.mark.gpu


def _fz():
    from mcs_amd import fuse
    return fuse


def run_device(rule, rig, targets, q, th, tl, flags=0, q_skip=None, ws=None):
    import torch
    fz = _fz()
    nbytes = q["desc"].shape[1]
    ts, qs, keep = fz.device_sets(fz.pack_targets(rig, targets, nbytes), fz.pack_queries(q, nbytes))
    sk = torch.from_numpy(np.ascontiguousarray(q_skip, np.uint8)).cuda() if q_skip is not None else None
    bk, bd, ep = fz.fuse_device(ws, rule, ts, qs, th, tl, flags=flags, q_skip=sk)
    torch.cuda.synchronize()
    return bk.cpu().numpy(), bd.cpu().numpy(), ep.cpu().numpy() if ep is not None else None


def check(rule, rig, targets, q, th=3.0, tl=None, flags=0, q_skip=None, ws=None, host=True):
    """Device entry (and host entry) == restatement on every triple -> the restatement."""
    fz = _fz()
    tl = th_low(q["desc"].shape[1], q.get("mask") is not None) if tl is None else tl
    want = np_fuse_candidates(rule, rig, targets, q, th, tl, flags=flags, q_skip=q_skip)
    assert want["margin"] > MARGIN
    got = [run_device(rule, rig, targets, q, th, tl, flags, q_skip, ws)]
    if host:
        got.append(fz.fuse(rule, rig, targets, q, th, tl, flags=flags, q_skip=q_skip))
    for bk, bd, ep in got:
        assert bk.shape == want["best_kp"].shape
        assert np.array_equal(bk, want["best_kp"])
        assert np.array_equal(bd, want["best_dist"])
        if rule == 0:
            assert np.array_equal(ep, want["epi_ok"])
        else:
            assert ep is None
    return want


@pytest.mark.parametrize("rule,nbytes,masked", [(0, 32, False), (1, 32, False), (2, 32, False), (0, 16, True),
                                                (0, 64, False), (1, 64, True), (2, 16, False), (2, 32, True),
                                                (1, 16, False), (0, 32, True), (2, 64, True)])
def test_rules_and_descriptor_sizes(gpu, rule, nbytes, masked):
    rig, targets, q = make_case(seed=10 + rule, T=2, nq=150, n_per_cam=130, nbytes=nbytes, masked=masked)
    w = check(rule, rig, targets, q)
    assert (w["best_kp"] >= 0).sum() > 20
    if rule == 0:
        hit = w["best_kp"] >= 0
        assert w["epi_ok"][hit].any() and not w["epi_ok"][hit].all()


@pytest.mark.parametrize("nq,T", [(1, 1), (63, 3), (64, 1), (65, 3), (257, 7)])
def test_query_and_batch_counts(gpu, nq, T):
    rig, targets, q = make_case(seed=20 + nq, T=T, nq=nq, n_per_cam=60)
    check(0, rig, targets, q)
    check(2, rig, targets, q, host=False)


def test_batch_of_seven_equals_seven_single_calls(gpu):
    rig, targets, q = make_case(seed=31, T=7, nq=65, n_per_cam=70)
    for rule in (0, 1):
        bk, bd, ep = run_device(rule, rig, targets, q, 3.0, 64)
        for t in range(7):
            sk, sd, se = run_device(rule, rig, targets[t:t + 1], q, 3.0, 64)
            assert np.array_equal(bk[t], sk[0]) and np.array_equal(bd[t], sd[0])
            if rule == 0:
                assert np.array_equal(ep[t], se[0])
    assert (bk >= 0).sum() > 30


def test_empty_target_and_empty_camera(gpu):
    rng = np.random.default_rng(41)
    rig = make_rig(3)
    targets = [make_target(rig, rng, 80, 32, False), make_target(rig, rng, 0, 32, False),
               make_target(rig, rng, [70, 0, 70], 32, False)]
    q = make_queries(rig, targets, rng, 90, 32, False)
    for rule in (0, 1, 2):
        w = check(rule, rig, targets, q)
        assert (w["best_kp"][1] == -1).all() and (w["best_dist"][1] == INT_MAX).all()
        assert (w["best_kp"][2][:, 1] == -1).all() and (w["best_kp"][2] >= 0).any()
    # nothing at all: every target empty
    check(2, rig, [targets[1], targets[1]], q)


def test_window_of_more_than_64_cells(gpu):
    """th = 40 at the top level: radius 40 * 1.2^7 px, a window of several hundred cells."""
    rig, targets, q = make_case(seed=51, T=2, nq=40, n_per_cam=300)
    q["dist"][:, 0] = 1e-3     # ratio far above the last scale factor -> level nLevels - 1
    q["dist"][:, 1] = 1e3
    for t in targets:
        t["kp_octave"][::2] = 7
        t["kp_octave"][1::4] = 6
    w = check(0, rig, targets, q, th=40.0)
    lv = w["level"]
    assert (lv[lv >= 0] == 7).all() and (w["radius"][lv >= 0] > 140).all()
    assert max(len(c) for c in w["cand"].values()) > 64
    check(1, rig, targets, q, th=40.0, host=False)


def test_cell_of_more_than_64_keypoints(gpu):
    """200 keypoints of camera 0 inside one grid cell (cell 25, 20: centre 25 * 754 / 64, 200)."""
    rng = np.random.default_rng(61)
    rig = make_rig(3)
    targets = [make_target(rig, rng, [200, 40, 40], 32, False, cluster=(0, 25 * 754 / 64.0, 200.0))]
    grid = np_grid(targets[0]["kp_xy"], targets[0]["kp_cam"], rig["grid_params"])
    assert max(len(v) for v in grid.values()) > 64
    targets[0]["kp_octave"][:200] = 3 + np.arange(200) % 2     # so that more than 64 also pass the level test
    q = make_queries(rig, targets, rng, 80, 32, False, jitter=1.0)
    for rule in (0, 1):
        w = check(rule, rig, targets, q, th=6.0)
        assert max(len(c) for c in w["cand"].values()) > 64


def test_equal_descriptors_first_in_enumeration_order_wins(gpu):
    rig, targets, q = make_case(seed=71, T=2, nq=80, n_per_cam=350, same_desc=True)
    w = check(0, rig, targets, q, th=12.0)
    multi = [k for k, c in w["cand"].items() if len(c) >= 2]
    assert len(multi) > 10
    for key in multi:
        assert w["best_dist"][key] == 0 and w["best_kp"][key] == w["cand"][key][0][0]
    check(2, rig, targets, q, th=12.0, host=False)


@pytest.mark.parametrize("n_cams", [1, 3])
def test_camera_counts(gpu, n_cams):
    rig, targets, q = make_case(seed=81, T=2, nq=70, n_per_cam=100, n_cams=n_cams)
    for rule in (0, 2):
        w = check(rule, rig, targets, q)
        assert w["best_kp"].shape[2] == n_cams and (w["best_kp"] >= 0).any()


def test_q_skip_for_a_third_of_the_pairs(gpu):
    rig, targets, q = make_case(seed=91, T=3, nq=90, n_per_cam=90)
    skip = (np.arange(3 * 90).reshape(3, 90) % 3 == 1).astype(np.uint8)
    full = np_fuse_candidates(0, rig, targets, q, 3.0, 64)
    w = check(0, rig, targets, q, q_skip=skip)
    s = skip.astype(bool)
    assert (w["best_kp"][s] == -1).all() and (w["best_dist"][s] == INT_MAX).all() and (w["epi_ok"][s] == 0).all()
    assert np.array_equal(w["best_kp"][~s], full["best_kp"][~s]) and (full["best_kp"][s] >= 0).any()


def test_rule_1_with_use_distance(gpu):
    fz = _fz()
    rig, targets, q = make_case(seed=101, T=2, nq=120, n_per_cam=140)
    as_written = check(1, rig, targets, q, th=5.0)
    scanned = check(1, rig, targets, q, th=5.0, flags=fz.USE_DISTANCE)
    rule2 = np_fuse_candidates(2, rig, targets, q, 5.0, 64)
    assert (as_written["best_kp"] != scanned["best_kp"]).any()
    hit = as_written["best_kp"] >= 0
    assert (as_written["best_dist"][hit] == 0).all() and (scanned["best_dist"][scanned["best_kp"] >= 0] > 0).any()
    same = (as_written["level"] >= 0) == (rule2["level"] >= 0)     # where float / double dist3D agree
    assert np.array_equal(scanned["best_kp"][same], rule2["best_kp"][same])


def test_select_on_device_rows_three_targets_with_rerun(gpu):
    """A rule-0 sequence over 3 targets: the device rows of each target through mcs_fuse_select
    equal the restatement's tail on the restatement's rows; a REPLACE survivor that is a later
    query is reported, its descriptor row refreshed, and the remaining targets re-run."""
    fz = _fz()
    rig, targets, q = make_case(seed=111, T=3, nq=150, n_per_cam=130)
    nq, n_mp = 150, 400
    rng = np.random.default_rng(112)
    q_mp = rng.permutation(n_mp)[:nq].astype(np.int32)
    q_mp[rng.choice(nq, 8, replace=False)] = -1
    states = []
    for t, tg in enumerate(targets):   # slots of each target hold other queries' map points
        n_kp = len(tg["kp_xy"])
        kp_mp = np.full(n_kp, -1, np.int32)
        own = rng.choice(n_kp, n_kp // 2, replace=False)
        kp_mp[own] = rng.permutation(n_mp)[:len(own)]
        states.append(kp_mp)
    mp_bad = (rng.random(n_mp) < 0.05).astype(np.uint8)
    reruns, t0 = 0, 0
    dev_bad, ref_bad = mp_bad.copy(), mp_bad.copy()
    while t0 < 3:
        bk, bd, ep = run_device(0, rig, targets[t0:], q, 4.0, 64)
        want = np_fuse_candidates(0, rig, targets[t0:], q, 4.0, 64)
        assert want["margin"] > MARGIN
        assert np.array_equal(bk, want["best_kp"]) and np.array_equal(ep, want["epi_ok"])
        again = False
        for t in range(t0, 3):
            kp_mp = states[t]
            in_kf = np.zeros(n_mp, np.uint8)
            in_kf[kp_mp[kp_mp >= 0]] = 1
            in_kf[ref_bad != 0] = 0
            ref = np_fuse_select(0, q_mp, want["best_kp"][t - t0], want["epi_ok"][t - t0], ref_bad, in_kf, kp_mp)
            dk, di = kp_mp.copy(), in_kf.copy()
            actions, nf, req = fz.fuse_select(0, q_mp, bk[t - t0], ep[t - t0], dev_bad, di, dk)
            assert np.array_equal(actions, ref[0]) and nf == ref[1] and np.array_equal(req, ref[2])
            assert np.array_equal(dev_bad, ref[3]) and np.array_equal(di, ref[4]) and np.array_equal(dk, ref[5])
            ref_bad, states[t] = ref[3].copy(), dk
            if len(req) and t + 1 < 3:   # the survivors' descriptors change: refresh, re-run the rest
                for m in req:
                    q["desc"][np.flatnonzero(q_mp == m)] ^= np.uint8(0x10)
                reruns, t0, again = reruns + 1, t + 1, True
                break
        if not again:
            break
    assert reruns >= 1


def test_workspace_reuse_leaks_no_state(gpu):
    fz = _fz()
    a = make_case(seed=121, T=5, nq=100, n_per_cam=90)
    b = make_case(seed=122, T=2, nq=33, n_per_cam=40, nbytes=16, masked=True)
    ws = fz.Workspace(6)
    check(0, *a, ws=ws, host=False)
    check(2, *b, ws=ws, host=False)
    check(1, *a, ws=ws, host=False)
    check(0, *b, ws=ws, host=False)


def test_argument_errors(gpu):
    import mcs_amd
    import torch
    fz = _fz()
    rig, targets, q = make_case(seed=131, T=3, nq=20, n_per_cam=30)
    ts, qs, keep = fz.device_sets(fz.pack_targets(rig, targets, 32), fz.pack_queries(q, 32))

    def code(ws, rule=0, t=ts, qq=qs):
        with pytest.raises(mcs_amd.McsError) as e:
            fz.fuse_device(ws, rule, t, qq, 3.0, 64)
        return e.value.code

    assert code(fz.Workspace(2)) == mcs_amd.MCS_ERR_ARG                  # workspace too small
    ws = fz.Workspace(3)
    assert code(ws, rule=3) == mcs_amd.MCS_ERR_ARG

    def variant(**kw):
        s = fz.FuseTargets()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(ts), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    big = dict(targets[0], kp_xy=np.zeros((1 << 19, 2), np.float32), kp_octave=np.zeros(1 << 19, np.int32),
               kp_cam=np.zeros(1 << 19, np.int32), desc=np.zeros((1 << 19, 32), np.uint8), rays=np.zeros((1 << 19, 3)))
    with pytest.raises(mcs_amd.McsError) as e:          # one target of 2^19 keypoints: position field of the key
        fz.fuse(0, rig, [targets[1], big], q, 3.0, 64)
    assert e.value.code == mcs_amd.MCS_ERR_ARG and b"2^19" in mcs_amd.lib().mcs_last_error()
    assert code(ws, t=variant(bytes=24)) == mcs_amd.MCS_ERR_ARG
    assert code(ws, t=variant(n_cams=9)) == mcs_amd.MCS_ERR_ARG
    one_sided = torch.zeros((ts.n_kp_total, 32), dtype=torch.uint8, device="cuda")
    assert code(ws, t=variant(mask=one_sided.data_ptr())) == mcs_amd.MCS_ERR_ARG   # mask on one side only
    assert b"mask" in mcs_amd.lib().mcs_last_error()
    bk, bd, ep = fz.fuse_device(ws, 0, ts, qs, 3.0, 64)                  # the sets are still usable
    torch.cuda.synchronize()
    assert np.array_equal(bk.cpu().numpy(), np_fuse_candidates(0, rig, targets, q, 3.0, 64)["best_kp"])


def test_malformed_offsets_and_grids_stay_inside_the_buffers(gpu):
    """Offsets, cell ranges and cell entries are device data: the kernel clamps them, so a broken
    set gives some answer for the broken target and the right one for the others."""
    import torch
    fz = _fz()
    rig, targets, q = make_case(seed=141, T=3, nq=60, n_per_cam=60)
    pt, pq = fz.pack_targets(rig, targets, 32), fz.pack_queries(q, 32)
    good = np_fuse_candidates(2, rig, targets, q, 3.0, 64)
    pt["cell_ptr"][1, ::7] = 1 << 30
    pt["cell_ptr"][1, 3::11] = -5
    o1, o2 = int(pt["off"][1]), int(pt["off"][2])
    pt["cell_kp"][o1:o2:3] = 1 << 29
    pt["cell_kp"][o1 + 1:o2:5] = -7
    ts, qs, keep = fz.device_sets(pt, pq)
    bk, bd, _ = fz.fuse_device(None, 2, ts, qs, 3.0, 64)
    torch.cuda.synchronize()
    bk = bk.cpu().numpy()
    assert np.array_equal(bk[[0, 2]], good["best_kp"][[0, 2]])
    assert ((bk[1] >= -1) & (bk[1] < o2 - o1)).all()
    pt2 = fz.pack_targets(rig, targets, 32)
    pt2["off"] = np.array([0, 1 << 28, -3, pt2["n_kp_total"]], np.int32)
    ts, qs, keep = fz.device_sets(pt2, pq)
    bk, bd, _ = fz.fuse_device(None, 2, ts, qs, 3.0, 64)
    torch.cuda.synchronize()
    assert (bk.cpu().numpy() >= -1).all()


def test_projection_to_fuse_stays_on_device(gpu):
    """Map-point positions produced by a device operation, isInFrustum and Fuse enqueued on one
    stream with no host synchronisation in between; one synchronisation at the end."""
    import torch
    import mcs_amd
    from mcs_amd import synth
    fz = _fz()
    rng = np.random.default_rng(151)
    rig = make_rig(3)
    pose = np.array([0.011, -0.023, 0.017, 0.03, -0.04, 0.02])
    targets = [make_target(rig, rng, 110, 32, False, pose=pose), make_target(rig, rng, 110, 32, False)]
    q = make_queries(rig, targets, rng, 130, 32, False)
    nq = 130
    perm = rng.permutation(nq)
    ts, qs, keep = fz.device_sets(fz.pack_targets(rig, targets, 32), fz.pack_queries(q, 32))
    ws = fz.Workspace(2)
    shuffled = torch.from_numpy(q["pos"][perm]).cuda()
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    d = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda() for k, v in dict(
        pose=pose, mc=np.array(synth.LAFIDA_MC), cam=rig["cam"], nrm=q["rays"], dist=q["dist"], scale=rig["scale"]).items()}
    mirror = keep[0]["mirror"]
    iv = torch.zeros((nq, 3), dtype=torch.uint8, device="cuda")
    pj = torch.zeros((nq, 3, 2), dtype=torch.float64, device="cuda")
    lv = torch.zeros((nq, 3), dtype=torch.int32, device="cuda")
    vc = torch.zeros((nq, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    pos = shuffled[inv].contiguous()                  # device op: the positions exist only on the device
    qs.pos = pos.data_ptr()
    rc = mcs_amd.lib().mcs_is_in_frustum_device(
        d["pose"].data_ptr(), d["mc"].data_ptr(), d["cam"].data_ptr(), 3, mirror.data_ptr(), 754, 480,
        pos.data_ptr(), d["nrm"].data_ptr(), d["dist"].data_ptr(), nq, d["scale"].data_ptr(), 8,
        iv.data_ptr(), pj.data_ptr(), lv.data_ptr(), vc.data_ptr(), stream)
    assert rc == 0
    bk, bd, ep = fz.fuse_device(ws, 2, ts, qs, 3.0, 64)
    torch.cuda.synchronize()
    want = np_fuse_candidates(2, rig, targets, q, 3.0, 64)
    assert np.array_equal(bk.cpu().numpy(), want["best_kp"]) and np.array_equal(bd.cpu().numpy(), want["best_dist"])
    seen = iv.cpu().numpy() == 1
    assert seen.sum() > 30
    np.testing.assert_allclose(pj.cpu().numpy()[seen], np.stack([want["u"][0], want["v"][0]], -1)[seen],
                               rtol=0, atol=1e-9)


def test_batch_above_2_pow_19_keypoints_in_total(gpu):
    """The 2^19 bound is per target: 90 targets of about 6000 keypoints (SearchInNeighbors' upper
    count, above 2^19 keypoints in total) in one call of each entry.  Rows of the first, a middle
    and the last target against the restatement; the host and the device entry agree on all."""
    fz = _fz()
    rng = np.random.default_rng(181)
    rig = make_rig(3)
    base = [make_target(rig, rng, 2000, 32, False) for _ in range(3)]
    targets = [dict(base[k % 3], m_t=fz.cayley2hom(np.concatenate([rng.uniform(-0.03, 0.03, 3),
                                                                    rng.uniform(-0.05, 0.05, 3)]))) for k in range(90)]
    assert sum(len(t["kp_xy"]) for t in targets) > (1 << 19)
    q = make_queries(rig, base, rng, 12, 32, False)
    bk, bd, ep = run_device(0, rig, targets, q, 3.0, 64)
    hk, hd, he = fz.fuse(0, rig, targets, q, 3.0, 64)
    assert np.array_equal(bk, hk) and np.array_equal(bd, hd) and np.array_equal(ep, he)
    for t in (0, 44, 89):
        w = np_fuse_candidates(0, rig, targets[t:t + 1], q, 3.0, 64)
        assert w["margin"] > MARGIN
        assert np.array_equal(bk[t], w["best_kp"][0]) and np.array_equal(bd[t], w["best_dist"][0])
        assert np.array_equal(ep[t], w["epi_ok"][0])
    assert (bk >= 0).sum() > 20


@pytest.mark.parametrize("name", ["r0", "r1", "r2"])
def test_cpp_adapter_reproduces_the_text(gpu, tmp_path, name):
    """tests/cpp/fuse_demo.cpp: mcs::Fuse over a map stand-in on the fixture's 3-target scenarios
    (the re-run path, the same point at two keypoints, a Sim3 of scale 1.7 through FuseSim3ToMt)
    gives the reference text's nFused, its ordered AddObservation / Replace calls and its end
    state, and refreshes the descriptors the restated sequence refreshes."""
    import subprocess
    s = load_scenario(name)
    rule, rig, targets, q = s["rule"], s["rig"], s["targets"], s["q"]
    n_mp = len(s["mp_bad"])
    d = tmp_path / "in"
    d.mkdir()

    def put(fname, a, dt):
        np.ascontiguousarray(a, dt).tofile(str(d / (fname + ".bin")))
    put("dims", [3, 754, 480, s["T"], n_mp], np.int32)
    for k, dt in (("m_c", np.float64), ("cam", np.float64), ("mirror", np.uint8), ("grid_params", np.float64),
                  ("scale", np.float64)):
        put(k, rig[k], dt)
    for t, tg in enumerate(targets):
        put("t%d_scw" % t, s["scw"][t], np.float64)
        for k, dt in (("kp_xy", np.float32), ("kp_octave", np.int32), ("kp_cam", np.int32), ("desc", np.uint8),
                      ("rays", np.float64), ("m_t", np.float64)):
            put("t%d_%s" % (t, k), tg[k], dt)
        put("t%d_kp_mp" % t, s["kp_mp"][t], np.int32)
        put("t%d_in_kf" % t, s["in_kf"][t], np.uint8)
    for k, dt in (("pos", np.float64), ("dist", np.float64), ("desc", np.uint8), ("rays", np.float64),
                  ("m_t", np.float64)):
        put("q_" + k, q[k], dt)
    put("q_mp", s["q_mp"], np.int32)
    put("mp_bad", s["mp_bad"], np.uint8)
    put("new_desc", s["new_desc"], np.uint8)
    want = np_fuse_sequence(rule, rig, targets, q, s["q_mp"], s["mp_bad"], s["in_kf"], s["kp_mp"], s["new_desc"],
                            s["th"], s["th_low"])
    out = subprocess.run([build_fuse_demo(tmp_path), str(d), str(rule), "32", repr(s["th"]), str(s["th_low"])],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    m_t = [np.array(ln[1:], np.float64).reshape(4, 4) for ln in lines if ln[0] == "m_t"]
    for t in range(s["T"]):
        assert np.array_equal(m_t[t], targets[t]["m_t"])        # rule 2: FuseSim3ToMt bit for bit
    actions = [tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "action"]
    assert [(t, kind, int(s["q_mp"][i]), k, other) for t, kind, i, k, other in actions] == s["actions"]
    assert [int(ln[2]) for ln in lines if ln[0] == "nfused"] == s["n_fused"]
    assert [int(ln[1]) for ln in lines if ln[0] == "refresh"] == want[2]
    assert [int(x) for ln in lines if ln[0] == "bad" for x in ln[1:]] == s["end"][-1][1].tolist()
    last = [[int(x) for x in ln[2:]] for ln in lines if ln[0] == "slots" and int(ln[1]) == s["T"] - 1][0]
    assert last == s["end"][-1][0].tolist()
    for t in range(s["T"]):          # the other keyframes after the whole call: the restated sequence's
        got = [[int(x) for x in ln[2:]] for ln in lines if ln[0] == "slots" and int(ln[1]) == t][0]
        assert got == want[4][t].tolist()
    if rule == 0:
        assert want[2], "the scenario must take the re-run path"


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_reference_text_scenarios(gpu, name, entry):
    """tests/golden/fuse_ref.npz: the device rows (mcs_fuse / mcs_fuse_device) equal the
    restatement's on every triple, which reproduces the text's windows
    (tests/test_fuse_ref.py), and the device rows fed through mcs_fuse_select over all targets,
    with the re-run after a refreshed descriptor, give the text's nFused, its ordered
    AddObservation / Replace calls and its end state."""
    fz = _fz()
    s = load_scenario(name)

    def device_candidates(rule, rig, targets, q, th, tl, q_skip=None):
        want = np_fuse_candidates(rule, rig, targets, q, th, tl, q_skip=q_skip)
        if entry == "host":
            bk, bd, ep = fz.fuse(rule, rig, targets, q, th, tl, q_skip=q_skip)
        else:
            bk, bd, ep = run_device(rule, rig, targets, q, th, tl, q_skip=q_skip)
        assert np.array_equal(bk, want["best_kp"]) and np.array_equal(bd, want["best_dist"])
        if rule == 0:
            assert np.array_equal(ep, want["epi_ok"])
        return dict(best_kp=bk, epi_ok=ep, margin=want["margin"])

    def lib_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp):
        bad, inkf, slots = mp_bad.copy(), mp_in_kf.copy(), kp_mp.copy()
        a, nf, req = fz.fuse_select(rule, q_mp, best_kp, epi_ok, bad, inkf, slots)
        return a, nf, req, bad, inkf, slots
    got = np_fuse_sequence(s["rule"], s["rig"], s["targets"], s["q"], s["q_mp"], s["mp_bad"], s["in_kf"], s["kp_mp"],
                           s["new_desc"], s["th"], s["th_low"], select=lib_select, candidates=device_candidates)
    check_sequence_against_text(s, got)
