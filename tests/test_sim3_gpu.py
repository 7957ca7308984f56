"""cORBmatcher::SearchBySim3 on the device (mcs_search_by_sim3, mcs_search_by_sim3_device;
reference src/cORBmatcher.cpp:1721-1988) against the NumPy restatement of tests/test_sim3_ref.py,
at the kernels' edge shapes.

All comparisons are exact, on vnMatch1, vnMatch2, the agreed matches and nFound of every candidate,
and each is made for the device entry and for the host entry.  The inputs keep the 1e-9 margin of
tests/test_sim3_ref.py on every decision that depends on atan (asserted on each input first), so a
last-ulp difference between the device's atan and libm's cannot flip one; everything else is the
same correctly rounded operations in the same order on both sides.  Every randomised case must
show more than 20 mutual matches and a failed agreement in the restatement, or it fails as vacuous."""
import ctypes

import numpy as np
import pytest

from tests.test_fuse_ref import MARGIN, make_rig
from tests.test_sim3_ref import (SCENARIOS, coverage, expected_matches12, finish_kf1, load_scenario, make_candidate,
                                 make_case, make_kf1, np_search_batch, project_rig, th_high)

pytestmark = pytest.mark.gpu
GUARD = 64                    # int32 elements around every output buffer of the guarded runs
COUNT_SEEDS = {(1, 1): 41, (21, 3): 45, (22, 3): 43, (22, 7): 44, (43, 1): 45, (86, 7): 46}


def _sm():
    from mcs_amd import sim3_match
    return sim3_match


def run_device(case, th, thh, ws=None, packed=None, guard=False):
    """-> (match1 [T, n1], match2 list per candidate, matches12 [T, n1], n_found [T])."""
    import torch
    sm = _sm()
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = case
    nbytes = kf1["desc"].shape[1]
    pk1, pp1, pk2, pp2, A1, A2, S, R, Tt = packed or sm.pack_call(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12,
                                                                  nbytes, True)
    k1, p1, keep1 = sm.device_sets(pk1, pp1)
    k2, p2, keep2 = sm.device_sets(pk2, pp2)
    dev = [torch.from_numpy(x).cuda() for x in (A1, A2, S, R, Tt)]
    T, n1, n2 = len(kf2s), pk1["n_kp_total"], pk2["n_kp_total"]
    out = None
    if guard:
        bufs = [torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in (T * n1, n2, T * n1, T)]
        out = (bufs[0][GUARD:GUARD + T * n1].view(T, n1), bufs[1][GUARD:GUARD + n2], bufs[2][GUARD:GUARD + T * n1].view(T, n1),
               bufs[3][GUARD:GUARD + T])
    m1, m2, m12, nf = sm.search_by_sim3_device(ws, k1, p1, k2, p2, *dev, th, thh, out=out)
    torch.cuda.synchronize()
    if guard:
        for b, n in zip(bufs, (T * n1, n2, T * n1, T)):
            b = b.cpu().numpy()
            assert (b[:GUARD] == 0x5A5A5A5A).all() and (b[GUARD + n:] == 0x5A5A5A5A).all()
    off = pk2["off"]
    m2 = m2.cpu().numpy()
    return m1.cpu().numpy(), [m2[off[k]:off[k + 1]] for k in range(T)], m12.cpu().numpy(), nf.cpu().numpy()


def same(got, want):
    m1, m2, m12, nf = got
    assert m1.shape == want["match1"].shape
    assert np.array_equal(m1, want["match1"])
    assert len(m2) == len(want["match2"]) and all(np.array_equal(a, b) for a, b in zip(m2, want["match2"]))
    assert np.array_equal(m12, want["matches12"])
    assert np.array_equal(nf, want["n_found"])


def check(case, th=10.0, thh=None, ws=None, host=True, vacuous_ok=False):
    """Device entry and host entry == restatement -> the restatement."""
    sm = _sm()
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = case
    thh = th_high(kf1["desc"].shape[1], kf1.get("mask") is not None) if thh is None else thh
    want = np_search_batch(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, th, thh)
    assert want["margin"] > MARGIN
    if not vacuous_ok:
        found, failed = coverage(want)
        assert found > 20 and failed >= 1, (found, failed)
    same(run_device(case, th, thh, ws), want)
    if host:
        same(sm.search_by_sim3(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, th, thh), want)
    return want


@pytest.mark.parametrize("nbytes,masked", [(16, False), (16, True), (32, False), (32, True), (64, False), (64, True)])
def test_descriptor_sizes(gpu, nbytes, masked):
    check(make_case(seed=10 + nbytes + masked, T=2, n_per_cam=130, nbytes=nbytes, masked=masked))


@pytest.mark.parametrize("s12", [0.6, 1.0, 1.7])
def test_sim3_scales(gpu, s12):
    check(make_case(seed=30, T=2, n_per_cam=130, s12=s12))


@pytest.mark.parametrize("n_per_cam,T", [(1, 1), (21, 3), (22, 3), (22, 7), (43, 1), (86, 7)])
def test_keypoint_and_batch_counts(gpu, n_per_cam, T):
    """n1 around 1, 63, 64 / 65 and 257 over 3 cameras (make_target drops a keypoint outside the
    image now and then): the wave and block boundaries of the agreement kernel.  Three keypoints
    cannot give 20 matches; every other shape must."""
    case = make_case(seed=COUNT_SEEDS[n_per_cam, T], T=T, n_per_cam=n_per_cam, p_active=0.97, paired=0.95)
    check(case, vacuous_ok=n_per_cam == 1)


def test_batch_of_seven_equals_seven_single_calls(gpu):
    """The rows of active1 differ per candidate: a kernel that read row 0 for all would fail."""
    case = make_case(seed=51, T=7, n_per_cam=70)
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = case
    assert all((a1[t] != a1[0]).any() for t in range(1, 7))
    want = check(case)
    m1, m2, m12, nf = run_device(case, 10.0, 96)
    for t in range(7):
        one = (rig, kf1, pts1, kf2s[t:t + 1], pts2s[t:t + 1], a1[t:t + 1], a2s[t:t + 1], s12[t:t + 1], R12[t:t + 1],
               t12[t:t + 1])
        s1, s2, s12_, sf = run_device(one, 10.0, 96)
        assert np.array_equal(m1[t], s1[0]) and np.array_equal(m2[t], s2[0]) and np.array_equal(m12[t], s12_[0])
        assert nf[t] == sf[0]
    # with candidate 0's flags for everybody the result differs
    a1_wrong = np.repeat(a1[:1], 7, axis=0)
    other = np_search_batch(rig, kf1, pts1, kf2s, pts2s, a1_wrong, a2s, s12, R12, t12, 10.0, 96)
    assert not np.array_equal(other["match1"], want["match1"])


def test_empty_cases(gpu):
    rng = np.random.default_rng(61)
    rig = make_rig(3)
    kf1, pts1 = make_kf1(rig, rng, 80, 32, False)
    full = make_candidate(rig, rng, kf1, pts1, 80, 32, False, 1.0)
    empty = make_candidate(rig, rng, kf1, pts1, 0, 32, False, 1.0)
    holed = make_candidate(rig, rng, kf1, pts1, [70, 0, 70], 32, False, 1.0)
    finish_kf1(pts1, rng)
    n1 = len(kf1["kp_xy"])

    def case(cands, a1=None):
        a1 = np.ones((len(cands), n1), np.uint8) if a1 is None else a1
        return (rig, kf1, pts1, [c[0] for c in cands], [c[1] for c in cands], a1,
                [np.ones(len(c[0]["kp_xy"]), np.uint8) for c in cands], np.array([c[2] for c in cands]),
                np.stack([c[3] for c in cands]), np.stack([c[4] for c in cands]))
    w = check(case([full, empty, holed]))
    assert (w["match1"][1] == -1).all() and w["n_found"][1] == 0 and len(w["match2"][1]) == 0
    assert w["n_found"][0] > 0 and w["n_found"][2] > 0
    cam1 = kf1["kp_cam"] == 1
    assert (w["match1"][2][cam1] == -1).all()                  # no keypoints of camera 1 in that candidate
    # KF1 with no active keypoint: nothing agrees, direction 2 still matches
    w = check(case([full, holed], a1=np.zeros((2, n1), np.uint8)), vacuous_ok=True)
    assert (w["match1"] == -1).all() and (w["matches12"] == -1).all() and (w["n_found"] == 0).all()
    assert (w["match2"][0] >= 0).any()
    # all candidates empty
    w = check(case([empty, empty]), vacuous_ok=True)
    assert (w["match1"] == -1).all() and (w["n_found"] == 0).all()
    # an empty KF1
    kf0, pts0 = make_kf1(rig, rng, 0, 32, False)
    c0 = (rig, kf0, pts0, [full[0]], [full[1]], np.zeros((1, 0), np.uint8), [np.ones(len(full[0]["kp_xy"]), np.uint8)],
          np.array([1.0]), full[3][None], full[4][None])
    w = check(c0, vacuous_ok=True)
    assert w["match1"].shape == (1, 0) and (w["match2"][0] == -1).all()


def test_window_of_more_than_64_cells(gpu):
    """th = 40 at the top level: radius 40 * 1.2^7 px, a window of several hundred cells."""
    case = make_case(seed=71, T=2, n_per_cam=300)
    rig, kf1, pts1, kf2s, pts2s = case[:5]
    for pts in [pts1] + pts2s:
        pts["dist"][:, 0] = 1e-3          # ratio far above the last scale factor -> level nLevels - 1
        pts["dist"][:, 1] = 1e3
    for kf in [kf1] + kf2s:
        kf["kp_octave"][::2] = 7
        kf["kp_octave"][1::4] = 6
    w = check(case, th=40.0)
    lv = [g[5] for r in w["per"] for g in r["gfa1"] + r["gfa2"]]
    assert lv and all(x == 7 for x in lv)
    assert max(len(g[6]) for r in w["per"] for g in r["gfa1"] + r["gfa2"]) > 64


def test_cell_of_more_than_64_keypoints(gpu):
    """200 keypoints of camera 2 inside one grid cell of the candidate, more than 64 of which pass
    the level test: the walk takes the cell in several rounds of 64."""
    from tests.test_fuse_ref import np_grid
    rng = np.random.default_rng(81)
    rig = make_rig(3)
    kf1, pts1 = make_kf1(rig, rng, 90, 32, False)
    kf2, pts2, s, R, t = make_candidate(rig, rng, kf1, pts1, [90, 90, 260], 32, False, 1.0)
    finish_kf1(pts1, rng)
    c2 = np.flatnonzero(kf2["kp_cam"] == 2)
    cx, cy = 30 * 754 / 64.0, 230.0
    clu = c2[-200:]
    kf2["kp_xy"][clu] = (np.array([cx, cy]) + rng.uniform(-2.0, 2.0, (200, 2))).astype(np.float32)
    kf2["kp_octave"][clu] = 3 + np.arange(200) % 2
    grid = np_grid(kf2["kp_xy"], kf2["kp_cam"], rig["grid_params"])
    assert max(len(v) for v in grid.values()) > 64
    # KF1 points of camera 2 that land on the cluster, at a level that admits octaves 3 and 4
    Mc2 = np.asarray(rig["m_c"][2])
    from mcs_amd import synth
    ray = np.array(synth.img_to_world(rig["cams"][2], np.float64(cx), np.float64(cy)))
    p2 = Mc2[:3, :3] @ (ray * 2.0) + Mc2[:3, 3]
    assert p2[2] > 0
    for i in np.flatnonzero(kf1["kp_cam"] == 2)[:30]:
        p2j = p2 + rng.normal(0, 0.004, 3)
        p1 = s * (R @ p2j) + t
        pts1["pos"][i] = kf1["m_t"][:3, :3] @ p1 + kf1["m_t"][:3, 3]
        d = project_rig(rig, 2, p2j)[2]
        pts1["dist"][i] = (d / (0.8 * 0.95 * rig["scale"][4]), d * 4.0)
        pts1["desc"][i] = kf2["desc"][clu[int(rng.integers(200))]]
    n1, n2 = len(kf1["kp_xy"]), len(kf2["kp_xy"])
    case = (rig, kf1, pts1, [kf2], [pts2], np.ones((1, n1), np.uint8), [np.ones(n2, np.uint8)], np.array([s]), R[None], t[None])
    w = check(case, vacuous_ok=True)
    passing = [sum(1 for k in g[6] if kf2["kp_octave"][k] in (g[5] - 1, g[5])) for g in w["per"][0]["gfa1"]]
    assert max(passing) > 64
    assert (np.isin(w["match1"][0], clu)).sum() >= 10


def test_constant_descriptor_first_in_enumeration_order_wins(gpu):
    case = make_case(seed=91, T=2, n_per_cam=350, same_desc=True)
    w = check(case, th=14.0)
    n_multi = 0
    for t, r in enumerate(w["per"]):
        for d, gfa, to, m in ((1, r["gfa1"], case[3][t], r["match1"]), (2, r["gfa2"], case[1], r["match2"])):
            for i, c, u, v, rad, lv, lst in gfa:
                ok = [k for k in lst if to["kp_octave"][k] in (lv - 1, lv)]
                assert m[i] == (ok[0] if ok else -1)
                n_multi += len(ok) >= 2
    assert n_multi > 20


def test_only_the_keypoints_own_camera_is_searched(gpu):
    """A KF1 keypoint of camera 0 whose point projects inside camera 2 of the candidate (right on a
    keypoint with the same descriptor) but outside camera 0: no match."""
    from mcs_amd import synth
    case = make_case(seed=101, T=1, n_per_cam=100)
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = case
    kf2 = kf2s[0]
    Mc2 = np.asarray(rig["m_c"][2])
    done = 0
    for k2 in np.flatnonzero(kf2["kp_cam"] == 2):
        ray = np.array(synth.img_to_world(rig["cams"][2], np.float64(kf2["kp_xy"][k2, 0]), np.float64(kf2["kp_xy"][k2, 1])))
        p2 = Mc2[:3, :3] @ (ray * 2.0) + Mc2[:3, 3]
        u0, v0, _ = project_rig(rig, 0, p2)
        inside0 = 0 < round(u0) < 754 and 0 < round(v0) < 480 and rig["mirror"][0][round(v0), round(u0)] > 0
        if p2[2] <= 0.1 or inside0 or kf2["kp_octave"][k2] < 1:      # at level 0 the ratio below would be under 1
            continue
        i = int(np.flatnonzero(kf1["kp_cam"] == 0)[done])
        p1 = s12[0] * (R12[0] @ p2) + t12[0]
        pts1["pos"][i] = kf1["m_t"][:3, :3] @ p1 + kf1["m_t"][:3, 3]
        d = project_rig(rig, 2, p2)[2]
        lvl = min(int(kf2["kp_octave"][k2]), 7)
        pts1["dist"][i] = (d / (0.8 * 0.95 * rig["scale"][lvl]), d * 4.0)
        pts1["desc"][i] = kf2["desc"][k2]
        a1[0, i] = 1
        # had the keypoint been one of camera 2, it would have matched k2
        alt = dict(kf1, kp_cam=kf1["kp_cam"].copy())
        alt["kp_cam"][i] = 2
        r = np_search_batch(rig, alt, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, 10.0, 96)
        assert r["match1"][0, i] == k2
        done += 1
        if done == 3:
            break
    assert done == 3
    w = check(case)
    assert (w["match1"][0, np.flatnonzero(kf1["kp_cam"] == 0)[:3]] == -1).all()


@pytest.mark.parametrize("name", SCENARIOS)
def test_reference_text_scenarios(gpu, name):
    """tests/golden/sim3_ref.npz through both entries: vnMatch1, vnMatch2, nFound and vpMatches12
    after the call are the reference text's."""
    sm = _sm()
    s = load_scenario(name)
    case = (s["rig"], s["kf1"], s["pts1"], [s["kf2"]], [s["pts2"]], s["active1"][None], [s["active2"]], np.array([s["s12"]]),
            s["R12"][None], s["t12"][None])
    for m1, m2, m12, nf in (run_device(case, s["th"], s["th_high"]),
                            sm.search_by_sim3(*case, s["th"], s["th_high"])):
        assert np.array_equal(m1[0], s["match1"]) and np.array_equal(m2[0], s["match2"])
        assert nf[0] == s["n_found"]
        assert np.array_equal(expected_matches12(s, m12[0]), s["matches12_out"])


def test_malformed_cameras_and_offsets_stay_inside_the_buffers(gpu):
    """kp_cam and off are device data: the kernel clamps them.  A keypoint whose camera is -1 or
    n_cams never matches, a decreasing offset gives -1 for what it breaks, the run completes and the
    guard regions around every output buffer are intact."""
    sm = _sm()
    case = make_case(seed=111, T=3, n_per_cam=60)
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = case
    good = np_search_batch(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, 10.0, 96)
    packed = list(sm.pack_call(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, 32, True))
    hit1 = np.flatnonzero(good["match1"][0] >= 0)
    hit2 = np.flatnonzero(good["match2"][1] >= 0)
    packed[0]["kp_cam"][hit1[0]], packed[0]["kp_cam"][hit1[1]] = -1, 3
    o1 = int(packed[2]["off"][1])
    packed[2]["kp_cam"][o1 + hit2[0]], packed[2]["kp_cam"][o1 + hit2[1]] = 3, -1
    m1, m2, m12, nf = run_device(case, 10.0, 96, packed=packed, guard=True)
    assert (m1[:, hit1[:2]] == -1).all() and (m12[:, hit1[:2]] == -1).all()
    assert (m2[1][hit2[:2]] == -1).all()
    keep = np.ones(len(kf1["kp_xy"]), bool)
    keep[hit1[:2]] = False
    assert np.array_equal(m1[:, keep], good["match1"][:, keep])
    packed = list(sm.pack_call(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, 32, True))
    n2 = packed[2]["n_kp_total"]
    packed[2]["off"] = np.array([0, 1 << 28, -3, n2], np.int32)
    m1, m2, m12, nf = run_device(case, 10.0, 96, packed=packed, guard=True)
    m1, m12, nf = m1.reshape(3, -1), m12.reshape(3, -1), nf.reshape(3)
    assert ((m1 >= -1) & (m1 < n2)).all() and ((m12 >= -1) & (m12 < n2)).all()
    assert ((nf >= 0) & (nf <= len(kf1["kp_xy"]))).all()
    # clamped, candidate 0 starts at 0 (its own grid still addresses its own keypoints alone) and
    # candidate 1 owns nothing
    assert np.array_equal(m1[0], good["match1"][0]) and (m1[1] == -1).all() and nf[1] == 0


def test_stream_ordered_with_a_workspace(gpu):
    """Two calls back to back on a non-default stream with one workspace, no synchronisation in
    between, vnMatch1 / vnMatch2 kept in the workspace (NULL outputs)."""
    import torch
    sm = _sm()
    a = make_case(seed=121, T=3, n_per_cam=70)
    b = make_case(seed=122, T=2, n_per_cam=40, nbytes=16, masked=True)
    wa = np_search_batch(*a, 10.0, 96)
    wb = np_search_batch(*b, 10.0, 24)
    assert min(wa["margin"], wb["margin"]) > MARGIN and coverage(wa)[0] > 20 and coverage(wb)[0] > 20
    ws = sm.Workspace(3, 256)
    st = torch.cuda.Stream()
    sets = []
    for case, nb in ((a, 32), (b, 16)):
        pk1, pp1, pk2, pp2, A1, A2, S, R, Tt = sm.pack_call(*case, nb, True)
        k1, p1, keep1 = sm.device_sets(pk1, pp1)
        k2, p2, keep2 = sm.device_sets(pk2, pp2)
        T, n1 = pk2["n_targets"], pk1["n_kp_total"]
        sets.append((k1, p1, k2, p2, [torch.from_numpy(x).cuda() for x in (A1, A2, S, R, Tt)], keep1, keep2,
                     (None, None, torch.empty((T, n1), dtype=torch.int32, device="cuda"),
                      torch.empty((T,), dtype=torch.int32, device="cuda"))))
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for (k1, p1, k2, p2, dev, _, _, out), thh in zip(sets, (96, 24)):
            sm.search_by_sim3_device(ws, k1, p1, k2, p2, *dev, 10.0, thh, out=out)
    st.synchronize()
    for s_, w in zip(sets, (wa, wb)):
        assert np.array_equal(s_[7][2].cpu().numpy(), w["matches12"]) and np.array_equal(s_[7][3].cpu().numpy(), w["n_found"])
    ws.close()


def test_argument_errors_of_the_device_entry(gpu):
    import mcs_amd
    import torch
    sm = _sm()
    case = make_case(seed=131, T=3, n_per_cam=30)
    pk1, pp1, pk2, pp2, A1, A2, S, R, Tt = sm.pack_call(*case, 32, True)
    k1, p1, keep1 = sm.device_sets(pk1, pp1)
    k2, p2, keep2 = sm.device_sets(pk2, pp2)
    dev = [torch.from_numpy(x).cuda() for x in (A1, A2, S, R, Tt)]

    def code(ws, k1=k1, p1=p1, k2=k2, p2=p2):
        with pytest.raises(mcs_amd.McsError) as e:
            sm.search_by_sim3_device(ws, k1, p1, k2, p2, *dev, 10.0, 96)
        return e.value.code

    def variant(src, **kw):
        s = type(src)()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(src), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    assert code(sm.Workspace(2, 256)) == mcs_amd.MCS_ERR_ARG             # more candidates than the workspace
    assert code(sm.Workspace(3, 50)) == mcs_amd.MCS_ERR_ARG              # more keypoints than the workspace
    ws = sm.Workspace(3, 256)
    assert code(ws, k1=variant(k1, bytes=24), k2=variant(k2, bytes=24)) == mcs_amd.MCS_ERR_ARG
    assert code(ws, k1=variant(k1, n_cams=9), k2=variant(k2, n_cams=9)) == mcs_amd.MCS_ERR_ARG
    assert code(ws, k1=variant(k1, mask=k1.desc)) == mcs_amd.MCS_ERR_ARG
    assert b"mask" in mcs_amd.lib().mcs_last_error()
    assert code(ws, k1=variant(k1, n_targets=2)) == mcs_amd.MCS_ERR_ARG
    assert code(ws, k2=variant(k2, n_levels=7)) == mcs_amd.MCS_ERR_ARG
    assert code(ws, k2=variant(k2, cell_ptr=None)) == mcs_amd.MCS_ERR_ARG
    want = np_search_batch(*case, 10.0, 96)                               # the sets are still usable
    m1, m2, m12, nf = sm.search_by_sim3_device(ws, k1, p1, k2, p2, *dev, 10.0, 96)
    torch.cuda.synchronize()
    assert np.array_equal(m12.cpu().numpy(), want["matches12"]) and np.array_equal(nf.cpu().numpy(), want["n_found"])
