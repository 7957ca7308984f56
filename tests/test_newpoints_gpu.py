"""CreateNewMapPoints on the device (include/mcs_newpoints.h) against the restatement of
tests/test_newpoints_ref.py, which newpoints_ref.npz pins to the reference text.

Verdicts are compared outside the unsure rows (a quantity within relative MARGIN of its threshold,
or the two 2 x 2 inverse forms disagreeing); positions, normals and distances to TOL_X = 10 x the
measured spread between the two inverse forms; indices, order, descriptor and mask bytes and the
has-map-point flags exactly.  Every expected result is computed once (gpu_case / loop_case) and
shared.
"""
import subprocess

import numpy as np
import pytest

from tests.test_newpoints_ref import (CREATED, EPI_THRESH, GPU_CASES, LOOP_KF2_FIRST, LOOP_SKIP, TOL_X, build_demo,
                                      gpu_case, loop_case, th_low)

pytestmark = pytest.mark.gpu
GUARD = 0x5A


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(got, want):
    if not len(want):
        assert not len(got)
        return 0.0
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    return float((np.abs(got - want).max(1) / np.abs(want).max(1)).max())


def check_points(got, want, n, masked):
    """got: dict of arrays (the first n rows used), want: the restatement's points."""
    assert n == len(want["kp1"])
    assert np.array_equal(got["kp1"][:n], want["kp1"]) and np.array_equal(got["kp2"][:n], want["kp2"])
    assert (np.diff(got["kp1"][:n]) > 0).all()                      # idx1 order
    for k in ("pos", "normal", "min_dist", "max_dist"):
        assert _rel(got[k][:n], want[k]) <= TOL_X, k
    assert np.array_equal(got["desc"][:n], want["desc"])
    if masked:
        assert np.array_equal(got["mask"][:n], want["mask"])


def run_pair(c, cap=None, ws=None, guard=0):
    """The pair entry on one case -> (count, outputs as numpy, verdict, has1, has2)."""
    import torch
    from mcs_amd import fuse, new_points as npz
    kf1, kf2 = c["kf1"], c["kf2"]
    n1, nb = len(kf1["kp_xy"]), kf1["desc"].shape[1]
    masked = kf1["mask"] is not None
    ks, keep = npz.device_set(fuse.pack_targets(c["rig"], [kf1, kf2], nb, False))
    ws = ws or npz.Workspace(max(n1, 1))
    cap = n1 if cap is None else cap
    out, ot = npz.new_out(cap + guard, nb, masked, fill=GUARD)
    out.cap = cap
    ot["count"].zero_()
    m12, h1, h2 = _dev(c["matches12"]), _dev(kf1["has_mp"]), _dev(kf2["has_mp"])
    vd = torch.full((max(n1, 1),), 9, dtype=torch.uint8, device="cuda")
    npz.pair_device(ws, ks, 0, 1, n1, 7, m12, c["kf2_first"], h1, h2, vd, out)
    torch.cuda.synchronize()
    return int(ot["count"].item()), {k: t.cpu().numpy() for k, t in ot.items()}, vd.cpu().numpy()[:n1], h1.cpu().numpy(), h2.cpu().numpy()


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_pair_entry_equals_the_restatement(gpu, name):
    c = gpu_case(name)
    w = c["want"]
    count, got, verdict, h1, h2 = run_pair(c)
    sure = ~w["unsure"]
    assert np.array_equal(verdict[sure], w["verdict"][sure])
    assert (verdict == CREATED).sum() == count
    masked = c["kf1"]["mask"] is not None
    # an unsure row may go either way on the device: the points of the sure rows are compared
    keep_d, keep_w = sure[got["kp1"][:count]], sure[w["kp1"]]
    assert (np.diff(got["kp1"][:count]) > 0).all()
    keys = ("kp1", "kp2", "pos", "normal", "min_dist", "max_dist", "desc") + (("mask",) if masked else ())
    check_points({k: got[k][:count][keep_d] for k in keys}, {k: w[k][keep_w] for k in keys}, int(keep_d.sum()), masked)
    assert (got["neighbour"][:count] == 7).all()
    e1, e2 = c["kf1"]["has_mp"].copy(), c["kf2"]["has_mp"].copy()
    e1[got["kp1"][:count]] = 1
    e2[got["kp2"][:count]] = 1
    assert np.array_equal(h1, e1) and np.array_equal(h2, e2)      # set at the created pairs and nowhere else


def test_repeated_call_on_one_workspace(gpu):
    """Two calls back to back on one workspace and stream, no synchronisation between them, outputs
    in separate buffers: identical results."""
    import torch
    from mcs_amd import fuse, new_points as npz
    c = gpu_case("c3x120")
    kf1, kf2 = c["kf1"], c["kf2"]
    n1, nb = len(kf1["kp_xy"]), 32
    ks, keep = npz.device_set(fuse.pack_targets(c["rig"], [kf1, kf2], nb, False))
    ws = npz.Workspace(n1)
    m12 = _dev(c["matches12"])
    runs = []
    for _ in range(2):
        out, ot = npz.new_out(n1, nb, False)
        h1, h2 = _dev(kf1["has_mp"]), _dev(kf2["has_mp"])
        vd = torch.zeros(n1, dtype=torch.uint8, device="cuda")
        runs.append((out, ot, h1, h2, vd))
    for out, ot, h1, h2, vd in runs:
        npz.pair_device(ws, ks, 0, 1, n1, 0, m12, c["kf2_first"], h1, h2, vd, out)
    torch.cuda.synchronize()
    a, b = runs
    assert int(a[1]["count"].item()) == len(c["want"]["kp1"])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_capacity_is_clamped_and_reported(gpu):
    """cap below the number created: count is the true number, the first cap rows are right, the
    guard rows behind them are untouched; the host entry returns MCS_ERR_CAPACITY."""
    c = gpu_case("c3x120")
    w = c["want"]
    total, cap = len(w["kp1"]), 37
    assert total > cap + 10
    count, got, verdict, h1, h2 = run_pair(c, cap=cap, guard=16)
    assert count == total
    first = {k: (v[:cap] if v is not None else None) for k, v in w.items() if k in ("kp1", "kp2", "pos", "normal", "min_dist", "max_dist", "desc")}
    check_points(got, first, cap, False)
    for k in ("kp1", "kp2", "neighbour", "pos", "normal", "min_dist", "max_dist", "desc"):
        tail = got[k][cap:]
        assert tail.size and (tail == GUARD).all(), k
    assert h1[w["kp1"]].all()                                     # the flags do not depend on the capacity


def test_n1_above_the_workspace_is_an_argument_error(gpu):
    import mcs_amd
    from mcs_amd import fuse, new_points as npz
    c = gpu_case("c3x40")
    n1 = len(c["kf1"]["kp_xy"])
    ks, keep = npz.device_set(fuse.pack_targets(c["rig"], [c["kf1"], c["kf2"]], 32, False))
    out, ot = npz.new_out(n1, 32, False)
    m12, h1, h2 = _dev(c["matches12"]), _dev(c["kf1"]["has_mp"]), _dev(c["kf2"]["has_mp"])
    with pytest.raises(mcs_amd.McsError) as e:
        npz.pair_device(npz.Workspace(n1 - 1), ks, 0, 1, n1, 0, m12, 0, h1, h2, None, out)
    assert e.value.code == mcs_amd.MCS_ERR_ARG and "workspace" in str(e.value)
    assert int(ot["count"].item()) == 0 and np.array_equal(h1.cpu().numpy(), c["kf1"]["has_mp"])     # nothing ran


def _loop_inputs(lc):
    from mcs_amd import fuse
    import mcs_amd
    kfs = [lc["kf1"]] + lc["kf2s"]
    T = len(lc["kf2s"])
    E = np.zeros((T, 3, 3, 9))
    mc = np.ascontiguousarray(lc["rig"]["m_c"], np.float64)
    for t in range(T):
        m1, m2 = (np.ascontiguousarray(k["m_t"], np.float64) for k in (lc["kf1"], lc["kf2s"][t]))
        assert mcs_amd.lib().mcs_compute_e_rig_hom(m1.ctypes.data, m2.ctypes.data, mc.ctypes.data, 3, E[t].ctypes.data) == 0
    return kfs, fuse.pack_targets(lc["rig"], kfs, 32, False), E


def _expected_points(lc):
    keys = ("kp1", "kp2", "pos", "normal", "min_dist", "max_dist", "desc")
    want = {k: np.concatenate([r[k] for _, r in lc["points"]]) for k in keys}
    want["neighbour"] = np.concatenate([np.full(len(r["kp1"]), t, np.int32) for t, r in lc["points"]])
    return want


def check_loop(lc, count, got, has, m12=None):
    want = _expected_points(lc)
    assert not any(r["unsure"].any() for _, r in lc["points"])
    n = len(want["kp1"])
    assert count == n
    for k in ("kp1", "kp2", "neighbour", "desc"):
        assert np.array_equal(got[k][:n], want[k]), k
    for k in ("pos", "normal", "min_dist", "max_dist"):
        assert _rel(got[k][:n], want[k]) <= TOL_X, k
    assert np.array_equal(has, np.concatenate(lc["has"]))
    if m12 is not None:
        assert np.array_equal(m12, lc["matches12"])


def test_full_loop_hands_the_flags_over(gpu):
    """T = 3 neighbours, the second skipped, against the sequential CPU evaluation (matcher oracle,
    restatement, flag update); test_loop_case_shows_the_flag_hand_over asserts on the CPU side that
    the case needs the hand-over."""
    import torch
    from mcs_amd import new_points as npz
    lc = loop_case()
    kfs, pk, E = _loop_inputs(lc)
    n_kp = [len(k["kp_xy"]) for k in kfs]
    n1, T = n_kp[0], len(kfs) - 1
    ks, keep = npz.device_set(pk)
    ws, tri = npz.Workspace(n1), npz.TriWorkspace(n1, max(n_kp[1:]))
    out, ot = npz.new_out(n1 * T, 32, False)
    ot["count"].fill_(123)                                         # the entry zeroes it
    has = _dev(np.concatenate([k["has_mp"] for k in kfs]))
    m12 = torch.zeros((T, n1), dtype=torch.int32, device="cuda")
    vd = torch.full((T, n1), 9, dtype=torch.uint8, device="cuda")
    npz.create_device(ws, tri, ks, n_kp, LOOP_SKIP, LOOP_KF2_FIRST, _dev(E), has, th_low(32, False), EPI_THRESH, out, m12, vd)
    torch.cuda.synchronize()
    check_loop(lc, int(ot["count"].item()), {k: t.cpu().numpy() for k, t in ot.items()}, has.cpu().numpy(), m12.cpu().numpy())
    v = vd.cpu().numpy()
    assert (v[1] == 0).all()
    for t, r in lc["points"]:
        assert np.array_equal(v[t], r["verdict"])


def test_host_entry_agrees_and_reports_capacity(gpu):
    import mcs_amd
    from mcs_amd import new_points as npz
    lc = loop_case()
    kfs, pk, E = _loop_inputs(lc)
    has = [k["has_mp"] for k in kfs]
    r = npz.create_new_map_points(lc["rig"], lc["kf1"], lc["kf2s"], LOOP_SKIP, LOOP_KF2_FIRST, E, has, th_low(32, False), EPI_THRESH)
    assert not r["capacity_exceeded"]
    check_loop(lc, r["count"], r, np.concatenate(r["has_mp"]), r["matches12"])
    small = npz.create_new_map_points(lc["rig"], lc["kf1"], lc["kf2s"], LOOP_SKIP, LOOP_KF2_FIRST, E, has, th_low(32, False),
                                      EPI_THRESH, cap=20)
    assert small["capacity_exceeded"] and small["count"] == r["count"] and len(small["kp1"]) == 20
    assert np.array_equal(small["kp1"], r["kp1"][:20]) and np.array_equal(small["pos"], r["pos"][:20])
    assert mcs_amd.lib().mcs_last_error()


def test_cpp_demo_agrees_with_the_device_entry(gpu, tmp_path):
    lc = loop_case()
    kfs = [lc["kf1"]] + lc["kf2s"]
    d = tmp_path / "in"
    d.mkdir()

    def put(fname, a, dt):
        np.ascontiguousarray(a, dt).tofile(str(d / (fname + ".bin")))
    for k in ("m_c", "cam", "scale"):
        put(k, lc["rig"][k], np.float64)
    put("skip", LOOP_SKIP, np.uint8)
    put("kf2_first", LOOP_KF2_FIRST, np.uint8)
    for t, kf in enumerate(kfs):
        p = "k%d_" % t
        for k, dt in (("kp_xy", np.float32), ("kp_octave", np.int32), ("kp_cam", np.int32), ("desc", np.uint8),
                      ("rays", np.float64), ("m_t", np.float64), ("has_mp", np.uint8)):
            put(p + k, kf[k], dt)
    exe = build_demo(tmp_path)
    res = subprocess.run([exe, str(d), "32", str(len(kfs) - 1), str(th_low(32, False))], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    pts = [ln.split() for ln in res.stdout.splitlines() if ln.startswith("point")]
    hs = [ln.split()[2:] for ln in res.stdout.splitlines() if ln.startswith("has")]
    got = dict(neighbour=np.array([p[1] for p in pts], np.int32), kp1=np.array([p[2] for p in pts], np.int32),
               kp2=np.array([p[3] for p in pts], np.int32), pos=np.array([p[4:7] for p in pts], np.float64),
               normal=np.array([p[7:10] for p in pts], np.float64), min_dist=np.array([p[10] for p in pts], np.float64),
               max_dist=np.array([p[11] for p in pts], np.float64),
               desc=np.array([list(bytes.fromhex(p[12])) for p in pts], np.uint8))
    assert all(p[13] == "-" for p in pts)
    check_loop(lc, len(pts), got, np.concatenate([np.array(h, np.uint8) for h in hs]))
