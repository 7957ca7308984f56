"""OptimizeSim3 on the GPU (include/mcs_matcher.h, csrc/sim3_opt.hip) against
tests/golden/sim3opt_ref.npz, the reference's own g2o (tests/golden/gen_sim3opt_ref.py): counts,
flags, iteration and trial counts exact, reals to the tolerance the fixture's measured spreads give
(tests/sim3opt_cases.py: compare).  Then what only the device form has: a candidate alone equals
the candidate in a batch bit for bit, two runs give identical bits, the host-buffer form, the
workspace, the merge helper, the stream-ordered chain from the RANSAC to the refined Sim3 and the
argument errors.
"""
import ctypes

import numpy as np
import pytest

from tests import sim3opt_cases as sc

pytestmark = pytest.mark.gpu
_CASES, _FIX = {}, []


def get_case(name):
    if name not in _CASES:
        _CASES[name] = sc.make_case(name)
    return _CASES[name]


def fixture():
    import os
    if not _FIX:
        _FIX.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3opt_ref.npz")))
    return _FIX[0]


def _so():
    from mcs_amd import sim3_opt
    return sim3_opt


class Device:
    """A case on the device: packed sets, per-slot arrays and the Sim3s as torch tensors."""

    def __init__(self, case, cands=None):
        import torch
        so = _so()
        c = case
        idx = list(range(len(c["kf2s"]))) if cands is None else list(cands)
        pick = lambda xs: [xs[t] for t in idx]  # noqa: E731
        pk1, pp1, pk2, pp2, m12, o1, o2, f2 = so.pack_call(c["rig"], c["kf1"], c["pts1"], pick(c["kf2s"]), pick(c["pts2s"]),
                                                          c["matches12"][idx], c["ok1"], pick(c["ok2s"]),
                                                          pick(c["first2s"]))
        self.k1, self.p1, self.keep1 = so.device_sets(pk1, pp1)
        self.k2, self.p2, self.keep2 = so.device_sets(pk2, pp2)
        self.T, self.n1 = len(idx), pk1["n_kp_total"]
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
        self.m12_in = up(m12, np.int32)
        self.ok1, self.ok2, self.f2 = up(o1, np.uint8), up(o2, np.uint8), up(f2, np.int32)
        self.is1, self.s2 = up(c["inv_sigma2_1"], np.float64), up(c["sigma2_2"], np.float64)
        self.s, self.R, self.t = up(c["s12"][idx], np.float64), up(c["R12"][idx], np.float64), up(c["t12"][idx], np.float64)
        self.opts = so.default_options(c["flags"], **{k: v for k, v in c["opts"].items()})

    def run(self, ws=None, opts=None, out=None):
        """-> (the arrays of mcs_sim3_opt_out as NumPy by name, matches12 after the call)."""
        import torch
        m12 = self.m12_in.clone()
        ts = _so().optimize_sim3_device(ws, self.k1, self.p1, self.k2, self.p2, m12, self.ok1, self.ok2, self.f2,
                                        self.is1, self.s2, self.s, self.R, self.t, opts or self.opts, out=out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in ts.items()}, m12.cpu().numpy()


def same_bits(a, b):
    for k in a[0]:
        assert a[0][k].tobytes() == b[0][k].tobytes(), k
    assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_device_entry_equals_the_reference_g2o(gpu, name):
    case = get_case(name)
    out, m12 = Device(case).run()
    sc.compare(fixture(), name, sc.results_of(out, m12))
    for t in range(len(case["kf2s"])):               # R12 is the rotation of q12; the input before the recover
        r = sc.results_of(out, m12)[t]
        if r["n_corr"] - r["n_bad"] < 3:
            assert np.array_equal(r["R"], case["R12"][t]) and r["s"] == case["s12"][t] and np.array_equal(r["t"], case["t12"][t])
        else:
            w, x, y, z = r["q"]
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            assert np.abs(R.reshape(9) - r["R"]).max() < 1e-14
        assert r["lam"][0] >= 0 and (r["iters"][1] > 0) == (r["lam"][1] > 0)


def test_a_candidate_alone_equals_the_batch_bit_for_bit(gpu):
    for name in ("C_batch", "K_batch_wide"):         # K: three slot rounds, candidates of 300 / 257 / 0 / 5 pairs
        case = get_case(name)
        out, m12 = Device(case).run()
        for t in range(len(case["kf2s"])):
            one, m1 = Device(case, [t]).run()
            for k in out:
                assert one[k][0].tobytes() == out[k][t].tobytes(), (name, t, k)
            assert np.array_equal(m1[0], m12[t]), (name, t)


def test_two_runs_give_identical_bits(gpu):
    for name in ("B_outliers", "K_batch_wide"):
        dev = Device(get_case(name))
        same_bits(dev.run(), dev.run())


def test_workspace_and_host_form_equal_the_plain_call(gpu):
    so = _so()
    case = get_case("C_batch")
    dev = Device(case)
    want = dev.run()
    ws = so.Workspace(4, 128)
    same_bits(dev.run(ws=ws), want)
    same_bits(dev.run(ws=ws), want)                  # the workspace is reusable
    ws.close()
    host = so.optimize_sim3(*sc.call_args(case), case["inv_sigma2_1"], case["sigma2_2"], case["s12"], case["R12"],
                            case["t12"], options=case["opts"], flags=case["flags"])
    for k in want[0]:
        assert host[k].tobytes() == want[0][k].tobytes(), k
    assert np.array_equal(host["matches12"], want[1])


def test_outputs_the_caller_leaves_out(gpu):
    """edge_chi2 and trials are nullable; the rest is unchanged without them."""
    so = _so()
    dev = Device(get_case("E_skips"))
    want = dev.run()
    got = dev.run(out=so.new_out(dev.T, dev.n1, edge_chi2=False, trials=False))
    assert "edge_chi2" not in got[0] and "trials" not in got[0]
    for k in got[0]:
        assert got[0][k].tobytes() == want[0][k].tobytes(), k
    assert np.array_equal(got[1], want[1])


def test_merge_helper_equals_numpy(gpu):
    import torch
    rng = np.random.default_rng(5)
    T, n1 = 3, 347                                   # T * n1 = 1041: four blocks of 256 and a tail
    bow = rng.integers(-1, 50, (T, n1)).astype(np.int32)
    new = rng.integers(-1, 50, (T, n1)).astype(np.int32)
    inl = (rng.random((T, n1)) < 0.3).astype(np.uint8)
    got = _so().merge_matches_device(*(torch.from_numpy(a).cuda() for a in (bow, inl, new)))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), np.where(inl != 0, bow, np.where(new >= 0, new, -1)))


def test_stream_ordered_chain_from_the_ransac_to_the_refined_sim3(gpu):
    """iterate -> active -> SearchBySim3 -> merge -> OptimizeSim3 on a side stream with workspaces
    and one synchronisation at the end, against the same steps through the host-buffer forms."""
    import torch
    from mcs_amd import sim3_match, sim3_solver
    from tests.test_sim3solver_ref import CAP, MIN_INL, PROB, get_case as solver_case, np_good_flags
    so = _so()
    c = solver_case("t3_mixed")
    good1, good2s = np_good_flags(c, 9)
    T, n1 = len(c["kf2s"]), len(c["kf1"]["kp_xy"])
    nb, th_high = 32, sim3_match.th_high(32, False)
    zeros = np.zeros
    pk1, pp1, pk2, pp2, _, _, _, _, _ = sim3_match.pack_call(c["rig"], c["kf1"], c["pts1"], c["kf2s"], c["pts2s"],
                                                            zeros((T, n1), np.uint8), [zeros(len(k["kp_xy"]), np.uint8) for k in c["kf2s"]],
                                                            zeros(T), zeros((T, 9)), zeros((T, 3)), nb, True)
    k1, p1, keep1 = sim3_match.device_sets(pk1, pp1)
    k2, p2, keep2 = sim3_match.device_sets(pk2, pp2)
    n2 = pk2["n_kp_total"]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])  # noqa: E731
    bow, ok1, ok2 = up(c["matches12"], np.int32), up(c["ok1"], np.uint8), up(cat(c["ok2s"], np.uint8), np.uint8)
    f1, f2 = up(c["first1"], np.int32), up(cat(c["first2s"], np.int32), np.int32)
    sig = np.asarray(c["sigma2"], np.float64)
    sigma2, inv_sigma2 = up(sig, np.float64), up(1.0 / sig, np.float64)
    samples, g1, g2 = up(c["samples"], np.int32), up(good1, np.uint8), up(cat(good2s, np.uint8), np.uint8)
    ws_s, ws_m, ws_o = sim3_solver.Workspace(T, n1, CAP), sim3_match.Workspace(T, max(n1, n2)), so.Workspace(T, n1)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        corr, _ = sim3_solver.new_corr(k1, T)
        ran, rt = sim3_solver.new_ransac(T, n1, CAP, hyp=False)
        a1 = torch.empty((T, n1), dtype=torch.uint8, device="cuda")
        a2 = torch.empty((n2,), dtype=torch.uint8, device="cuda")
        sim3_solver.prepare_device(k1, p1, k2, p2, bow, ok1, ok2, f1, f2, sigma2, corr)
        sim3_solver.iterate_device(ws_s, corr, samples, CAP, PROB, MIN_INL, CAP, sim3_solver.INIT, ran)
        sim3_solver.active_device(k1, k2, rt["inlier"], g1, g2, bow, f2, a1, a2)
        _, _, new12, _ = sim3_match.search_by_sim3_device(ws_m, k1, p1, k2, p2, a1, a2, rt["s12"], rt["R12"], rt["t12"],
                                                        10.0, th_high)
        merged = so.merge_matches_device(bow, rt["inlier"], new12)
        m_in = merged.clone()
        got = so.optimize_sim3_device(ws_o, k1, p1, k2, p2, merged, ok1, ok2, f2, inv_sigma2, sigma2, rt["s12"],
                                      rt["R12"], rt["t12"])
    st.synchronize()                                  # the one synchronisation
    # the same steps through the host-buffer forms
    h = sim3_solver.sim3_solver(c["rig"], c["kf1"], c["pts1"], c["kf2s"], c["pts2s"], c["matches12"], c["ok1"], c["ok2s"],
                                c["first1"], c["first2s"], sig, c["samples"], CAP, PROB, MIN_INL, CAP, sim3_solver.INIT,
                                good1=good1, good2s=good2s)
    _, _, h_new, _ = sim3_match.search_by_sim3(c["rig"], c["kf1"], c["pts1"], c["kf2s"], c["pts2s"], h["active1"],
                                              h["active2"], h["s12"], h["R12"], h["t12"], 10.0, th_high)
    h_merged = np.where(h["inlier"] != 0, c["matches12"], np.where(h_new >= 0, h_new, -1)).astype(np.int32)
    assert np.array_equal(m_in.cpu().numpy(), h_merged)
    print("inliers", int((h["inlier"] != 0).sum()), "merged", int((h_merged >= 0).sum()))
    assert (h["inlier"] != 0).sum() > 0, "the chain must carry RANSAC inliers"
    ho = so.optimize_sim3(c["rig"], c["kf1"], c["pts1"], c["kf2s"], c["pts2s"], h_merged, c["ok1"], c["ok2s"],
                          c["first2s"], 1.0 / sig, sig, h["s12"], h["R12"], h["t12"])
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == ho[k].tobytes(), k
    assert np.array_equal(merged.cpu().numpy(), ho["matches12"])
    assert ho["n_corr"].max() >= 3
    for w in (ws_s, ws_m, ws_o):
        w.close()


def test_argument_errors_of_the_device_entries(gpu):
    import mcs_amd
    import torch
    so = _so()
    dev = Device(get_case("C_batch"))
    out = so.new_out(dev.T, dev.n1)

    def variant(src, **kw):
        s = type(src)()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(src), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def code(ws=None, k1=dev.k1, k2=dev.k2, p1=dev.p1, opts=dev.opts, out=out, m12=dev.m12_in, ok2=dev.ok2):
        with pytest.raises(mcs_amd.McsError) as e:
            so.optimize_sim3_device(ws, k1, p1, k2, dev.p2, m12, dev.ok1, ok2, dev.f2, dev.is1, dev.s2, dev.s, dev.R,
                                    dev.t, opts, out=out)
        return e.value.code
    ARG = mcs_amd.MCS_ERR_ARG
    assert code(ws=so.Workspace(3, 128)) == ARG                               # more candidates than the workspace
    assert code(ws=so.Workspace(4, 64)) == ARG                                # more keypoints
    assert code(k1=variant(dev.k1, n_targets=2)) == ARG
    assert code(k1=variant(dev.k1, n_cams=9), k2=variant(dev.k2, n_cams=9)) == ARG
    assert code(k2=variant(dev.k2, n_levels=7)) == ARG
    assert code(k2=variant(dev.k2, n_cams=2)) == ARG
    assert code(k1=variant(dev.k1, kp_xy=None)) == ARG
    assert code(p1=variant(dev.p1, n=dev.n1 - 1)) == ARG
    assert code(p1=variant(dev.p1, pos=None)) == ARG
    assert code(m12=None) == ARG
    assert code(ok2=None) == ARG
    assert code(opts=variant(dev.opts, its_round1=17)) == ARG
    assert code(opts=variant(dev.opts, its_culled=-1)) == ARG
    assert code(opts=variant(dev.opts, max_trials=0)) == ARG
    assert code(opts=variant(dev.opts, std_sim=-4.0)) == ARG
    assert code(opts=variant(dev.opts, flags=2)) == ARG
    assert code(out=(variant(out[0], q12=None), out[1])) == ARG
    z = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(mcs_amd.McsError) as e:
        lib = mcs_amd.lib()
        mcs_amd._check(lib.mcs_sim3_merge_matches_device(z.data_ptr(), None, z.data_ptr(), 2, 8, z.data_ptr(), None))
    assert e.value.code == ARG
    with pytest.raises(mcs_amd.McsError) as e:
        mcs_amd._check(mcs_amd.lib().mcs_sim3_merge_matches_device(z.data_ptr(), z.data_ptr(), z.data_ptr(), -1, 8,
                                                                   z.data_ptr(), None))
    assert e.value.code == ARG
    sc.compare(fixture(), "C_batch", sc.results_of(*dev.run()))               # everything is still usable
