"""OptimizeEssentialGraph on the GPU (include/mcs_essgraph.h, csrc/essential_graph.hip) against
tests/golden/essgraph_ref.npz, the reference's own g2o (tests/golden/gen_essgraph_ref.py): edge
lists, iteration and trial counts exact, reals to the tolerance the fixture's measured spreads give
(tests/essgraph_cases.py: compare).  Then what only the device form has: identical bits from two
runs, a permuted edge list re-sorted to the same bits, the point references resolved on the device,
a second call on a workspace that allocates nothing, the banded solve against the dense one, and
the status word for indices out of range.

The one-trial cases (essgraph_cases.ONE_TRIAL) are past one round of every kernel: more than 256
and more than 16384 edges (2 to 64 chi2 partials, the stride loop), more than 256 keyframes and
points, 11 to 33 tiles, the loop keyframe off tile 0.  They are held to g2o by the same rule and,
about ten times tighter, to the host replica's outputs at the same difference step
(`host_<case>_*`, tolerance from the replica's own spread over its three steps).
"""
import os

import numpy as np
import pytest

from tests import essgraph_cases as ec

pytestmark = pytest.mark.gpu
_CASES, _FIX = {}, []


def get_case(name):
    if name not in _CASES:
        _CASES[name] = ec.make_case(name)
    return _CASES[name]


def fixture():
    if not _FIX:
        _FIX.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essgraph_ref.npz")))
    return _FIX[0]


def _es():
    from mcs_amd import essential_graph
    return essential_graph


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


class Device:
    """A case on the device as torch tensors."""

    def __init__(self, case, edges=None, band=None):
        es = _es()
        self.case = case
        self.edges_np = np.ascontiguousarray(fixture()[case["name"] + "_edges"] if edges is None else edges, np.int32)
        self.Scw, self.Snc = up(case["Scw"], np.float64), up(case["Snc"], np.float64)
        self.edges = up(self.edges_np, np.int32)
        self.pos = up(case["pos"], np.float64)
        self.ref, self.bad = up(ec.point_refs(case), np.int32), up(case["bad"], np.uint8)
        o = case["opts"]
        self.opts = es.default_options(iterations=o["iterations"], terminate_max_iter=o["terminate_max_iter"],
                                       gain_threshold=o["gain_threshold"], lambda0=o["lambda0"],
                                       max_trials=o["max_trials"],
                                       tile_band=es.tile_band(case["N"], case["loop"], self.edges_np) if band is None else band)

    def run(self, ws=None, out=None, edges=None, ref=None):
        """-> the arrays of mcs_essgraph_out by name (NumPy) and `points`."""
        import torch
        pos = self.pos.clone()
        ts = _es().optimize_device(ws, self.Scw, self.Snc, self.case["loop"], self.edges if edges is None else edges,
                                   pos, self.ref if ref is None else ref, self.bad, self.opts, out=out)
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in ts.items()}
        r["points"] = pos.cpu().numpy()
        return r


def as_result(r):
    return dict(r, iterations=int(r["iterations"][0]), trials=r["trials"])


def same_bits(a, b, skip=()):
    for k in a:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", list(ec.CASES))
def test_device_entry_equals_the_reference_g2o(gpu, name):
    case = get_case(name)
    r = Device(case).run()
    assert r["status"][0] == 0
    ec.compare(fixture(), name, as_result(r))
    n_it = r["iterations"][0]
    assert (r["trials"][n_it:] == 0).all() and (r["chi2"][n_it:] == 0).all() and r["lambda"][0] > 0
    for i in range(case["N"]):                          # rot is the rotation of the quaternion, pose its inverse SE3
        s, (w, x, y, z), t = r["sim3"][i, 0], r["sim3"][i, 1:5], r["sim3"][i, 5:8]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.abs(R.reshape(9) - r["rot"][i]).max() < 1e-14
        M = r["pose"][i].reshape(4, 4)
        assert np.abs(M[:3, :3] - R.T).max() < 1e-14 and np.abs(M[:3, 3] + R.T @ (t / s)).max() < 1e-12
    if name == "E_consistent":                          # rho = 0: one rejected trial, nothing moves
        assert r["trials"][0] == 1 and np.array_equal(r["sim3"], case["Scw"])
        keep = case["bad"] == 0
        assert np.array_equal(r["points"][keep], case["pos"][keep])
    bad = case["bad"] != 0
    assert np.array_equal(r["points"][bad], case["pos"][bad])          # :498 a bad point stays


ONE_TRIAL = [n for n in ec.CASES if "opts" in ec.CASES[n]]


@pytest.mark.parametrize("name", ONE_TRIAL)
def test_device_entry_equals_the_host_replica_at_the_same_step(gpu, name):
    """The device and the replica share the difference step and the edge math; summation order and
    the solver differ.  Tolerance: 8 x the replica's spread over the steps 5e-9, 1e-8, 2e-8."""
    case = get_case(name)
    es = _es()
    band = es.tile_band(case["N"], case["loop"], fixture()[name + "_edges"])
    print(name, "tile band", band)
    r = Device(case).run()
    assert r["status"][0] == 0
    ec.compare(fixture(), "host_" + name, as_result(r))


def test_two_runs_give_identical_bits(gpu):
    for name in ("C_cov40", "I_dense300"):           # I: 64 chi2 partials, added in index order
        dev = Device(get_case(name))
        same_bits(dev.run(), dev.run())


def test_permuted_edge_list_is_resorted_to_the_same_bits(gpu):
    """The entry sorts the edges by (v0, v1, kind) before anything is summed, so the order in which
    the caller lists them does not reach a single bit; per-edge outputs follow the caller's order."""
    for name in ("C_cov40", "I_dense300"):
        dev = Device(get_case(name))
        want = dev.run()
        perm = np.random.default_rng(5).permutation(len(dev.edges_np))
        got = dev.run(edges=up(dev.edges_np[perm], np.int32))
        same_bits(want, got, skip=("edge_chi2",))
        assert want["edge_chi2"][perm].tobytes() == got["edge_chi2"].tobytes()


def test_point_references_resolved_on_the_device(gpu):
    import torch
    case = get_case("C_cov40")
    ref = _es().resolve_point_refs_device(up(case["ids"], np.int64), up(case["corrected_by"], np.int64),
                                          up(case["corrected_ref"], np.int64), up(case["ref_kf"], np.int64),
                                          int(case["ids"][case["cur"]]))
    torch.cuda.synchronize()
    want = ec.point_refs(case)
    assert np.array_equal(ref.cpu().numpy(), want)
    assert (case["corrected_by"] == case["ids"][case["cur"]]).sum() > 10 and len(set(want.tolist())) > 10
    dev = Device(case)
    same_bits(dev.run(), dev.run(ref=ref))
    miss = _es().resolve_point_refs_device(up(case["ids"], np.int64), up([-1, 5], np.int64), up([0, 0], np.int64),
                                           up([1, int(case["ids"][3])], np.int64), 5)
    assert miss.cpu().numpy().tolist() == [-1, -1]          # no keyframe has the id: the entry's range check refuses it


def test_workspace_call_allocates_nothing_and_equals_the_plain_call(gpu):
    import torch
    es = _es()
    case = get_case("B_ring12")
    dev = Device(case)
    want = dev.run()
    ws = es.Workspace(16, 64, 32)
    out = es.new_out(case["N"], len(dev.edges_np))
    same_bits(dev.run(ws=ws, out=out), want)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    pos = dev.pos.clone()
    free1 = torch.cuda.mem_get_info()[0]
    es.optimize_device(ws, dev.Scw, dev.Snc, case["loop"], dev.edges, pos, dev.ref, dev.bad, dev.opts, out=out)
    free2 = torch.cuda.mem_get_info()[0]               # before any synchronisation: nothing was allocated
    torch.cuda.synchronize()
    assert free2 == free1 <= free0
    assert out[1]["sim3"].cpu().numpy().tobytes() == want["sim3"].tobytes()
    import mcs_amd
    with pytest.raises(mcs_amd.McsError) as e:         # counts above the workspace
        Device(get_case("C_cov40")).run(ws=ws)
    assert e.value.code == mcs_amd.MCS_ERR_ARG
    ws.close()
    host = es.optimize(case["Scw"], case["Snc"], case["loop"], dev.edges_np, case["pos"], ec.point_refs(case),
                       case["bad"], options=case["opts"])
    for k in want:
        assert host[k].tobytes() == want[k].tobytes(), k


def test_workspace_sized_for_the_largest_case_is_reused_for_the_smallest(gpu):
    """A workspace of exactly J_n300's counts (33 tiles), then A_ring6 (1 tile) and J_n300 again on
    it: the cached task table changes between the calls, the results are those of the plain calls."""
    es = _es()
    big, small = Device(get_case("J_n300")), Device(get_case("A_ring6"))
    want_big, want_small = big.run(), small.run()
    ws = es.Workspace(big.case["N"], len(big.edges_np), big.case["P"])
    same_bits(big.run(ws=ws), want_big)
    same_bits(small.run(ws=ws), want_small)
    same_bits(big.run(ws=ws), want_big)
    ws.close()


def test_banded_solve_equals_the_dense_one(gpu):
    """40 keyframes with the edges of neighbours at most two apart: 5 tiles of band 2.  The banded
    factorisation skips only tiles that are zero, so it solves the same systems; the rule's floor,
    1e-9 of the field's scale, bounds what a different task order could leave."""
    case = get_case("C_cov40")
    e = fixture()["C_cov40_edges"]
    near = e[np.abs(e[:, 0] - e[:, 1]) <= 2]
    es = _es()
    assert es.tile_band(case["N"], case["loop"], near) == 2 and es.tile_band(case["N"], case["loop"], e) == 5
    banded, dense = Device(case, near).run(), Device(case, near, band=0).run()
    assert banded["status"][0] == 0 and dense["status"][0] == 0 and banded["iterations"][0] > 0
    assert np.array_equal(banded["trials"], dense["trials"])
    for k in ("sim3", "pose", "points", "chi2", "edge_chi2"):
        assert np.abs(banded[k] - dense[k]).max() <= 1e-9 * max(1.0, np.abs(dense[k]).max()), k
    narrow = Device(case, e, band=2).run()              # an edge outside the stated band
    assert narrow["status"][0] == -1


def test_banded_solve_equals_the_dense_one_at_eleven_tiles(gpu):
    """G_mid100 as it is: neighbours at most 6 keyframes apart are 11 tiles of band 2 with the fixed
    keyframe in tile 4; the same rule as above against band = 0.  H_cov130's edges reach across
    the whole chain: band 2 is refused."""
    es = _es()
    case = get_case("G_mid100")
    e = fixture()["G_mid100_edges"]
    assert es.tile_band(case["N"], case["loop"], e) == 2
    banded, dense = Device(case).run(), Device(case, band=0).run()
    assert banded["status"][0] == 0 and dense["status"][0] == 0 and banded["iterations"][0] == 1
    assert np.array_equal(banded["trials"], dense["trials"])
    for k in ("sim3", "pose", "points", "chi2", "edge_chi2"):
        d = np.abs(banded[k] - dense[k]).max()
        print("G_mid100 banded - dense", k, d)
        assert d <= 1e-9 * max(1.0, np.abs(dense[k]).max()), k
    wide = get_case("H_cov130")
    assert es.tile_band(wide["N"], wide["loop"], fixture()["H_cov130_edges"]) > 2
    assert Device(wide, band=2).run()["status"][0] == -1


def test_index_out_of_range_is_reported_and_nothing_is_touched(gpu):
    import torch
    es = _es()
    case = get_case("A_ring6")
    dev = Device(case)
    for what in ("v0", "v1", "self", "kind", "ref"):
        edges, ref = dev.edges_np.copy(), ec.point_refs(case).copy()
        if what == "v0":
            edges[3, 0] = case["N"]
        elif what == "v1":
            edges[5, 1] = -1
        elif what == "self":
            edges[2, 1] = edges[2, 0]
        elif what == "kind":
            edges[1, 2] = 2
        else:
            ref[int(np.flatnonzero(case["bad"] == 0)[0])] = case["N"] + 3
        out = es.new_out(case["N"], len(edges))
        for t in out[1].values():
            t.fill_(7)
        r = dev.run(out=out, edges=up(edges, np.int32), ref=up(ref, np.int32))
        assert r["status"][0] == -1, what
        assert np.array_equal(r["points"], case["pos"]), what
        for k in ("sim3", "rot", "pose", "chi2", "edge_chi2", "iterations", "trials", "lambda"):
            assert (r[k] == 7).all(), (what, k)
    torch.cuda.synchronize()
    import mcs_amd
    with pytest.raises(mcs_amd.McsError) as e:          # the host form turns the status into its return value
        es.optimize(case["Scw"], case["Snc"], case["loop"], np.array([[1, 9, 0]], np.int32))
    assert e.value.code == mcs_amd.MCS_ERR_ARG


def test_unsupported_above_the_solver_limit_from_size_arithmetic(gpu):
    import mcs_amd
    es = _es()
    assert es.supported(878) and not es.supported(879)
    with pytest.raises(mcs_amd.McsError) as e:
        es.Workspace(879, 8, 0)
    assert e.value.code == mcs_amd.MCS_ERR_UNSUPPORTED
    big = np.tile(get_case("A_ring6")["Scw"][:1], (2000, 1))
    with pytest.raises(mcs_amd.McsError) as e:
        es.optimize(big, big, 0, np.array([[1, 0, 0]], np.int32))
    assert e.value.code == mcs_amd.MCS_ERR_UNSUPPORTED
