"""The host plan of the block-sparse essential-graph solver (include/mcs_essgraph.h:
mcs_essgraph_plan_create with device < 0, csrc/essential_graph_plan.cpp) on the edge lists of
tests/golden/essgraph_ref.npz: the invariants every numeric kernel relies on, checked from the
plan's own arrays by brute force, the canonical form, and a 10 000-keyframe map.  No GPU."""
import time

import numpy as np
import pytest

from tests import essgraph_cases as ec
from tests import essgraph_sparse_cases as sc

GRAPHS = ("A_ring6", "C_cov40", "G_mid100", "H_cov130", "J_n300")


def _es():
    from mcs_amd import essential_graph
    return essential_graph


def pattern(arr, n):
    """The plan's lower block pattern of L (permuted order) as a dense boolean matrix, and the supernode of every column."""
    L = np.zeros((n, n), bool)
    sn = np.zeros(n, np.int32)
    for s in range(len(arr["col0"]) - 1):
        c0, c1 = arr["col0"][s], arr["col0"][s + 1]
        rows = arr["rows"][arr["row_ptr"][s]:arr["row_ptr"][s + 1]]
        assert np.array_equal(rows[:c1 - c0], np.arange(c0, c1)) and (np.diff(rows) > 0).all()
        sn[c0:c1] = s
        for c in range(c0, c1):
            L[rows[rows >= c], c] = True
    return L, sn


@pytest.mark.parametrize("leaf", [None, 4, 16])
@pytest.mark.parametrize("name", GRAPHS)
def test_plan_invariants(built, name, leaf):
    es = _es()
    edges, N, loop = sc.graph(name)
    plan = es.Plan(N, loop, edges, leaf_size=leaf, device=-1)
    info, arr = plan.info, plan.arrays()
    n = N - 1
    print(name, leaf, info)
    assert info["free_blocks"] == n and info["leaf_size"] == (4 if leaf is None else leaf)
    assert info["device_bytes"] == 0
    perm = arr["perm"]
    assert np.array_equal(np.sort(perm), np.arange(n))                       # the ordering is a permutation
    L, sn = pattern(arr, n)
    free = lambda v: -1 if v == loop else (v if v < loop else v - 1)         # noqa: E731
    pairs = {(min(free(a), free(b)), max(free(a), free(b))) for a, b, _ in edges.tolist()
             if free(a) >= 0 and free(b) >= 0}
    A = np.eye(n, dtype=bool)
    for a, b in pairs:                                                       # every edge pair has a slot
        i, j = max(perm[a], perm[b]), min(perm[a], perm[b])
        assert L[i, j], (a, b)
        A[i, j] = True
    assert info["a_blocks"] == n + len(pairs) == int(arr["a_block"].sum())
    assert info["l_blocks"] == int(L.sum()) and info["panel_blocks"] == len(arr["a_block"])
    # a_block marks exactly the blocks of A
    marked = np.zeros((n, n), bool)
    for s in range(info["supernodes"]):
        c0, c1 = arr["col0"][s], arr["col0"][s + 1]
        rows = arr["rows"][arr["row_ptr"][s]:arr["row_ptr"][s + 1]]
        blk = arr["a_block"][arr["block_off"][s]:arr["block_off"][s + 1]].reshape(len(rows), c1 - c0)
        for p, r in enumerate(rows):
            for c in range(c1 - c0):
                if blk[p, c]:
                    assert r >= c0 + c
                    marked[r, c0 + c] = True
    assert np.array_equal(marked, A)
    # closed under elimination: boolean elimination of the plan's pattern adds nothing, and the
    # elimination of A's pattern stays inside it
    for start in (L, A):
        F = start.copy()
        for k in range(n):
            below = np.flatnonzero(F[k + 1:, k]) + k + 1
            F[np.ix_(below, below)] |= np.tril(np.ones((len(below), len(below)), bool))
        assert not (F & ~L).any()
    # a tree parent comes after its children; levels are heights; a level's supernodes are independent
    par, lev = arr["parent"], arr["level"]
    for s in range(info["supernodes"]):
        rows = arr["rows"][arr["row_ptr"][s]:arr["row_ptr"][s + 1]]
        below = rows[rows >= arr["col0"][s + 1]]
        if len(below):
            assert par[s] == sn[below[0]] and par[s] > s and lev[par[s]] > lev[s]
            assert (lev[sn[below]] > lev[s]).all()                           # every block below lies in a later level
        else:
            assert par[s] == -1
    assert info["levels"] == lev.max() + 1
    for s in range(info["supernodes"]):
        kids = np.flatnonzero(par == s)
        assert lev[s] == (lev[kids].max() + 1 if len(kids) else 0)
    assert info["solver_launches_per_trial"] <= 2 * info["levels"]
    assert info["launches_per_trial"] == info["solver_launches_per_trial"] + 6
    if name == "C_cov40" and leaf == 4:
        assert info["levels"] >= 3
    plan.close()


@pytest.mark.parametrize("name", ["C_cov40", "H_cov130", "J_n300"])
def test_permuted_edge_list_gives_the_same_plan(built, name):
    es = _es()
    edges, N, loop = sc.graph(name)
    want = es.Plan(N, loop, edges, device=-1)
    rng = np.random.default_rng(9)
    shuffled = edges[rng.permutation(len(edges))].copy()
    flip = rng.uniform(size=len(shuffled)) < 0.5                              # the pair is unordered
    shuffled[flip, 0], shuffled[flip, 1] = shuffled[flip, 1].copy(), shuffled[flip, 0].copy()
    got = es.Plan(N, loop, np.concatenate([shuffled, shuffled[:7]]), device=-1)    # a pair twice counts once
    assert got.info == want.info and want.info["digest"] != 0
    a, b = want.arrays(), got.arrays()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    other = es.Plan(N, loop, edges[:-3], device=-1)
    assert other.info["digest"] != want.info["digest"]


def test_plan_refuses_bad_arguments_and_keeps_the_dense_limits(built):
    import mcs_amd
    es = _es()
    for bad in ([[0, 9, 0]], [[2, 2, 0]], [[-1, 1, 0]]):
        with pytest.raises(mcs_amd.McsError) as e:
            es.Plan(6, 0, np.array(bad, np.int32), device=-1)
        assert e.value.code == mcs_amd.MCS_ERR_ARG
    with pytest.raises(mcs_amd.McsError) as e:
        es.Plan(6, 6, np.array([[0, 1, 0]], np.int32), device=-1)
    assert e.value.code == mcs_amd.MCS_ERR_ARG
    assert es.supported(878) and not es.supported(879)                       # the dense entries' cap stays
    one = es.Plan(1, 0, np.zeros((0, 3), np.int32), device=-1)               # nothing free: an empty plan
    assert one.info["free_blocks"] == 0 and one.info["supernodes"] == 0


def test_ten_thousand_keyframes_plan(built):
    """A 10 000-keyframe chain with 12 neighbours and the `cov` loop edges: time and fill are
    printed (DESIGN 3.14 records them), nothing about them is asserted."""
    es = _es()
    edges = sc.chain_edges(10000, 12, cov=True)
    t0 = time.perf_counter()
    plan = es.Plan(10000, 0, edges, device=-1)
    dt = time.perf_counter() - t0
    i = plan.info
    print("10000 keyframes: %d edges, plan %.1f ms, fill %.3f, supernodes %d, levels %d, launches per trial %d, "
          "L %.1f MB, %.2f Gflop per factor" % (len(edges), 1e3 * dt, i["fill"], i["supernodes"], i["levels"],
                                               i["launches_per_trial"], i["panel_blocks"] * 392 / 1e6,
                                               i["flops_per_factor"] / 1e9))
    assert i["free_blocks"] == 9999 and np.array_equal(np.sort(plan.arrays()["perm"]), np.arange(9999))
