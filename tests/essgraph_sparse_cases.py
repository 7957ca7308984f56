"""Cases of the block-sparse essential-graph solver beyond what tests/essgraph_cases.py holds: the
graphs of its fixture as plain edge lists, a synthetic chain of any length, and K_cov1000, a map
above the dense solver's 878 keyframes, for tests/golden/gen_essgraph_sparse_ref.py and
tests/test_essgraph_sparse_gpu.py.  essgraph_cases.CASES is left as it is: other modules
parametrise over it.

K_cov1000 is C_cov40's content (second neighbours around the weight threshold, an earlier loop,
loop connections of three keyframes, a pair with two edges) on 1000 keyframes with 12 neighbours.
essgraph_cases.make_case cannot make it: its height 0.05 i and rotation vector (0.02 i, -0.03 i, .)
grow with the index, and at N = 1000 the reference's three difference steps then disagree after one
trial, so the fixture's own rule would hold nothing.  The track here is bounded: centre
4 (cos a, sin a, 0.5 sin 0.03 i), rotation vector (0.4 sin 0.05 i, -0.6 cos 0.04 i, a); everything
else, the order of the random draws included, is make_case's.
"""
import os

import numpy as np

from tests import essgraph_cases as ec

SPARSE_CASES = {
    "K_cov1000": dict(seed=402, N=1000, drift=(0.10, 0.5, 1.10), P=200, cov=True, n_corr=4, nbr=12, loop=0,
                      opts=ec.ONE_TRIAL),
}

_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essgraph_ref.npz")))
    return _FIX[0]


def graph(name):
    """(edges int32 [E, 3], N, loop) of a case of essgraph_cases, the edges from its fixture."""
    return (np.ascontiguousarray(fixture()[name + "_edges"], np.int32), ec.CASES[name]["N"],
            ec.CASES[name].get("loop", 0))


def chain_edges(N, nbr, cov=False, loop=0):
    """The pairs a chain of N keyframes with `nbr` covisible predecessors gives, as an edge list;
    cov adds loop connections from the last three keyframes to the first three, which join free
    keyframes across the chain."""
    rows = [(i, i - k, 0) for k in range(1, nbr + 1) for i in range(k, N)]
    cur = N - 1
    rows += [(cur, loop, 0)]
    if cov:
        rows += [(cur, 1, 0), (cur - 1, 0, 0), (cur - 1, 2, 0), (cur - 2, 2, 0), (cur - 2, 1, 0)]
    return np.array(rows, np.int32)


def make_sparse_case(name, seed=None):
    """essgraph_cases.make_case on the bounded track (see the head)."""
    P = SPARSE_CASES[name]
    rng = np.random.default_rng(P["seed"] if seed is None else seed)
    N = P["N"]
    loop = P.get("loop", 0)
    cur = N - 1
    ids = np.arange(N, dtype=np.int64) + 3
    Snc = np.zeros((N, 8))
    span = max(1, cur - loop)
    axis, tdir = rng.normal(size=3), rng.normal(size=3)
    axis, tdir = axis / np.linalg.norm(axis), tdir / np.linalg.norm(tdir)
    jit = rng.uniform(0.9, 1.1, 2)
    rot, tr, sc = P["drift"]
    for i in range(N):
        f = (i - loop) / span
        ang = 2 * np.pi * (i - loop) / (span + 1)
        centre = 4.0 * np.array([np.cos(ang), np.sin(ang), 0.5 * np.sin(0.03 * i)])
        rv = np.array([0.4 * np.sin(0.05 * i), -0.6 * np.cos(0.04 * i), ang])
        drift = ec.sim3(1.0, rot * jit[0] * f * axis, tr * jit[1] * f * tdir)
        true = ec.sim3(1.0, rv, [0, 0, 0])
        true[5:8] = -ec.qrot(true[1:5], centre * (1.0 + (sc - 1.0) * f))
        Snc[i] = ec.smul(drift, true)
        Snc[i][0] = 1.0
    Scw = Snc.copy()
    has_corr = np.zeros(N, np.uint8)
    n_corr = P.get("n_corr", 1)
    gamma = ec.sinv(ec.sim3(sc, rot * jit[0] * axis, tr * jit[1] * tdir))
    cur_corr = ec.smul(gamma, Snc[cur])
    for i in range(cur - n_corr + 1, cur + 1):
        Scw[i] = ec.smul(ec.smul(Snc[i], ec.sinv(Snc[cur])), cur_corr)
        has_corr[i] = 1
    parent = np.arange(-1, N - 1, dtype=np.int32)
    loops = [[] for _ in range(N)]
    cov = [[] for _ in range(N)]
    lc = [[] for _ in range(N)]
    for k in range(1, P.get("nbr", 1) + 1):
        for i in range(k, N):
            cov[i].append((i - k, 150))
            cov[i - k].append((i, 150))
    lc[cur].append((loop, 30))
    if P.get("cov"):
        for i in range(2, N):
            w = 99 + i % 3
            cov[i].append((i - 2, w))
            cov[i - 2].append((i, w))
        loops[20].append(5)
        loops[5].append(20)
        lc[cur] = [(0, 30), (1, 120), (2, 80)]
        lc[cur - 1] = [(0, 100), (1, 99)]
        lc[cur - 2] = [(0, 99), (2, 101)]
        cov[cur].append((1, 120))
        cov[1].append((cur, 120))
    lp, li = ec._csr(loops)
    cp, cf = ec._csr(cov)
    lcp, lcf = ec._csr(lc)
    npts = P["P"]
    ref = rng.integers(0, N, npts)
    pos = np.zeros((npts, 3))
    for j in range(npts):
        pos[j] = ec.smap(ec.sinv(Scw[ref[j]]), rng.uniform(-1, 1, 3) + np.array([0, 0, 3.0]))
    corrected_by = np.full(npts, -1, np.int64)
    corrected_ref = np.full(npts, -1, np.int64)
    bad = (rng.uniform(size=npts) < 0.1).astype(np.uint8)
    for j in range(0, npts, 3):
        corrected_by[j] = ids[cur]
        corrected_ref[j] = ids[cur - (j // 3) % max(1, n_corr)]
    return dict(name=name, N=N, P=npts, cur=cur, loop=loop, min_weight=100, ids=ids, parent=parent,
                has_corr=has_corr, Scw=Scw, Snc=Snc, loop_ptr=lp, loop_idx=np.array(li, np.int32),
                cov_ptr=cp, cov_idx=np.array([c for c, _ in cf], np.int32), cov_w=np.array([w for _, w in cf], np.int32),
                lc_ptr=lcp, lc_idx=np.array([c for c, _ in lcf], np.int32), lc_w=np.array([w for _, w in lcf], np.int32),
                pos=pos, corrected_by=corrected_by, corrected_ref=corrected_ref, ref_kf=ids[ref], bad=bad,
                opts=dict(ec.default_options(), **P.get("opts", {})))
