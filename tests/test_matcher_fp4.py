"""The 32-byte top-2 matcher on the FP4 matrix cores (`k_top2_mfma32`) against the oracle's
`oracle_hamming_top2`, exact integer equality.

The kernel expands a descriptor bit to one FP4 element and lets the block-scaled MFMA produce
the key 2^14 * Hamming + 2^13 + (train index relative to the sub-tile at hand) in f32, re-based
by -32.0f after every 32 trains.  What can go wrong there, and the case that shows it:
  * the A (train) and B (query) fragments disagree on where a descriptor bit sits -> one-hot
    descriptors, every bit against every bit;
  * a partial sum is not exact in f32 at the largest keys -> every distance 0..256 at train
    indices next to 0 and next to 8191, the largest index the keyed kernel takes;
  * the tie rule (lowest train index first) across sub-tile and tile boundaries;
  * ragged train / query counts, and the batch entry with per-set counts.
The oracle returns no second index, so that one is checked against a numpy restatement of the
same scan (stable sort by distance), which is itself compared with the oracle.
"""
import ctypes

import numpy as np
import pytest

from tests import oracle_bind as ob

pytestmark = pytest.mark.gpu

_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def _descs(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(d, bits):
    """d with the listed bit positions (0..255) flipped."""
    out = d.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _expected(q, t):
    """(best_idx, best_dist, second_idx, second_dist): the oracle's three arrays, plus the second
    index from a numpy restatement that must agree with the oracle on the other three."""
    bi, bd, sd = ob.hamming_top2(q, t)
    dist = np.zeros((len(q), len(t)), np.int32)
    for k in range(32):
        dist += _POP[q[:, k, None] ^ t[None, :, k]]
    order = np.argsort(dist, axis=1, kind="stable")
    rows = np.arange(len(q))
    assert np.array_equal(order[:, 0], bi) and np.array_equal(dist[rows, order[:, 0]], bd)
    if len(t) > 1:
        si = order[:, 1].astype(np.int32)
        assert np.array_equal(dist[rows, si], sd)
    else:
        si = np.full(len(q), -1, np.int32)
        assert np.all(sd == 257)
    return bi, bd, si, sd


def _device_top2(q, t):
    import torch
    import mcs_amd
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(t)).cuda()
    out = [torch.full((len(q),), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    rc = mcs_amd.lib().mcs_hamming_top2_device(dq.data_ptr(), len(q), dt.data_ptr(), len(t), 32,
                                               *[o.data_ptr() for o in out],
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(q, t):
    got = _device_top2(q, t)
    exp = _expected(q, t)
    for name, g, e in zip(("best_idx", "best_dist", "second_idx", "second_dist"), got, exp):
        assert np.array_equal(g, e), (name, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    return got


def _one_hot():
    d = np.zeros((256, 32), np.uint8)
    for i in range(256):
        d[i, i >> 3] = 1 << (i & 7)
    return d


@pytest.mark.parametrize("permuted", [False, True])
def test_fragment_map(gpu, permuted):
    """Query i has bit i alone, train j bit perm[j] alone: distance 0 where the bits meet, 2
    elsewhere.  A bit that the A and the B fragment place differently moves a zero."""
    q = _one_hot()
    perm = np.random.default_rng(11).permutation(256) if permuted else np.arange(256)
    t = q[perm]
    bi, bd, si, sd = _check(q, t)
    inv = np.argsort(perm)
    assert np.array_equal(bi, inv) and np.all(bd == 0) and np.all(sd == 2)
    assert np.array_equal(si, np.where(inv == 0, 1, 0))   # the lowest other index


def _ladder(q0, order):
    """257 descriptors at Hamming distance 0..256 from q0 (the bits of `order` flipped in turn)."""
    rows = np.empty((257, 32), np.uint8)
    cur = q0.copy()
    rows[0] = cur
    for d in range(256):
        cur = _flip(cur, [order[d]])
        rows[d + 1] = cur
    return rows


def test_every_distance_both_ends_of_key_range(gpu):
    """nt = 8192 (the largest keyed train count): trains 0..256 and 7935..8191 at distance
    0..256 from query 0, every train between at 256; the other queries random, so their
    winners fall anywhere among the ladders' rows."""
    rng = np.random.default_rng(21)
    q = _descs(64, 22)
    t = np.repeat((~q[0])[None, :], 8192, 0)
    t[:257] = _ladder(q[0], rng.permutation(256))
    t[7935:] = _ladder(q[0], rng.permutation(256))
    bi, bd, si, sd = _check(q, t)
    assert (bi[0], bd[0], si[0], sd[0]) == (0, 0, 7935, 0)


def test_every_distance_wins(gpu):
    """Each distance as a winning key, at the top of the index range and at the bottom.  Query d
    lies at distance d from T and 256 - d from ~T.  Trains: ~T everywhere, T in the last two
    rows -> for d < 128 the winners are 8190 / 8191 at distance d, for d > 128 rows 0 / 1 at
    256 - d.  Two more queries take the largest keys there are: every train at 256 (rows 0 / 1
    win), and rows 8190 / 8191 alone at 255."""
    T = _descs(1, 31)[0]
    q = np.concatenate([_ladder(T, np.random.default_rng(32).permutation(256)), _descs(2, 33)])
    t = np.repeat((~T)[None, :], 8192, 0)
    t[8190:] = T
    bi, bd, si, sd = _check(q, t)
    assert (bi[5], bd[5], si[5], sd[5]) == (8190, 5, 8191, 5)
    assert (bi[200], bd[200], si[200], sd[200]) == (0, 56, 1, 56)
    t = np.repeat((~q[257])[None, :], 8192, 0)
    bi, bd, si, sd = _check(q[257:258], t)
    assert (bi[0], bd[0], si[0], sd[0]) == (0, 256, 1, 256)
    t[8190] = _flip(t[8190], [3])
    t[8191] = _flip(t[8191], [250])
    bi, bd, si, sd = _check(q[257:258], t)
    assert (bi[0], bd[0], si[0], sd[0]) == (8190, 255, 8191, 255)


@pytest.mark.parametrize("first,second", [(31, 32), (63, 64), (127, 128), (5, 300), (128, 129), (255, 256)])
def test_ties(gpu, first, second):
    """Several trains at the same best distance: the lowest index wins and the next index at
    that distance is second, with the duplicates on either side of a 32-train sub-tile, a
    64-train and a 128-train tile boundary.  Query 1's best is unique and its second tied."""
    q = _descs(70, 41)
    t = _descs(400, 42)
    near = _flip(q[0], [7, 100, 201])
    for j in (first, second, 399):
        t[j] = near
    t[second + 2] = _flip(q[1], [9])
    for j in (second + 1, 390):
        t[j] = _flip(q[1], [1, 2, 3, 4])
    bi, bd, si, sd = _check(q, t)
    assert (bi[0], bd[0], si[0], sd[0]) == (first, 3, second, 3)
    assert (bi[1], bd[1], si[1], sd[1]) == (second + 2, 1, second + 1, 4)


@pytest.mark.parametrize("nt", [1, 31, 33, 63, 65, 127, 129, 257])
def test_ragged_edges(gpu, nt):
    """Train counts around the sub-tile (32) and tile (128) sizes, query counts around the
    workgroup's 256; with one train the second index is -1 and the second distance 257."""
    t = _descs(nt, 50 + nt)
    for nq in (1, 255, 257):
        q = _descs(nq, 60 + nq)
        q[0] = t[nt - 1]   # the last valid row wins somewhere
        bi, bd, si, sd = _check(q, t)
        assert bi[0] == (np.flatnonzero((t == t[nt - 1]).all(1))[0]) and bd[0] == 0
        if nt == 1:
            assert np.all(si == -1) and np.all(sd == 257) and np.all(bi == 0)


def test_batch_ragged_counts(gpu):
    """The batch entry: per-set counts around the tile sizes, a zero-count set on either side."""
    import torch
    import mcs_amd
    cap = 300
    counts = np.array([300, 129, 0, 33, 1, 257], np.int32)
    sets = np.zeros((len(counts), cap, 32), np.uint8)
    for s, n in enumerate(counts):
        sets[s, :n] = _descs(n, 70 + s)
        sets[s, n:] = 0xA5   # rows past the count are not part of the set
    sets[5, :129] = sets[1, :129]
    pairs = np.array([[0, 5], [5, 0], [1, 5], [3, 4], [4, 3], [2, 0], [0, 2], [5, 1], [4, 4]], np.int32)
    d = torch.from_numpy(sets).cuda()
    dc = torch.from_numpy(counts).cuda()
    dp = torch.from_numpy(pairs).cuda()
    out = [torch.full((len(pairs), cap), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    rc = mcs_amd.lib().mcs_hamming_top2_batch_device(d.data_ptr(), dc.data_ptr(), dp.data_ptr(),
                                                     len(pairs), cap, 32,
                                                     *[o.data_ptr() for o in out], None)
    assert rc == 0
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out]
    for p, (qs, ts) in enumerate(pairs):
        nq, nt = counts[qs], counts[ts]
        if nq == 0:
            continue
        if nt == 0:   # no train: the oracle's empty scan
            bi, bd, sd = ob.hamming_top2(sets[qs, :nq], sets[ts, :0])
            exp = (bi, bd, np.full(nq, -1, np.int32), sd)
            assert np.all(bi == -1) and np.all(bd == 257) and np.all(sd == 257)
        else:
            exp = _expected(sets[qs, :nq], sets[ts, :nt])
        for g, e in zip(got, exp):
            assert np.array_equal(g[p, :nq], e)
    for g in got:   # nothing written past a pair's query count
        for p, (qs, _) in enumerate(pairs):
            assert np.all(g[p, counts[qs]:] == -7)
