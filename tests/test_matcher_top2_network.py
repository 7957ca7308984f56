"""The matcher's best / second-best update takes four keys at a time (csrc/top2_net.hpp: five
min3 / med3 instructions instead of eight min / med3).  Which of the five a key passes through
depends on where its train row sits: the register of the triple or the single, the group, the
lane half, the sub-tile.  So every place meets every other, as the best and as the second best.

Train k has the bits of group k set (a group is `gw` adjacent bits) and nothing else; the query
for (i, j) has group i set and all but one bit of group j.  Its distances are gw - 1 to train i,
gw + 1 to train j and 3 gw - 1 to every other train, so i must come out best and j second.  With
group j set in full both are at distance gw, and the lower index must win.

CPU: tests/cpp/top2_net_check.cpp, exhaustive over small values, plain and under
AddressSanitizer / UBSan as a stand-alone program.
GPU: all four outputs of mcs_hamming_top2_device against a numpy brute force, exact.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "top2_net_check.cpp")
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", *flags, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok single 27984 chain 4200000"), r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_update_exhaustive(tmp_path):
    """Every (k1 <= k2, a, b, c, d) over 0..5 against sorting; 16 keys chained against the scan."""
    _build_and_run(tmp_path, "top2_net_check", ["-O2"])


def test_update_exhaustive_sanitized(tmp_path):
    """The same stand-alone program built with ASan + UBSan, run directly."""
    _build_and_run(tmp_path, "top2_net_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _trains(n, nbytes, gw):
    assert n * gw <= 8 * nbytes
    bits = np.zeros((n, 8 * nbytes), np.uint8)
    for k in range(n):
        bits[k, k * gw:(k + 1) * gw] = 1
    return np.packbits(bits, axis=1, bitorder="little")


def _queries(pairs, nbytes, gw, tie):
    """One query per (i, j): group i set, group j set but for its last bit (in full if tie);
    j < 0: group i alone."""
    bits = np.zeros((len(pairs), 8 * nbytes), np.uint8)
    for n, (i, j) in enumerate(pairs):
        bits[n, i * gw:(i + 1) * gw] = 1
        if j >= 0:
            bits[n, j * gw:(j + 1) * gw - (0 if tie else 1)] = 1
    return np.packbits(bits, axis=1, bitorder="little")


def _brute(q, t):
    """(best_idx, best_dist, second_idx, second_dist) of the reference scan: the two smallest
    (distance, train index); -1 and 8 * bytes + 1 where there is no such train."""
    nbytes = q.shape[1]
    dist = np.zeros((len(q), len(t)), np.int32)
    for k in range(nbytes):
        dist += _POP[q[:, k, None] ^ t[None, :, k]]
    order = np.argsort(dist, axis=1, kind="stable")
    rows = np.arange(len(q))
    out = [np.full(len(q), -1, np.int32), np.full(len(q), 8 * nbytes + 1, np.int32),
           np.full(len(q), -1, np.int32), np.full(len(q), 8 * nbytes + 1, np.int32)]
    for rank in range(min(2, len(t))):
        out[2 * rank] = order[:, rank].astype(np.int32)
        out[2 * rank + 1] = dist[rows, order[:, rank]]
    return out


def _device_top2(q, t):
    import torch
    import mcs_amd
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(t)).cuda()
    out = [torch.full((len(q),), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    rc = mcs_amd.lib().mcs_hamming_top2_device(dq.data_ptr(), len(q), dt.data_ptr(), len(t),
                                               q.shape[1], *[o.data_ptr() for o in out],
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(q, t):
    got, exp = _device_top2(q, t), _brute(q, t)
    for name, g, e in zip(("best_idx", "best_dist", "second_idx", "second_dist"), got, exp):
        assert np.array_equal(g, e), (name, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    return exp


def _check_places(pairs, nt, nbytes, gw, tie):
    """Run the pairs and assert that (i, j) are the winners the case was built for."""
    q, t = _queries(pairs, nbytes, gw, tie), _trains(nt, nbytes, gw)
    bi, bd, si, sd = _check(q, t)
    p = np.array(pairs, np.int32).reshape(-1, 2)
    two = p[:, 1] >= 0
    if tie:
        lo = np.where(two, np.minimum(p[:, 0], p[:, 1]), p[:, 0])
        hi = np.where(two, np.maximum(p[:, 0], p[:, 1]), -1)
        assert np.array_equal(bi, lo) and np.array_equal(si[two], hi[two])
        assert np.all(bd[two] == gw) and np.all(sd[two] == gw)
    else:
        assert np.array_equal(bi, p[:, 0]) and np.array_equal(si[two], p[two, 1])
        assert np.all(bd[two] == gw - 1) and np.all(sd[two] == gw + 1)
    assert np.all(bd[~two] == 0)
    if nt > 1:   # a lone target: the second is the lowest other train, at distance 2 gw
        assert np.array_equal(si[~two], np.where(p[~two, 0] == 0, 1, 0)) and np.all(sd[~two] == 2 * gw)
    else:
        assert np.all(si[~two] == -1) and np.all(sd[~two] == 8 * nbytes + 1)


def _ordered_pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


@pytest.mark.gpu
@pytest.mark.parametrize("tie", [False, True])
def test_places_one_subtile(gpu, tie):
    """nq = 992, nt = 64: every ordered pair of places of the first 32-train sub-tile."""
    pairs = _ordered_pairs(32)
    assert len(pairs) == 992
    _check_places(pairs, 64, 32, 4, tie)


@pytest.mark.gpu
@pytest.mark.parametrize("tie", [False, True])
def test_places_two_subtiles(gpu, tie):
    """One winner in sub-tile 0 and the other in sub-tile 1, both ways round: the running keys
    are re-based between the two."""
    pairs = [(i, 32 + j) for i in range(32) for j in range(32)]
    pairs += [(32 + j, i) for i in range(32) for j in range(32)]
    _check_places(pairs, 64, 32, 4, tie)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 33, 35])
def test_places_partial_tile(gpu, nt):
    """The rows past nt get the none key before the update; these counts end a group after its
    first, second and third register and after the single, in the first and the second sub-tile."""
    pairs = _ordered_pairs(nt) + [(i, -1) for i in range(nt)]
    _check_places(pairs, nt, 32, 4, False)
    _check_places(pairs, nt, 32, 4, True)


@pytest.mark.gpu
def test_unkeyed_8200(gpu):
    """nt = 8200 > 2^13 takes the unkeyed instantiation (key = dist << 16 | train).  Random trains
    (about 128 bits apart); train j is train i with 6 bits flipped, the query train i with one other
    bit flipped (distances 1 and 7), or with 3 of the 6 flipped (3 and 3: the lower index wins)."""
    rng = np.random.default_rng(5)
    nt = 8200
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    places = np.concatenate([np.arange(0, 40), np.arange(120, 136), np.arange(8150, 8200),
                             rng.choice(np.arange(200, 8100), 94, replace=False)])
    places = rng.permutation(places)
    assert len(places) == 200 and len(set(places.tolist())) == 200
    pi, pj = places[:100], places[100:]
    q = np.empty((200, 32), np.uint8)
    for n, (i, j) in enumerate(zip(pi, pj)):
        bits = rng.choice(256, 7, replace=False)
        tj = t[i].copy()
        for b in bits[:6]:
            tj[b >> 3] ^= np.uint8(1 << (b & 7))
        t[j] = tj
        q[n] = t[i]
        q[n, bits[6] >> 3] ^= np.uint8(1 << (bits[6] & 7))
        q[100 + n] = t[i]
        for b in bits[:3]:
            q[100 + n, b >> 3] ^= np.uint8(1 << (b & 7))
    bi, bd, si, sd = _check(q, t)
    assert np.array_equal(bi[:100], pi) and np.array_equal(si[:100], pj)
    assert np.all(bd[:100] == 1) and np.all(sd[:100] == 7)
    assert np.array_equal(bi[100:], np.minimum(pi, pj)) and np.array_equal(si[100:], np.maximum(pi, pj))
    assert np.all(bd[100:] == 3) and np.all(sd[100:] == 3)


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes,nt,gw", [(16, 39, 2), (64, 67, 4)])
def test_places_other_widths(gpu, nbytes, nt, gw):
    """k_top2<W> (16- and 64-byte descriptors): groups of four trains and a tail of three taken
    one at a time; more than one block of queries."""
    pairs = _ordered_pairs(nt) + [(i, -1) for i in range(nt)]
    assert len(pairs) > 512
    _check_places(pairs, nt, nbytes, gw, False)
    _check_places(pairs, nt, nbytes, gw, True)
