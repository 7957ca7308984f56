"""Keyframe database on the device (include/mcs_kfdb.h) against the restatement tests/np_kfdb.py,
all EXACT: candidates and their order, the shared-word counts, the scores as raw 64-bit patterns,
the min score and the six members after every call.  No tolerance: every quantity is an integer or
a double produced by + - / fabs in a stated order, correctly rounded on both sides.
"""
import os

import numpy as np
import pytest

from tests import kfdb_cases as kc
from tests import np_kfdb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "small_orb_omni_voc_9_6.npz")
GUARD = 8
CASES = kc.all_cases()


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device="cuda:0")


def _guarded(n, dtype, fill):
    import torch
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda:0")


def _query(word, value):
    """Device query whose buffers are longer than the count (the count is device data)."""
    from mcs_amd import kfdb
    import torch
    n = len(word)
    w = torch.full((n + 3,), 0x7FFFFFFF, dtype=torch.int32, device="cuda:0")
    v = torch.full((n + 3,), 7.0, dtype=torch.float64, device="cuda:0")
    w[:n] = _t(np.asarray(word, np.uint32).view(np.int32))
    v[:n] = _t(value, np.float64)
    cnt = _t([n], np.int32)
    return kfdb.query_of(w, v, cnt), (w, v, cnt)


class DevDB:
    """np_kfdb.Database's interface on mcs_amd.kfdb.  Every output buffer carries GUARD sentinel
    elements behind it, checked when the result is read."""

    def __init__(self, n_words, max_keyframes=512, max_entries=40000):
        from mcs_amd import kfdb
        self.k = kfdb
        self.db = kfdb.KeyFrameDatabase(int(n_words), max_keyframes, max_entries)
        self.last_min = None   # (host value, device tensor)

    def add(self, word, value, reloc_score_init=0.0):
        n = len(word)
        w = _t(np.asarray(word, np.uint32).view(np.int32)) if n else _t(np.zeros(1, np.int32))
        v = _t(value, np.float64) if n else _t(np.zeros(1))
        return self.db.add_device(w, v, _t([n], np.int32), n_upper=n, reloc_score_init=reloc_score_init)

    def erase(self, slot):
        self.db.erase(slot)

    def members(self):
        return self.db.members()

    def min_score(self, qw, qv, slots):
        import torch
        q, keep = _query(qw, qv)
        out = _guarded(1, torch.float64, -3.0)
        s = _t(slots, np.int32) if len(slots) else torch.zeros(0, dtype=torch.int32, device="cuda:0")
        self.db.min_score_device(q, s, out)
        h = out.cpu().numpy()
        assert np.all(h[1:] == -3.0)
        self.last_min = (float(h[0]), out)
        return float(h[0])

    def _launch(self, loop, qw, qv, query_id, connected, min_score, neigh, cap=None):
        import torch
        n = len(self.db)
        cap = n if cap is None else cap
        q, keep = _query(qw, qv)
        bufs = {"candidates": _guarded(cap, torch.int32, -77), "n_candidates": _guarded(1, torch.int32, -77),
                "common": _guarded(n, torch.int32, -77), "score": _guarded(n, torch.float64, -3.0)}
        res = self.k.Result(bufs["candidates"].data_ptr(), cap, bufs["n_candidates"].data_ptr(),
                            bufs["common"].data_ptr(), bufs["score"].data_ptr())
        ng = _t(neigh, np.int32)
        if loop:
            if self.last_min is not None and np.float64(min_score).tobytes() == np.float64(self.last_min[0]).tobytes():
                ms = self.last_min[1]          # the previous call's device double, no upload
            else:
                ms = _t([min_score], np.float64)
            cn = _t(connected, np.uint8)
            self.db.detect_loop_device(q, query_id, cn, ms, ng, res)
            keep = keep + (cn, ms)
        else:
            self.db.detect_reloc_device(q, query_id, ng, res)
        return {"bufs": bufs, "keep": keep + (ng,), "cap": cap, "n": n}

    @staticmethod
    def _read(pending):
        b, cap, n = pending["bufs"], pending["cap"], pending["n"]
        h = {k: t.cpu().numpy() for k, t in b.items()}
        nc = int(h["n_candidates"][0])
        assert np.all(h["candidates"][cap:] == -77) and np.all(h["n_candidates"][1:] == -77)
        assert np.all(h["common"][n:] == -77) and np.all(h["score"][n:] == -3.0)
        assert np.all(h["candidates"][min(nc, cap):cap] == -77)
        return {"candidates": h["candidates"][:min(nc, cap)], "n_candidates": nc, "common": h["common"][:n],
                "score": h["score"][:n]}

    def detect_loop(self, qw, qv, query_id, connected, min_score, neigh):
        return self._read(self._launch(True, qw, qv, query_id, connected, min_score, neigh))

    def detect_reloc(self, qw, qv, query_id, neigh):
        return self._read(self._launch(False, qw, qv, query_id, None, None, neigh))


@pytest.fixture(scope="module")
def expected():
    """The restatement's records per scenario, computed once."""
    return {c["name"]: kc.run(np_kfdb.Database(), c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_restatement(gpu, expected, case):
    kc.same(kc.run(DevDB(case["n_words"]), case), expected[case["name"]])


def test_back_to_back_without_synchronisation(gpu):
    """Two detect calls and a min-score call queued on one stream, read only afterwards."""
    import torch
    case = kc.case_random(65, 31)
    adds = [op for op in case["ops"] if op[0] == "add"]
    loop = next(op for op in case["ops"] if op[0] == "loop" and op[3] == 5)
    reloc = next(op for op in case["ops"] if op[0] == "reloc")
    ref, dev = np_kfdb.Database(), DevDB(729)
    for op in adds:
        ref.add(*op[1:])
        dev.add(*op[1:])
    slots = np.flatnonzero(loop[4]).tolist()
    q, keep = _query(loop[1], loop[2])
    dmin = _guarded(1, torch.float64, -3.0)
    dev.db.min_score_device(q, _t(slots, np.int32), dmin)
    dev.last_min = (0.0, dmin)
    p1 = dev._launch(True, loop[1], loop[2], 5, loop[4], 0.0, loop[6])
    p2 = dev._launch(False, reloc[1], reloc[2], 7, None, None, reloc[4])
    got1, got2 = dev._read(p1), dev._read(p2)
    ms = ref.min_score(loop[1], loop[2], slots)
    assert np.float64(ms).tobytes() == dmin.cpu().numpy()[:1].tobytes()
    e1 = ref.detect_loop(loop[1], loop[2], 5, loop[4], ms, loop[6])
    e2 = ref.detect_reloc(reloc[1], reloc[2], 7, reloc[4])
    for got, exp in ((got1, e1), (got2, e2)):
        assert got["candidates"].tolist() == list(exp["candidates"])
        assert np.array_equal(got["common"], exp["common"])
        assert np.array_equal(got["score"].view(np.uint64), exp["score"].view(np.uint64))
    m, em = dev.members(), ref.members()
    for k in em:
        assert m[k].tobytes() == em[k].tobytes(), k


def test_candidate_capacity(gpu):
    """More candidates than cap: the count is reported, the first cap are written, guards intact."""
    case = kc.case_random(301, 23)
    ref, dev = np_kfdb.Database(), DevDB(729)
    for op in case["ops"]:
        if op[0] == "add":
            ref.add(*op[1:])
            dev.add(*op[1:])
    reloc = next(op for op in case["ops"] if op[0] == "reloc")
    exp = ref.detect_reloc(reloc[1], reloc[2], 7, reloc[4])
    assert len(exp["candidates"]) > 2
    got = dev._read(dev._launch(False, reloc[1], reloc[2], 7, None, None, reloc[4], cap=2))
    assert got["n_candidates"] == len(exp["candidates"])
    assert got["candidates"].tolist() == list(exp["candidates"][:2])


def test_add_capacity_writes_nothing(gpu):
    from mcs_amd import MCS_ERR_CAPACITY, McsError
    rng = np.random.default_rng(3)
    dev, ref = DevDB(729, max_keyframes=2, max_entries=100), np_kfdb.Database()
    pool = np.arange(0, 200)
    a, b, c = kc.rand_bow(rng, pool, 60), kc.rand_bow(rng, pool, 60), kc.rand_bow(rng, pool, 40)
    assert dev.add(*a) == 0
    with pytest.raises(McsError) as e:
        dev.add(*b)                       # 60 + 60 > 100 entries
    assert e.value.code == MCS_ERR_CAPACITY and len(dev.db) == 1
    assert dev.add(*c) == 1               # the refused add consumed neither a slot nor entries
    with pytest.raises(McsError) as e:
        dev.add(*c)                       # a third keyframe
    assert e.value.code == MCS_ERR_CAPACITY and len(dev.db) == 2
    ref.add(*a)
    ref.add(*c)
    q = kc.rand_bow(rng, pool, 80)
    ng = kc.NO_NEIGH(2)
    got, exp = dev.detect_reloc(q[0], q[1], 1, ng), ref.detect_reloc(q[0], q[1], 1, ng)
    assert got["candidates"].tolist() == list(exp["candidates"])
    assert np.array_equal(got["score"].view(np.uint64), exp["score"].view(np.uint64))
    dev.db.clear()
    assert len(dev.db) == 0 and dev.add(*b) == 0


def test_unsupported_scoring_and_malformed_input(gpu):
    from mcs_amd import MCS_ERR_UNSUPPORTED, McsError, kfdb, vocab
    v = vocab.Vocabulary(vocab.synthetic(k=9, L=3, scoring=vocab.L2_NORM))
    with pytest.raises(McsError) as e:
        kfdb.KeyFrameDatabase(v, 4, 100)
    assert e.value.code == MCS_ERR_UNSUPPORTED
    # neighbour ids, slot lists and a device count outside their ranges are clamped, not followed
    import torch
    dev = DevDB(729, max_keyframes=4, max_entries=64)
    w, val = np.array([3, 9, 700], np.uint32), np.array([0.5, 0.25, 0.25])
    dev.add(w, val)
    dev.add(w, val)
    ng = np.full((2, 10), 1 << 30, np.int32)
    ng[1, :] = -(1 << 30)
    qv = np.array([0.25, 0.5, 0.25])                                              # every score is 0.75
    keep = (_t(w.view(np.int32)), _t(qv), _t([1 << 30], np.int32))               # count above the buffer
    q = kfdb.query_of(*keep)
    res, ts = kfdb.new_result(2, 2)
    dev.db.detect_reloc_device(q, 1, _t(ng), res)
    assert ts["n_candidates"].cpu().tolist() == [2] and ts["candidates"].cpu().tolist() == [0, 1]
    assert ts["common"].cpu().tolist() == [3, 3] and ts["score"].cpu().tolist() == [0.75, 0.75]
    out = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    dev.db.min_score_device(q, _t([-5, 1 << 30, 1], np.int32), out)
    assert out.cpu().tolist() == [0.75]


def _features(voc, n, seed, n_src):
    """Descriptors drawn around a few vocabulary leaves, so that keyframes share words."""
    rng = np.random.default_rng(seed)
    leaves = voc["desc"][np.searchsorted(voc["node_id"], voc["word_node"][:n_src])]
    src = leaves[rng.integers(0, len(leaves), size=n)].copy()
    bits = np.unpackbits(src, axis=1)
    for r in range(bits.shape[0]):
        bits[r, rng.integers(0, 256, size=3)] ^= 1
    return np.packbits(bits, axis=1)


@pytest.mark.parametrize("real", [False, True], ids=["synthetic", "lafida_voc"])
def test_end_to_end_from_descriptors(gpu, real):
    """descriptors -> transform_words_device -> bow_vector_device -> add_device x N ->
    min_score_device -> detect_loop_device, all on one stream; the device BowVector must equal the
    host transform's bit for bit, the candidates the restatement's."""
    import torch
    from mcs_amd import bow_match, kfdb, vocab
    vd = vocab.load_npz(FIXTURE) if real else vocab.synthetic(k=9, L=3)
    order = np.argsort(vd["node_id"])
    vs = dict(vd, node_id=vd["node_id"][order], parent_id=vd["parent_id"][order], weight=vd["weight"][order],
              desc=vd["desc"][order])
    v = vocab.Vocabulary(vd)
    n_words = v.info()["n_words"]
    if not real:
        assert n_words == 729
    N, nd = 8, 300
    ws = bow_match.Workspace(nd, 1)
    db = kfdb.KeyFrameDatabase(v, N, N * nd)
    ref = np_kfdb.Database()
    keep = []
    descs = [_features(vs, nd, 40 + i, 400) for i in range(N + 1)]
    descs[2] = descs[2][:1]                                  # a keyframe of one descriptor
    bows = []
    for i, d in enumerate(descs):
        t = _t(d, np.uint8)
        word, weight, node = v.transform_words(t, 4)
        bw, bv, bn = v.bow_vector(ws, word, weight)
        keep.append((t, word, weight, node, bw, bv, bn))
        bows.append((bw, bv, bn))
        if i < N:
            assert db.add_device(bw, bv, bn, n_upper=len(d)) == i
    rng = np.random.default_rng(9)
    ng = kc.rand_neigh(rng, N)
    conn = np.zeros(N, np.uint8)
    conn[[1, 5]] = 1
    qb = bows[N]
    q = kfdb.query_of(*qb)
    dmin = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    db.min_score_device(q, _t([1, 5], np.int32), dmin)
    res, ts = kfdb.new_result(N, N)
    db.detect_loop_device(q, 100, _t(conn), dmin, _t(ng), res)
    # expected: the host transform's BowVector (mcs_vocab_transform), then the restatement
    host = []
    for i, d in enumerate(descs):
        bow, _ = v.transform(d, 4)
        hw = np.array(sorted(bow), np.uint32)
        hv = np.array([bow[k] for k in sorted(bow)], np.float64)
        bw, bv, bn = bows[i]
        m = int(bn.cpu()[0])
        assert m == len(hw), i
        assert np.array_equal(bw.cpu().numpy()[:m].view(np.uint32), hw), i
        assert bv.cpu().numpy()[:m].tobytes() == hv.tobytes(), i
        host.append((hw, hv))
        if i < N:
            ref.add(hw, hv)
    ms = ref.min_score(host[N][0], host[N][1], [1, 5])
    assert np.float64(ms).tobytes() == dmin.cpu().numpy().tobytes()
    exp = ref.detect_loop(host[N][0], host[N][1], 100, conn, ms, ng)
    nc = int(ts["n_candidates"].cpu()[0])
    assert ts["candidates"].cpu().numpy()[:nc].tolist() == list(exp["candidates"])
    assert np.array_equal(ts["common"].cpu().numpy()[:N], exp["common"])
    assert ts["score"].cpu().numpy()[:N].tobytes() == exp["score"].tobytes()
    assert max(exp["common"]) > 0


@pytest.mark.parametrize("weighting,scoring", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 5), (2, 5)])
def test_bow_vector_matches_host_transform(gpu, weighting, scoring):
    """mcs_bow_vector_device against mcs_vocab_transform's bow_* for every evaluation path, with
    repeated words (w + w + ... + w) and stopped words."""
    from mcs_amd import bow_match, vocab
    vd = vocab.synthetic(k=4, L=2, seed=3, stop_frac=0.3, weighting=weighting, scoring=scoring)
    v = vocab.Vocabulary(vd)
    rng = np.random.default_rng(weighting * 7 + scoring)
    ws = bow_match.Workspace(2500, 1)
    for n in (1, 64, 2500):
        d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        word, weight, node = v.transform_words(_t(d, np.uint8), 1)
        bw, bv, bn = v.bow_vector(ws, word, weight)
        bow, _ = v.transform(d, 1)
        m = int(bn.cpu()[0])
        assert m == len(bow)
        assert bw.cpu().numpy()[:m].view(np.uint32).tolist() == sorted(bow)
        assert bv.cpu().numpy()[:m].tobytes() == np.array([bow[k] for k in sorted(bow)]).tobytes()


def test_host_entries(gpu):
    """The host-buffer forms against the restatement."""
    case = kc.case_random(65, 22)
    ref, dev = np_kfdb.Database(), DevDB(729)
    for op in case["ops"]:
        if op[0] == "add":
            ref.add(*op[1:])
            dev.add(*op[1:])
    loop = next(op for op in case["ops"] if op[0] == "loop" and op[3] == 5)
    slots = np.flatnonzero(loop[4]).tolist()
    ms = dev.db.min_score(loop[1], loop[2], slots)
    assert np.float64(ms).tobytes() == np.float64(ref.min_score(loop[1], loop[2], slots)).tobytes()
    got = dev.db.detect_loop(loop[1], loop[2], 5, loop[4], ms, loop[6])
    exp = ref.detect_loop(loop[1], loop[2], 5, loop[4], ms, loop[6])
    assert got["candidates"].tolist() == list(exp["candidates"]) and not got["capacity_exceeded"]
    assert got["score"].tobytes() == exp["score"].tobytes() and np.array_equal(got["common"], exp["common"])
    got = dev.db.detect_reloc(loop[1], loop[2], 6, loop[6])
    exp = ref.detect_reloc(loop[1], loop[2], 6, loop[6])
    assert got["candidates"].tolist() == list(exp["candidates"])
    m, em = dev.members(), ref.members()
    for k in em:
        assert m[k].tobytes() == em[k].tobytes(), k
