"""Keyframe database, CPU side.

  * tests/np_kfdb.py (the plain Python restatement: inverted file, lists and members as in the text)
    reproduces tests/golden/kfdb_ref.npz exactly: the fixture is what the reference TEXT of
    cMultiKeyFrameDatabase / L1Scoring::score / the DetectLoop minScore loop computes on the
    scenarios of tests/kfdb_cases.py (tests/golden/gen_kfdb_ref.py), numbers only.
  * every scenario contains the case it is named after.
  * the restatement's BowVector equals oracle/vocab_oracle's.
  * ABI: symbols, MCS_ERR_ARG / MCS_ERR_UNSUPPORTED before any device use, MCS_ERR_NO_DEVICE here.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import kfdb_cases as kc
from tests import np_kfdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
CASES = kc.all_cases()
FIELDS = {"min": ("min_score",),
          "loop": ("candidates", "common", "score", "loop_query", "loop_words", "loop_score", "reloc_query",
                   "reloc_words", "reloc_score")}
FIELDS["reloc"] = FIELDS["loop"]


@pytest.fixture(scope="module")
def records():
    return {c["name"]: kc.run(np_kfdb.Database(), c) for c in CASES}


def load_golden(name):
    """The fixture's records of one scenario, in kfdb_cases.run's form."""
    z = np.load(GOLDEN)
    kinds = [("min", "loop", "reloc")[k] for k in z[name + "/kinds"].tolist()]
    recs = []
    for i, kind in enumerate(kinds):
        r = {"kind": kind}
        for f in FIELDS[kind]:
            a = z["%s/%d/%s" % (name, i, f)]
            r[f] = np.float64(a) if f == "min_score" else a
        recs.append(r)
    return recs


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference_text(records, case):
    """Candidate lists, word counts, every score bit for bit and the members after each call."""
    kc.same(records[case["name"]], load_golden(case["name"]))


def _rec(records, name, kind, nth=0):
    return [r for r in records[name] if r["kind"] == kind][nth]


def test_scenarios_contain_their_cases(records):
    # accScore == 0.75 * bestAccScore exactly is NOT retained (strict >): slot 0 scores 0.375 = 0.75 * 0.5
    for kind in ("reloc", "loop"):
        r = _rec(records, "retain_exact", kind)
        assert r["score"].tolist() == [0.375, 0.5, 0.40625] and r["candidates"].tolist() == [1, 2]
        assert r["score"][0] == 0.75 * r["score"][1]
    # si == minScore exactly is kept (>=)
    assert _rec(records, "min_score_equal", "min")["min_score"] == 0.5
    r = _rec(records, "min_score_equal", "loop")
    assert r["score"][0] == 0.5 and r["candidates"].tolist() == [0, 2]
    # dedupe: slots 0 and 2 both stand behind slot 3, named once at its first list position
    assert _rec(records, "dedupe", "reloc")["candidates"].tolist() == [3, 1]
    assert _rec(records, "dedupe", "loop")["candidates"].tolist() == [3, 1]
    # stale reloc_score: slot 2 keeps the first query's score and it keeps slot 1 out
    r1, r2 = _rec(records, "stale_reloc", "reloc", 0), _rec(records, "stale_reloc", "reloc", 1)
    assert r2["common"].tolist() == [10, 9, 1] and r2["reloc_query"].tolist() == [2, 2, 2]
    assert r2["reloc_score"][2] == r1["reloc_score"][2] == r1["score"][2] and r2["score"][2] != r2["reloc_score"][2]
    assert r2["score"][1] > 0.75 * r2["score"][0]                                  # retained without it
    assert not r2["score"][1] > 0.75 * (r2["score"][0] + r2["reloc_score"][2])    # but not with it
    assert r2["candidates"].tolist() == [0]
    # connected keyframes: not listed, loop_query unchanged, loop_words ends at 1
    r = _rec(records, "connected", "loop")
    assert r["common"][1] > 1 and r["loop_words"].tolist()[1::2][:2] == [1, 1] and r["loop_query"][1] == 0
    assert r["loop_query"][0] == 4 and r["loop_words"][0] == r["common"][0]
    # query id 0 against fresh members: nothing listed, the words are still counted
    r = _rec(records, "random65", "loop", 0)
    assert len(r["candidates"]) == 0 and np.array_equal(r["loop_words"], r["common"]) and r["common"].max() > 0
    # the repeated id: nothing listed, loop_words += common for the listed ones
    a, b = _rec(records, "random65", "loop", 1), _rec(records, "random65", "loop", 2)
    assert len(a["candidates"]) > 0 and len(b["candidates"]) == 0
    listed = a["loop_query"] == 5
    assert listed.any() and np.array_equal(b["loop_words"][listed], 2 * a["common"][listed])
    # an erased keyframe in the middle shares nothing afterwards
    r = _rec(records, "random301", "reloc", 1)
    assert r["common"][150] == 0 and r["common"][100] == 0 and (r["common"] > 0).sum() > 250
    assert len(_rec(records, "random301", "loop", 1)["candidates"]) > 1
    # lengths 0, 1, 63, 64, 65, 129 with shared words at positions 0, 63, 64 and last; no shared word
    r = _rec(records, "lengths", "loop")
    assert r["common"].tolist() == [0, 1, 2, 2, 3, 4, 0]
    assert _rec(records, "lengths", "reloc", 1)["common"].tolist() == [0, 0, 0, 0, 0, 1, 0]   # one-word query
    assert len(_rec(records, "lengths", "reloc", 2)["candidates"]) == 0                       # empty query


def test_l1_score_walk_equals_the_plain_sum():
    rng = np.random.default_rng(1)
    pool = np.arange(0, 200)
    for _ in range(20):
        (w1, v1), (w2, v2) = kc.rand_bow(rng, pool, 60), kc.rand_bow(rng, pool, 90)
        s = 0.0
        d2 = dict(zip(w2.tolist(), v2.tolist()))
        for w, v in zip(w1.tolist(), v1.tolist()):
            if w in d2:
                s += abs(v - d2[w]) - abs(v) - abs(d2[w])
        assert np_kfdb.l1_score(w1.tolist(), v1.tolist(), w2.tolist(), v2.tolist()) == -s / 2.0


@pytest.mark.parametrize("weighting,scoring", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 5), (2, 5)])
def test_restatement_bow_vector_equals_the_oracle(built, weighting, scoring):
    """The expected value of mcs_bow_vector_device is the host bow_* of mcs_vocab_transform; on the
    CPU the same evaluation is oracle/vocab_oracle's, and the restatement's BowVector equals it."""
    from mcs_amd import vocab
    from tests import oracle_bind as ob
    vd = vocab.synthetic(k=4, L=2, seed=3, stop_frac=0.3, weighting=weighting, scoring=scoring)
    rng = np.random.default_rng(weighting * 7 + scoring)
    for n in (0, 1, 64, 700):
        d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        word, weight, _ = ob.vocab_words(vd, d, 1)
        bow, _ = ob.vocab_transform(vd, d, 1)
        bw, bv = np_kfdb.bow_vector(word, weight, weighting, scoring)
        assert bw.tolist() == sorted(bow)
        assert bv.tobytes() == np.array([bow[k] for k in sorted(bow)], np.float64).tobytes()
        if n == 700:
            assert len(bw) < 16 and (weight <= 0).any()      # repeated words and stopped words


# ----------------------------------------------------------------------------- ABI

SYMBOLS = ["mcs_bow_vector_device", "mcs_kfdb_create", "mcs_kfdb_create_n", "mcs_kfdb_destroy", "mcs_kfdb_size",
           "mcs_kfdb_add_device", "mcs_kfdb_add", "mcs_kfdb_erase", "mcs_kfdb_clear", "mcs_kfdb_min_score_device",
           "mcs_kfdb_detect_loop_device", "mcs_kfdb_detect_reloc_device", "mcs_kfdb_members_device",
           "mcs_kfdb_min_score", "mcs_kfdb_detect_loop", "mcs_kfdb_detect_reloc"]


def test_symbols_exported(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in mcs_amd.SIGNATURES, s


def test_argument_errors_come_before_any_device_use(built):
    import mcs_amd
    from mcs_amd import MCS_ERR_ARG, MCS_ERR_UNSUPPORTED
    L = mcs_amd.lib()
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert L.mcs_kfdb_create_n(0, 729, 0, 0, 100, out) == MCS_ERR_ARG          # capacity of 0
    assert L.mcs_kfdb_create_n(0, 729, 0, 4, 0, out) == MCS_ERR_ARG
    assert L.mcs_kfdb_create_n(0, -1, 0, 4, 100, out) == MCS_ERR_ARG
    assert L.mcs_kfdb_create_n(0, 729, 0, 4, 100, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_create_n(0, 729, 7, 4, 100, out) == MCS_ERR_ARG          # no such scoring type
    for scoring in (1, 2, 3, 4, 5):                                             # a vocabulary that is not L1
        assert L.mcs_kfdb_create_n(0, 729, scoring, 4, 100, out) == MCS_ERR_UNSUPPORTED
        assert b"L1" in L.mcs_last_error()
    assert L.mcs_kfdb_create(0, None, 4, 100, out) == MCS_ERR_ARG
    assert h.value is None
    # null database / buffers, negative counts
    w, v = np.zeros(4, np.uint32), np.zeros(4, np.float64)
    i4, d1 = np.zeros(40, np.int32), np.zeros(1, np.float64)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert L.mcs_kfdb_min_score(None, p(w), p(v), 4, p(i4), 1, p(d1)) == MCS_ERR_ARG
    assert L.mcs_kfdb_detect_loop(None, p(w), p(v), 4, 1, None, 0.0, p(i4), p(i4), 4, p(i4), None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_detect_reloc(None, p(w), p(v), -1, 1, p(i4), p(i4), 4, p(i4), None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_add_device(None, None, None, None, 0, 0.0, None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_add(None, p(w), p(v), 4, 0.0, p(i4)) == MCS_ERR_ARG
    assert L.mcs_kfdb_erase(None, 0, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_clear(None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_min_score_device(None, None, None, 0, None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_detect_loop_device(None, None, 0, None, None, None, None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_detect_reloc_device(None, None, 0, None, None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_members_device(None, None, None, None, None, None, None, None) == MCS_ERR_ARG
    assert L.mcs_bow_vector_device(None, None, None, None, 0, None, None, None, None) == MCS_ERR_ARG
    assert L.mcs_kfdb_size(None) == 0
    L.mcs_kfdb_destroy(None)


def test_no_device_without_a_gpu(built):
    import mcs_amd
    if mcs_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    assert mcs_amd.lib().mcs_kfdb_create_n(0, 729, 0, 4, 100, ctypes.byref(h)) == mcs_amd.MCS_ERR_NO_DEVICE
    assert h.value is None
    from mcs_amd import kfdb
    with pytest.raises(mcs_amd.McsError) as e:
        kfdb.KeyFrameDatabase(729, 4, 100)
    assert e.value.code == mcs_amd.MCS_ERR_NO_DEVICE
