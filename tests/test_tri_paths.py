"""The case table of tests/tri_cases.py on the CPU: the path restatement agrees with the oracle on
every case, every case reaches the paths it declares, and the table as a whole reaches every
path of the device search (csrc/tri_search.hip).  No GPU is used.
"""
import os
import re

import numpy as np
import pytest

from tests import tri_cases as tc
from tests.test_matcher import _oracle_tri

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "multicol-slam-annotation_amd", "csrc")


def _constexpr(fname, name):
    text = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "%s: no constexpr int %s" % (fname, name)
    return int(m.group(1))


def test_constants_are_the_kernels():
    """The restatement's copies of the tuning constants equal the sources': after a retune the path
    table has to be worked out again."""
    assert tc.K_TRI_SEG == _constexpr("tri_search.hip", "kTriSeg")
    assert tc.K_TRI_SUB == _constexpr("tri_search.hip", "kTriSub")
    assert tc.K_TRI_WIN == _constexpr("tri_search.hip", "kTriWin")
    assert tc.K_HAM_TILE == _constexpr("ham_dist.hpp", "kHamTile")
    assert _constexpr("ham_dist.hpp", "kHamThreads") == 256   # the query blocks of the tile cases


def oracle(name):
    c = tc.get(name)
    return _oracle_tri(c.d1, c.d2, c.cam1, c.cam2, c.has1, c.has2, c.r1, c.r2, c.E, c.thresh, c.m1, c.m2)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_reaches_its_paths(built, name):
    case = tc.get(name)
    _, declared, least = tc.CASES[name]
    assert case.th_low == (case.nbytes if case.masked else 2 * case.nbytes)
    assert tc._verdict_margin_ok(case) or case.seed is None
    reached, m12 = tc.reached(name)
    nref, ref = oracle(name)
    assert np.array_equal(m12, ref) and reached["matches"] == nref
    missing = [p for p in declared if reached[p] <= 0]
    assert not missing, "%s does not reach %s" % (name, missing)
    assert set(declared) <= set(tc.ALL_PATHS)
    assert nref >= least


def test_case_counts(built):
    """The per-case figures DESIGN 3.6 quotes, each a condition on the inputs."""
    r = lambda name: tc.reached(name)[0]
    p = r("mixed")
    assert (p["q_private_won"], p["q_private_nomatch"], p["q_flagged"], p["global_overflow"]) == (34, 6, 60, 0)
    assert p["seq_pair"] == 30 and p["seq_pair_second_sees_first_winner"] == 20
    p = r("multi_all_pass")
    assert (p["seq_multi_round"], p["seq_multi_best_in_later_round"], p["ens_next"]) == (70, 6, 13)
    assert r("multi_rare_pass")["seq_multi_winner_after_best_round"] == 9
    p = r("cap_over_only")
    assert (p["q_cap_over_only"], p["seq_rescan"], p["global_overflow"], p["q_private_won"]) == (2, 2, 0, 1)
    assert r("total_1024")["seq_rescan"] == 0 and r("total_1025")["q_cap_over_only"] == 2
    assert r("segment_96")["global_overflow"] == 0 and r("segment_97")["slot_overflow_pairs"] == 2
    p = r("window_jump")
    assert (p["ens_jump"], p["seq_pair_refused_span"]) == (1, 1)
    assert (r("tiles_4097")["tiles_per_seg_max"], r("tiles_4097")["segs_nonempty"]) == (2, 9)
    assert r("tiles_8193")["tiles_per_seg_max"] == 3 and r("tiles_15")["segs_nonempty"] == 1
    assert r("eight_cameras")["cams_with_flagged"] == 8
    p = r("eight_cameras_largest")
    assert p["lds_bytes"] == 128 * 1024 and p["tiles_per_seg_max"] == 128
    assert [r("entries_%d" % n)["ns"] for n in (0, 64, 65)] == [0, 64, 65]
    assert r("early_break")["seq_multi_early_break"] == 2
    assert np.array_equal(tc.reached("duplicates")[1][:3], [5, 7, 10])      # the lower index wins
    assert np.array_equal(tc.reached("listed_elsewhere")[1][:2], [4, 9])
    assert tc.reached("best_zero")[1].tolist() == [-1, -1, -1, -1, -1, -1, -1, 33]


def test_cases_cover_every_path(built):
    seen = set()
    for name in tc.CASES:
        reached, _ = tc.reached(name)
        seen |= {p for p in tc.ALL_PATHS if reached[p] > 0}
    uncovered = [p for p in tc.ALL_PATHS if p not in seen]
    assert not uncovered, "no case reaches %s" % uncovered


def test_older_random_fixtures_flag_nothing(built):
    """What the case table is for: the random fixtures of tests/test_matcher.py send no query to
    the ordered pass and never walk a second tile."""
    from tests.test_matcher import _tri_problem
    p, _ = tc.paths(tc.from_arrays(*_tri_problem(0), 0.3))
    assert (p["ns"], p["global_overflow"], p["tiles_per_seg_max"]) == (0, 0, 1)
