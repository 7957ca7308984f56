"""The device SearchForTriangulationRaw (csrc/tri_search.hip) on the case table of
tests/tri_cases.py, through the device-resident entry and the host entry: matches12 and the
count bit-equal to the oracle.  tests/test_tri_paths.py shows on the CPU which kernel paths each
case reaches.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tri_cases as tc
from tests.test_matcher import _oracle_tri, _p, _run_tri_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(c):
    return _oracle_tri(c.d1, c.d2, c.cam1, c.cam2, c.has1, c.has2, c.r1, c.r2, c.E, c.thresh, c.m1, c.m2)


def _device(ws, c):
    return _run_tri_device(ws, c.d1, c.d2, c.cam1, c.cam2, c.has1, c.has2, c.r1, c.r2, c.E, c.nbytes,
                           c.th_low, c.thresh, c.m1, c.m2)


def _host(c):
    import mcs_amd
    L = mcs_amd.lib()
    got = np.full(len(c.d1), -9, np.int32)
    nm = ctypes.c_int32(-9)
    if c.masked:
        rc = L.mcs_search_for_triangulation_raw_masked(
            _p(c.d1), _p(c.m1), _p(c.cam1), _p(c.has1), _p(c.r1), len(c.d1), _p(c.d2), _p(c.m2), _p(c.cam2),
            _p(c.has2), _p(c.r2), len(c.d2), c.ncams, _p(c.E), c.nbytes, c.th_low, c.thresh, _p(got),
            ctypes.byref(nm))
    else:
        rc = L.mcs_search_for_triangulation_raw(
            _p(c.d1), _p(c.cam1), _p(c.has1), _p(c.r1), len(c.d1), _p(c.d2), _p(c.cam2), _p(c.has2),
            _p(c.r2), len(c.d2), c.ncams, _p(c.E), c.nbytes, c.th_low, c.thresh, _p(got), ctypes.byref(nm))
    assert rc == 0, L.mcs_last_error()
    return nm.value, got


def _workspace(n1, n2):
    import mcs_amd
    ws = ctypes.c_void_p()
    assert mcs_amd.lib().mcs_tri_workspace_create(0, n1, n2, ctypes.byref(ws)) == 0
    return ws


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_matches_oracle(gpu, name):
    import mcs_amd
    c = tc.get(name)
    nref, ref = _oracle(c)
    assert nref >= tc.CASES[name][2]
    ws = _workspace(len(c.d1), len(c.d2))
    try:
        n, got = _device(ws, c)
    finally:
        mcs_amd.lib().mcs_tri_workspace_destroy(ws)
    bad = np.nonzero(got != ref)[0]
    assert n == nref and len(bad) == 0, "device entry: n %d vs %d, queries %s got %s want %s" % (
        n, nref, bad[:8], got[bad[:8]], ref[bad[:8]])
    n, got = _host(c)
    bad = np.nonzero(got != ref)[0]
    assert n == nref and len(bad) == 0, "host entry: n %d vs %d, queries %s got %s want %s" % (
        n, nref, bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.mark.gpu
def test_workspace_reuse_across_cases(gpu):
    """One workspace larger than every case, used for a slot-overflow case, then the mixed case,
    then an all-private one: cand / cnt / flag / overflow contents of the earlier call must not
    show in the later ones."""
    import mcs_amd
    ws = _workspace(1000, 1100)
    try:
        for name in ("segment_97", "shared_32", "mixed", "all_private", "segment_97"):
            c = tc.get(name)
            nref, ref = _oracle(c)
            n, got = _device(ws, c)
            assert n == nref and np.array_equal(got, ref), name
    finally:
        mcs_amd.lib().mcs_tri_workspace_destroy(ws)


def _host_growth_main():
    """Runs in a process of its own: the host entry's workspace cache starts empty there."""
    small = tc.build(8, 40, 1, [dict(cam=0, q=[0, 1, 2], t=[10, 5, 7, 20], tflip=(0, 9))])
    more_n1 = tc.build(300, 40, 1, [dict(cam=0, q=[0, 290, 299], t=[10, 5, 7, 39], tflip=(0, 9)),
                                    dict(cam=0, q=[150], t=[30], tflip=(0, 9))])
    more_n2 = tc.get("mixed")
    for c in (small, more_n1, more_n2, small):
        nref, ref = _oracle(c)
        n, got = _host(c)
        assert nref >= 3 and n == nref and np.array_equal(got, ref), (len(c.d1), len(c.d2), n, nref)
    print("host growth ok")


@pytest.mark.gpu
def test_host_entry_cache_growth(gpu):
    """The host entry keeps one workspace per device and regrows it: a small call, one with more
    queries, one with more KF2 rows, the small one again.  The cache lives as long as the process,
    so the sequence runs in a fresh one."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p] + [env.get("PYTHONPATH", "")])
    out = subprocess.run(
        [sys.executable, "-c", "from tests.test_tri_search_gpu import _host_growth_main as m; m()"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host growth ok" in out.stdout, out.stdout + out.stderr
