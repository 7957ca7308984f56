"""csrc/omni_geom.hpp, the one definition of the camera and pose math, pinned to the oracle on the
CPU.  tests/cpp/omni_geom_host.cpp exports the header's host functions; compiled with
g++ -O2 -ffp-contract=off they are compared BIT FOR BIT (tobytes) with the oracle's independent
restatement (tests/oracle_bind.py), where both sides call the same libm atan:

  WorldToImg / ImgToWorld   both forms (mcs_cam_model at its degree, the packed cam[17]) against
                            cam_world_to_img / cam_img_to_world, on the three Lafida cameras and on
                            a model with fewer terms than the packed form holds
  edge_error                the BA's computeError through the shared pieces against ba_edge
  compute_e / epi_check     a rig's table against compute_e_rig, the verdict against
                            check_dist_epipolar_line, den == 0 included
  horner                    a polynomial equals itself padded with zeros to 12 terms, the fact
                            that lets the two WorldToImg forms share one body

The -Wall -Werror build is also the proof that the header is clean host C++.  No GPU is needed.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mcs_amd import CamModel, synth
from mcs_amd.ba_synth import cam_vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_D = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_D)


@pytest.fixture(scope="module")
def og(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("omni_geom") / "libomni_geom_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "omni_geom_host.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.og_horner.restype = ctypes.c_double
    lib.og_horner.argtypes = [_D, ctypes.c_int, ctypes.c_double]
    lib.og_epi_check.argtypes = [_D, _D, _D, ctypes.c_double]
    return lib


def _short_cam():
    """Fewer terms than the Lafida models: p_deg 4 < 5, invp_deg 7 < 12."""
    cam = dict(synth.LAFIDA_CAMS[1])
    cam["a"], cam["pol"] = cam["a"][:4], cam["pol"][:7]
    return cam


CAMS = [("lafida0", synth.LAFIDA_CAMS[0]), ("lafida1", synth.LAFIDA_CAMS[1]), ("lafida2", synth.LAFIDA_CAMS[2]),
        ("short", _short_cam())]


def _points(rng, n):
    """|X| from 1e-3 to 50 in every direction (half of them behind the camera, z > 0 or < 0), then
    the axis x = y = 0, x = -0.0 and y = -0.0."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    X = d * np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n))[:, None]
    special = [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-0.0, 0.0, 2.0], [-0.0, 1.0, -2.0], [1.0, -0.0, 0.5],
               [-0.0, -0.0, -3.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 0.0, -0.0], [1e-3, 0.0, 50.0]]
    return np.ascontiguousarray(np.vstack([X, special]))


@pytest.mark.parametrize("name,cam", CAMS, ids=[c[0] for c in CAMS])
def test_world_to_img_both_forms_equal_the_oracle(built, og, name, cam):
    from tests import oracle_bind as ob
    m, X = CamModel.from_dict(cam), _points(np.random.default_rng(11), 1000)
    n = len(X)
    ref = np.array([ob.cam_world_to_img(m, *x) for x in X])
    assert np.isfinite(ref).all()
    got_m, got_p = np.zeros((n, 2)), np.zeros((n, 2))
    og.og_world_to_img_model(ctypes.byref(m), n, _p(X), _p(got_m))
    camv = np.zeros(17)                       # the packed form: zero padded to 12 terms
    camv[:5 + len(cam["pol"])] = cam_vec(cam)
    og.og_world_to_img_packed(_p(camv), n, _p(X), _p(got_p))
    assert got_m.tobytes() == ref.tobytes()
    assert got_p.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name,cam", CAMS, ids=[c[0] for c in CAMS])
def test_img_to_world_equals_the_oracle(built, og, name, cam):
    from tests import oracle_bind as ob
    rng = np.random.default_rng(12)
    m = CamModel.from_dict(cam)
    uv = np.column_stack([rng.uniform(-50, 800, 1000), rng.uniform(-50, 530, 1000)])
    uv = np.ascontiguousarray(np.vstack([uv, [[cam["u0"], cam["v0"]], [0.0, 0.0], [-0.0, 5.0]]]))
    ref = np.array([ob.cam_img_to_world(m, u, v) for u, v in uv])
    got = np.zeros((len(uv), 3))
    og.og_img_to_world(ctypes.byref(m), len(uv), _p(uv), _p(got))
    assert got.tobytes() == ref.tobytes()


def test_edge_error_through_the_shared_pieces_equals_the_oracle(built, og):
    from tests import oracle_bind as ob
    rng = np.random.default_rng(13)
    cases = []
    for k in range(600):
        c = k % 3
        pose = np.concatenate([rng.normal(scale=0.4, size=3), rng.normal(scale=2.0, size=3)])
        mc = np.array(synth.LAFIDA_MC[c]) if k % 2 else np.concatenate([rng.normal(scale=0.8, size=3),
                                                                          rng.normal(scale=0.2, size=3)])
        X = pose[3:] + rng.normal(size=3) * np.exp(rng.uniform(np.log(1e-3), np.log(50.0)))
        cases.append((pose, X, mc, c))
    z6 = np.zeros(6)                          # identity rig and pose: signed zeros in every product
    cases += [(z6, np.array([0.0, 0.0, 1.0]), z6, 0), (z6, np.array([-0.0, 0.0, -1.0]), z6, 1),
              (z6, np.array([1.0, -2.0, 3.0]), np.array(synth.LAFIDA_MC[2]), 2),
              (np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0]), np.zeros(3), z6, 0)]
    for pose, X, mc, c in cases:
        camv = cam_vec(synth.LAFIDA_CAMS[c])
        meas = np.array([400.0 + 7 * c, 240.0 - 3 * c])
        ref = ob.ba_edge(pose, X, mc, camv, meas)[0]
        a = [np.ascontiguousarray(v, np.float64) for v in (pose, X, mc, camv, meas)]
        got = np.zeros(2)
        og.og_edge_error(*[_p(v) for v in a], _p(got))
        assert np.isfinite(ref).all()
        assert got.tobytes() == ref.tobytes(), (pose, X, mc, c, got, ref)


def test_compute_e_and_epi_check_equal_the_oracle(built, og):
    from tests import oracle_bind as ob
    rng = np.random.default_rng(14)
    mc = np.ascontiguousarray(synth.LAFIDA_MC, np.float64)
    for k in range(40):
        mt1 = np.concatenate([rng.normal(scale=0.5, size=3), rng.normal(scale=1.5, size=3)])
        mt2 = mt1 + np.concatenate([rng.normal(scale=0.05, size=3), rng.normal(scale=0.3, size=3)])
        ref = ob.compute_e_rig(mt1, mt2, mc)
        got = np.zeros((3, 3, 3, 3))
        og.og_compute_e_rig(_p(mt1), _p(mt2), _p(mc), 3, _p(got))
        assert np.isfinite(ref).all()
        assert got.tobytes() == ref.tobytes()
        for _ in range(25):
            r1, r2 = rng.normal(size=3), rng.normal(size=3)
            r1, r2 = r1 / np.linalg.norm(r1), r2 / np.linalg.norm(r2)
            E = np.ascontiguousarray(ref[rng.integers(3), rng.integers(3)])
            # thresholds on both sides of the distance, so both verdicts occur
            ok, dsqr = ob.check_dist_epipolar_line(r1, r2, E, 1e-2)
            for th in (1e-2, dsqr * 0.5, dsqr * 2.0):
                assert bool(og.og_epi_check(_p(r1), _p(r2), _p(E), th)) == ob.check_dist_epipolar_line(r1, r2, E, th)[0]
    # den == 0: a zero E, and rays in the null spaces of E and of its transpose
    r = np.array([0.0, 0.0, 1.0])
    for E in (np.zeros((3, 3)), np.diag([1.0, 1.0, 0.0])):
        ok, dsqr = ob.check_dist_epipolar_line(r, r, E, 1e-2)
        assert not ok and np.isnan(dsqr)
        assert og.og_epi_check(_p(r), _p(r), _p(np.ascontiguousarray(E)), 1e-2) == 0


def test_horner_ignores_zero_padding(og):
    rng = np.random.default_rng(15)
    xs = np.concatenate([rng.normal(scale=s, size=200) for s in (1e-3, 1.0, 50.0)] + [[0.0, -0.0, 1.0, -1.5707963267948966]])
    for d in (1, 4, 5, 7, 11, 12):
        c = rng.normal(scale=30.0, size=d)
        pad = np.zeros(12)
        pad[:d] = c
        for x in xs:
            a, b = og.og_horner(_p(c), d, float(x)), og.og_horner(_p(pad), 12, float(x))
            assert np.float64(a).tobytes() == np.float64(b).tobytes(), (d, x, a, b)
