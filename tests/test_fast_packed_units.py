"""k_fast_rows waves hold one or two runs of cells (pack_fast_units): where a cell
row's last wave has lanes to spare, the head of the next cell row goes into them.

CPU: tests/cpp/fast_units_check.cpp requires of the packed waves what the kernel relies on
(every cell once, disjoint lanes that hold each run's halo, pairs on one level and equally high,
every load inside the level, cells within the per-lane counters), plain and under
AddressSanitizer / UBSan as a stand-alone program, and prints wave-bands per level before and
after.
GPU: shapes at which the planner pairs runs (the CPU test asserts that it does), bit-exact
against the oracle per level (read_stage 2) and in the final keypoints and descriptors:
  401x300, 3 levels: level 0 with odd pitch and 32-row cells (rows 32 apart sit alike in their
           dwords), level 1 with aligned pitch; the last cell row has its own height
  333x205, 2 levels: odd pitch and 33-row cells, so consecutive cell rows sit differently in
           their dwords and the planner pairs none on level 0: the case the kernel's one uniform
           byte shift per row relies on
  320x240 with the registered disc masks of test_pyr_mask_units.py (ragged live ranges), once
           over a stale workspace
and FAST types 12 and 8, thresholds 0 and 1 on noise (full lists, every cell counter busy), and
block ties across the lane boundary between two runs.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import oracle_bind as ob
from tests.test_pyr_mask_units import MIDX, _Batch, _bits, _disc, _masks, _ref, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam-annotation_amd", "csrc")
W, H = 320, 240


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def _cpu_cases():
    """(name, mask or None, W, H, scale, nlevels)"""
    from mcs_amd import synth
    cases = [("lafida%d" % c, synth.mirror_mask(synth.LAFIDA_CAMS[c]), 754, 480, 1.2, 8) for c in range(3)]
    cases.append(("nomask", None, 754, 480, 1.2, 8))
    cases.append(("401x300", None, 401, 300, 1.2, 3))
    cases.append(("333x205", None, 333, 205, 1.2, 2))
    m = _masks()
    half = np.zeros((H, W), np.uint8)
    half[:, :W // 2 - 7] = 255
    small = {"all255": np.full((H, W), 255, np.uint8), "all0": np.zeros((H, W), np.uint8),
             "halfplane": half, "disc150": m[0], "cutdisc": m[1], "twodiscs": m[2],
             "ring": _disc(W, H, 160, 120, 115) & ~_disc(W, H, 160, 120, 70)}
    for s, nl in [(1.2, 3), (2.0, 2)]:
        cases.append(("320x240_%g" % s, None, W, H, s, nl))
        for name, mk in small.items():
            cases.append(("%s_%g" % (name, s), mk, W, H, s, nl))
    return cases


def _build_and_run(tmp_path, name, flags):
    assert shutil.which("hipcc"), "no hipcc"
    exe = str(tmp_path / name)
    # host code only; extractor_plan.cpp pulls the HIP runtime header in for its types
    subprocess.check_call(["hipcc", "--offload-host-only", "-x", "hip", "-std=c++17", *flags,
                           os.path.join(ROOT, "tests", "cpp", "fast_units_check.cpp"),
                           os.path.join(CSRC, "extractor_plan.cpp"), "-o", exe])
    cases = _cpu_cases()
    inp = tmp_path / (name + ".in")
    with open(inp, "wb") as f:
        for _, mk, w, h, s, nl in cases:
            f.write(np.array([w, h, nl, _bits(s), 0 if mk is None else 1], np.uint32).tobytes())
            f.write(np.ascontiguousarray(np.zeros((h, w), np.uint8) if mk is None else mk).tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("ok cases %d" % len(cases)), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    wb = {}
    for ln in r.stdout.split("\n"):
        f = ln.split()
        if f and f[0] == "wb":    # (unpacked, packed, two-run waves) per level
            wb.setdefault(cases[int(f[1])][0], []).append((int(f[3]), int(f[4]), int(f[5])))
    return wb


def test_packed_waves_keep_the_kernel_bounds(tmp_path):
    wb = _build_and_run(tmp_path, "fast_units_check", ["-O2"])
    for name, rows in wb.items():
        print("%-14s wave-bands per level, unpacked/packed/two-run waves:" % name, rows)
        assert all(p <= u for u, p, _ in rows), name      # never more on any level
    for name in ("lafida0", "lafida1", "lafida2", "nomask"):
        unpacked, packed = (sum(r[i] for r in wb[name]) for i in (0, 1))
        print(name, "total", unpacked, "->", packed)
        assert packed < unpacked, name
    # the shapes of the GPU tests pair runs where their docstring says
    assert wb["401x300"][0][2] > 0 and wb["401x300"][1][2] > 0
    assert wb["401x300"][0][1] < wb["401x300"][0][0] and wb["401x300"][1][1] < wb["401x300"][1][0]
    assert wb["333x205"][0][2] == 0      # rows 33 x 333 bytes apart: never in one wave
    assert wb["320x240_1.2"][0][2] > 0 and wb["320x240_2"][0][2] > 0
    for name in ("disc150", "cutdisc", "twodiscs"):
        assert wb[name + "_1.2"][0][2] > 0 and wb[name + "_2"][0][2] > 0, name
    assert all(u == 0 and p == 0 for u, p, _ in wb["all0_1.2"])


def test_packed_waves_keep_the_kernel_bounds_sanitized(tmp_path):
    """The same stand-alone program built with ASan + UBSan, run directly."""
    _build_and_run(tmp_path, "fast_units_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
FAST_TH = 20


def _check(img, mask, scale, nlevels, th=FAST_TH, fast_type=2, nfeatures=500):
    """One frame through the single-call path: per-level candidates and the final output."""
    import mcs_amd
    h, w = img.shape
    p = mcs_amd.ExtractorParams(nfeatures=nfeatures, scale_factor=scale, nlevels=nlevels,
                                fast_threshold=th, fast_agast_type=fast_type)
    ex = mcs_amd.Extractor(p, w, h, max_frames=1)
    kps, desc = ex.extract(img, mask)
    lv = ob.pyramid(img, nlevels, scale)
    mk = ob.mask_pyramid(mask, nlevels, scale) if mask is not None else [None] * nlevels
    total = 0
    for l in range(nlevels):
        ref = ob.level_candidates(lv[l], mk[l], th, fast_type=fast_type)
        got = ex.read_stage(2, 0, l)
        assert got.shape == ref.shape, (l, got.shape, ref.shape)
        assert np.array_equal(got, ref), "FAST candidates differ at level %d" % l
        total += len(ref)
    okps, odesc = ob.extract(img, mask, nfeatures=nfeatures, scale=scale, nlevels=nlevels,
                             fast_th=th, fast_type=fast_type)
    assert len(kps) == len(okps), (len(kps), len(okps))
    assert np.array_equal(kps, okps) and np.array_equal(desc, odesc)
    ex.close()
    return total


SHAPES = [(401, 300, 3), (333, 205, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl", SHAPES)
@pytest.mark.parametrize("kind", ["fisheye", "fisheye_masked", "random"])
def test_packed_shapes_bitexact(gpu, w, h, nl, kind):
    from mcs_amd import synth
    if kind == "random":
        img, mask = synth.random_frame(w, h, seed=w), None
    else:
        img, mask = synth.fisheye_frame(w, h, seed=w + h)
        mask = mask if kind == "fisheye_masked" else None
    assert _check(img, mask, 1.2, nl) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("fast_type", [1, 0])
def test_packed_fast_types_12_and_8(gpu, fast_type):
    from mcs_amd import synth
    img, mask = synth.fisheye_frame(401, 300, seed=61 + fast_type)
    assert _check(img, mask, 1.2, 3, fast_type=fast_type) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl", SHAPES)
@pytest.mark.parametrize("th", [0, 1])
def test_packed_noise_full_lists(gpu, w, h, nl, th):
    """Nearly every pixel survives the pre-test and is a corner: full lists in both runs, and
    every cell counter of a two-run wave in use."""
    img = np.random.default_rng(11 + th).integers(0, 256, size=(h, w), dtype=np.uint8)
    n = _check(img, None, 1.2, nl, th=th, nfeatures=1000)
    assert n > (w - 50) * (h - 50) // 8    # the lists really are full


@pytest.mark.gpu
@pytest.mark.parametrize("period", [7, 5])
def test_packed_block_ties_across_the_run_boundary(gpu, period):
    """2x2 blocks every `period` px: four equal-score corners per block, which strict NMS drops;
    the blocks straddle cell borders and the lanes where one run's halo ends and the next run's
    begins, where a score of the other run must never be read as a neighbour."""
    y, x = np.mgrid[0:300, 0:401]
    img = np.where(((x % period) < 2) & ((y % period) < 2), 200, 40).astype(np.uint8)
    _check(img, None, 1.2, 3, th=10)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", [(1.2, 3), (2.0, 2)])
def test_packed_masked_batch_over_stale_workspace(gpu, scale, nlevels):
    """Ragged live ranges: the three registered disc masks, after an unmasked batch of noise has
    filled the workspaces; per-level candidates and the final output against the oracle."""
    from mcs_amd import synth
    imgs, masks, exp, _ = _ref(scale, nlevels)
    b = _Batch(scale, nlevels)
    b.set_masks(None)
    b.run(np.stack([synth.random_frame(W, H, 70 + k) for k in range(5)]))
    b.set_masks(masks)
    got = b.run(imgs, MIDX)
    for f in range(5):
        lv = ob.pyramid(imgs[f], nlevels, scale)
        mk = ob.mask_pyramid(masks[MIDX[f]], nlevels, scale)
        for l in range(nlevels):
            ref = ob.level_candidates(lv[l], mk[l], FAST_TH)
            assert np.array_equal(b.ex.read_stage(2, f, l), ref), (f, l)
    _same(got, exp, "masked, packed")
    b.ex.close()
