"""Second stage of the pyramid unit planner: strips of frames of one mask side by side in a
wave (pack_pyr_units, csrc/pyr_units.cpp) and the rule that puts frames into groups
(csrc/pyr_groups.hpp); DESIGN 3.1b.

CPU: tests/cpp/pyr_packed_check.cpp restates the kernel's bounds and the grouping rule and
checks the planner against them, plain and under AddressSanitizer / UBSan as a stand-alone
program.  Cases: the three Lafida masks and no mask at 754x480 (8 levels, 1.2), the small
320x240 masks of test_pyr_mask_units.py at (1.2, 3) and (2.0, 2), and 333x205 frames, whose
stride is no multiple of 4, so the levels that read the input must keep one run per wave.
GPU: batches of 1, 2, 5 and 2 G + 1 = 9 frames of 320x240 over the three disc masks of that
file, with mask indices in several orders, bit-exact against the oracle after a batch of noise
filled the workspace; the stages of every frame where its mask is set; a 333x205 batch; and a
batch of 513 such frames, whose grouping on the device crosses the waves and the rounds of
k_pyr_groups.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import oracle_bind as ob
from tests.test_pyr_mask_units import (CONFIGS, CSRC, H, NFEAT, ROOT, W, _Batch, _bits, _cpu_cases,
                                       _disc, _frames, _masks, _same)

GROUPS = (2, 4, 8)


def _cases():
    cases = [(n, mk, s, nl, 0) for n, mk, s, nl in _cpu_cases()]
    cases.append(("nomask", np.zeros((480, 754), np.uint8), 1.2, 8, 1))
    cases.append(("odd_1.2", np.zeros((205, 333), np.uint8), 1.2, 3, 1))
    cases.append(("odd_2", np.zeros((205, 333), np.uint8), 2.0, 2, 1))
    return cases


def _build_and_run(tmp_path, name, flags):
    assert shutil.which("hipcc"), "no hipcc"
    exe = str(tmp_path / name)
    # host code only; extractor_plan.cpp pulls the HIP runtime header in for its types
    subprocess.check_call(["hipcc", "--offload-host-only", "-x", "hip", "-std=c++17", *flags,
                           os.path.join(ROOT, "tests", "cpp", "pyr_packed_check.cpp"),
                           os.path.join(CSRC, "pyr_units.cpp"),
                           os.path.join(CSRC, "extractor_plan.cpp"), "-o", exe])
    cases = _cases()
    inp = tmp_path / (name + ".in")
    with open(inp, "wb") as f:
        for _, mk, s, nl, nomask in cases:
            f.write(np.array([mk.shape[1], mk.shape[0], nl, _bits(s), nomask], np.uint32).tobytes())
            f.write(np.ascontiguousarray(mk).tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("ok cases %d" % len(cases)), r.stdout[-2000:]
    assert "sort ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    waves = {}      # case -> G -> [(unpacked per frame, packed per group) per level]
    for ln in r.stdout.split("\n"):
        f = ln.split()
        if f and f[0] == "waves":
            waves.setdefault(cases[int(f[1])][0], {}).setdefault(int(f[2]), []).append((int(f[4]), int(f[5])))
    return waves


def test_packed_waves_cover_the_units_and_keep_the_bounds(tmp_path):
    waves = _build_and_run(tmp_path, "pyr_packed_check", ["-O2"])
    for name in ["lafida0", "lafida1", "lafida2", "nomask"]:
        for G in GROUPS:
            lv = waves[name][G]
            print("%s G=%d waves per frame and level, unpacked:" % (name, G), [u for u, _ in lv],
                  "packed:", [round(p / G, 2) for _, p in lv],
                  "total %d -> %.1f" % (sum(u for u, _ in lv), sum(p for _, p in lv) / G))
            assert sum(p for _, p in lv) < G * sum(u for u, _ in lv), (name, G)
    # a frame stride that is no multiple of 4: the input's readers (level-0 blur, level 1) keep
    # one run per wave (the program also requires it of every such level)
    for name in ["odd_1.2", "odd_2"]:
        for G in GROUPS:
            lv = waves[name][G]
            assert all(p == G * u for u, p in lv[:2]), (name, G, lv)


def test_packed_waves_sanitized(tmp_path):
    """The same stand-alone program built with ASan + UBSan, run directly."""
    _build_and_run(tmp_path, "pyr_packed_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
NF = 9      # 2 G + 1 frames for groups of G = 4
# mask indices by batch size: interleaved, all equal, sorted, with -1 and 7 (clamped to 0 and 2)
ORDERS = {
    1: [[2]],
    2: [[1, 1], [2, 0]],
    5: [[0, 1, 2, 1, 0], [1, 1, 1, 1, 1]],
    9: [[0, 1, 2, 0, 1, 2, 0, 1, 2], [1] * 9, [0, 0, 0, 0, 0, 1, 2, 2, 2], [2, -1, 7, 0, 1, 7, -1, 1, 0]],
}


class _Ref:
    """Inputs of one configuration and its oracle outputs per (frame, mask), computed on first
    use and left unchanged."""

    def __init__(self, scale, nlevels, w=W, h=H, masks=None):
        self.scale, self.nlevels, self.w, self.h = scale, nlevels, w, h
        from mcs_amd import synth
        if (w, h) == (W, H):
            self.imgs = np.concatenate([_frames(40), _frames(60)[:NF - 5]])
            self.masks = _masks()
        else:
            self.imgs = np.stack([synth.fisheye_frame(w, h, seed=80 + k)[0] for k in range(4)] +
                                 [synth.random_frame(w, h, 89)])
            self.masks = masks
        self.noise = np.stack([synth.random_frame(w, h, 70 + k) for k in range(len(self.imgs))])
        self._out, self._pyr = {}, {}

    def expect(self, f, m):
        """m: mask number or None"""
        if (f, m) not in self._out:
            self._out[(f, m)] = ob.extract(self.imgs[f], None if m is None else self.masks[m],
                                           nfeatures=NFEAT, scale=self.scale, nlevels=self.nlevels)
        return self._out[(f, m)]

    def pyramid(self, f):
        if f not in self._pyr:
            self._pyr[f] = ob.pyramid(self.imgs[f], self.nlevels, self.scale)
        return self._pyr[f]


_REFS = {}


def _ref(scale, nlevels):
    if (scale, nlevels) not in _REFS:
        _REFS[(scale, nlevels)] = _Ref(scale, nlevels)
    return _REFS[(scale, nlevels)]


class _SizedBatch(_Batch):
    """_Batch for another frame size"""

    def __init__(self, scale, nlevels, w, h, F):
        import torch
        import mcs_amd
        p = mcs_amd.ExtractorParams(nfeatures=NFEAT, scale_factor=scale, nlevels=nlevels)
        self.ex = mcs_amd.Extractor(p, w, h, max_frames=F)
        self.torch, self.mcs, self.F, self.cap = torch, mcs_amd, F, self.ex.capacity
        self.s = torch.cuda.current_stream().cuda_stream
        self.keep = []


def _clamped(midx):
    return [min(max(m, 0), 2) for m in midx]


def _masked_after_noise(b, ref, midx):
    """A no-mask batch of noise fills every byte of the workspaces; the masked batch after it
    must equal the oracle (a pixel no wave wrote, or one stored into another frame, differs)."""
    F = len(midx)
    b.set_masks(None)
    b.run(ref.noise[:F])
    b.set_masks(ref.masks)
    got = b.run(ref.imgs[:F], np.array(midx, np.int32))
    _same(got, [ref.expect(f, m) for f, m in enumerate(_clamped(midx))], "midx %s" % (midx,))


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", CONFIGS)
@pytest.mark.parametrize("F", sorted(ORDERS))
def test_packed_batches_bitexact_after_noise(gpu, scale, nlevels, F):
    ref = _ref(scale, nlevels)
    b = _Batch(scale, nlevels, F=NF)
    for midx in ORDERS[F]:
        _masked_after_noise(b, ref, midx)
    b.ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", CONFIGS)
def test_no_index_and_no_masks(gpu, scale, nlevels):
    """Masks registered but no index: every frame takes mask 0.  No masks registered: whole
    levels, groups of consecutive frames."""
    ref = _ref(scale, nlevels)
    b = _Batch(scale, nlevels, F=NF)
    b.set_masks(None)
    b.run(ref.noise)
    b.set_masks(ref.masks)
    _same(b.run(ref.imgs), [ref.expect(f, 0) for f in range(NF)], "no index")
    b.set_masks(None)
    for F in (NF, 5, 2, 1):
        b.run(ref.noise[:F])
        _same(b.run(ref.imgs[:F]), [ref.expect(f, None) for f in range(F)], "no masks, %d frames" % F)
    b.ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", CONFIGS)
def test_groups_rebuilt_per_call_and_stages_of_every_frame(gpu, scale, nlevels):
    """The same extractor twice in a row with two index orders (the group table of the first
    call must not survive), then stages 0 and 1 of every frame wherever its level's mask is
    set: a run stored into the wrong frame of its group shows here."""
    ref = _ref(scale, nlevels)
    b = _Batch(scale, nlevels, F=NF)
    b.set_masks(None)
    b.run(ref.noise)
    b.set_masks(ref.masks)
    first, second = ORDERS[NF][2], ORDERS[NF][0]
    _same(b.run(ref.imgs, np.array(first, np.int32)), [ref.expect(f, m) for f, m in enumerate(first)], "first order")
    _same(b.run(ref.imgs, np.array(second, np.int32)), [ref.expect(f, m) for f, m in enumerate(second)], "second order")
    for f in range(NF):
        mk = ob.mask_pyramid(ref.masks[second[f]], nlevels, scale)
        pyr = ref.pyramid(f)
        for l in range(nlevels):
            on = mk[l] != 0
            assert np.array_equal(b.ex.read_stage(0, f, l)[on], pyr[l][on]), (f, l)
            assert np.array_equal(b.ex.read_stage(1, f, l)[on], ob.box_blur5(pyr[l])[on]), (f, l)
    b.ex.close()


@pytest.mark.gpu
def test_odd_frame_stride_keeps_one_run_per_wave(gpu):
    """333x205 frames: the input's stride is no multiple of 4, so the level-0 blur and level 1
    stay unpacked while level 2 packs; masked and unmasked, bit-exact."""
    w, h = 333, 205
    masks = np.stack([_disc(w, h, 166, 102, 140), _disc(w, h, 250, 150, 100),
                      _disc(w, h, 80, 100, 65) | _disc(w, h, 250, 100, 60)])
    ref = _Ref(1.2, 3, w, h, masks)
    b = _SizedBatch(1.2, 3, w, h, 5)
    midx = [0, 1, 2, 1, 0]
    _masked_after_noise(b, ref, midx)
    b.set_masks(None)
    _same(b.run(ref.imgs), [ref.expect(f, None) for f in range(5)], "no masks")
    b.ex.close()


NBIG = 513      # the flagship's batch: three rounds of 256 frames, four waves each, in k_pyr_groups


def _big_orders():
    rng = np.random.RandomState(5)
    return {"interleaved": np.arange(NBIG) % 3,
            "random": rng.randint(0, 3, NBIG),
            "clamped": rng.randint(-2, 8, NBIG),          # -2, -1 -> mask 0; 3 .. 7 -> mask 2
            "long runs": np.repeat([2, 0, 1, 0], [200, 70, 143, 100])}


@pytest.mark.gpu
def test_grouping_beyond_one_wave_and_one_round(gpu):
    """513 small frames over three masks: the frames' ranks in k_pyr_groups cross its waves (64
    frames) and its rounds (256 frames).  Five distinct images tiled over the batch keep the
    oracle to 15 extractions; every frame is compared bit for bit after a batch of noise, so a
    frame sorted into a group of another mask, into two groups or into none differs."""
    scale, nlevels = CONFIGS[0]
    ref = _ref(scale, nlevels)
    pick = np.arange(NBIG) % 5
    imgs, noise = ref.imgs[pick], ref.noise[(pick + 2) % 5]
    b = _Batch(scale, nlevels, F=NBIG)
    for name, midx in _big_orders().items():
        midx = midx.astype(np.int32)
        b.set_masks(None)
        b.run(noise)
        b.set_masks(ref.masks)
        got = b.run(imgs, midx)
        exp = [ref.expect(int(pick[f]), m) for f, m in enumerate(_clamped(midx.tolist()))]
        _same(got, exp, name)
    b.ex.close()


@pytest.mark.gpu
def test_more_masks_than_the_grouping_kernel_counts_in_lds(gpu):
    """260 registered masks (the three discs, repeated): k_pyr_groups keeps its counters in the
    extractor's scratch buffer past 256 masks, and the tables stay per mask."""
    scale, nlevels = CONFIGS[1]
    ref = _ref(scale, nlevels)
    nm = 260
    b = _Batch(scale, nlevels, F=NF)
    b.set_masks(None)
    b.run(ref.noise)
    b.set_masks(ref.masks[np.arange(nm) % 3])
    midx = np.array([259, 0, 130, 257, 1, 258, 300, 130, 2], np.int32)
    exp = [ref.expect(f, min(int(m), nm - 1) % 3) for f, m in enumerate(midx)]
    _same(b.run(ref.imgs, midx), exp, "260 masks")
    b.ex.close()
