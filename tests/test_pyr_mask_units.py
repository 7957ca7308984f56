"""With registered masks the pyramid kernel computes a level only where an output can depend on
it (csrc/pyr_units.cpp): per mask, a table of strips x row segments.

CPU: tests/cpp/pyr_units_check.cpp simulates on its own which pixels can reach an output and
requires the planner's units to cover them, to keep the kernel's bounds, and to be today's
strips x segments without a mask; plain and under AddressSanitizer / UBSan, as a stand-alone
program.
GPU: a 5-frame batch over three registered masks at 320x240 (3 levels at 1.2, and 2 levels at
2.0 for the wide kernel instantiation), bit-exact against the oracle, also with a workspace
full of noise from an earlier batch; the stages where the mask is set; an empty and a full mask;
and the full geometry again after the masks are dropped.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import oracle_bind as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam-annotation_amd", "csrc")
W, H, NFEAT = 320, 240, 500
CONFIGS = [(1.2, 3), (2.0, 2)]


def _disc(w, h, cx, cy, r):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x - cx) ** 2 + (y - cy) ** 2 < r * r, 255, 0).astype(np.uint8)


def _masks():
    """The three registered masks of the GPU tests: a centred disc of radius 150 (wider than
    one strip, cut by the top and bottom borders), a disc cut by the right and bottom borders,
    two discs separated by a dead band."""
    return np.stack([_disc(W, H, 160, 120, 150), _disc(W, H, 250, 180, 110),
                     _disc(W, H, 80, 120, 70) | _disc(W, H, 245, 120, 65)])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def _bits(scale):
    return int(np.array(scale, np.float32).view(np.uint32))


def _cpu_cases():
    from mcs_amd import synth
    cases = [("lafida%d" % c, synth.mirror_mask(synth.LAFIDA_CAMS[c]), 1.2, 8) for c in range(3)]
    small = {"all255": np.full((H, W), 255, np.uint8), "all0": np.zeros((H, W), np.uint8)}
    pts = np.zeros((H, W), np.uint8)
    for x, y in [(26, 26), (W - 27, 26), (26, H - 27), (W - 27, H - 27), (W // 2, H // 2)]:
        pts[y, x] = 255      # inside the first / last FAST cell of the first / last cell row
    small["points"] = pts
    half = np.zeros((H, W), np.uint8)
    half[:, :W // 2 - 7] = 255
    small["halfplane"] = half
    m = _masks()
    small["twodiscs"] = m[2]
    small["ring"] = _disc(W, H, 160, 120, 115) & ~_disc(W, H, 160, 120, 70)
    small["cutdisc"] = m[1]
    small["disc150"] = m[0]
    for name, mk in small.items():
        for s, nl in CONFIGS:
            cases.append(("%s_%g" % (name, s), mk, s, nl))
    return cases


def _build_and_run(tmp_path, name, flags):
    assert shutil.which("hipcc"), "no hipcc"
    exe = str(tmp_path / name)
    # host code only; extractor_plan.cpp pulls the HIP runtime header in for its types
    subprocess.check_call(["hipcc", "--offload-host-only", "-x", "hip", "-std=c++17", *flags,
                           os.path.join(ROOT, "tests", "cpp", "pyr_units_check.cpp"),
                           os.path.join(CSRC, "pyr_units.cpp"),
                           os.path.join(CSRC, "extractor_plan.cpp"), "-o", exe])
    cases = _cpu_cases()
    inp = tmp_path / (name + ".in")
    with open(inp, "wb") as f:
        for _, mk, s, nl in cases:
            f.write(np.array([mk.shape[1], mk.shape[0], nl, _bits(s), 0], np.uint32).tobytes())
            f.write(np.ascontiguousarray(mk).tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("ok cases %d" % len(cases)), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    waves = {}
    for ln in r.stdout.split("\n"):
        f = ln.split()
        if f and f[0] == "waves":
            waves.setdefault(cases[int(f[1])][0], []).append((int(f[5]), int(f[6])))
    return waves


def test_units_cover_every_influence(tmp_path):
    waves = _build_and_run(tmp_path, "pyr_units_check", ["-O2"])
    for c in range(3):      # the wave counts per level at 256 frames
        print("lafida%d full/masked per level:" % c, waves["lafida%d" % c])
        full, masked = (sum(v[i] for v in waves["lafida%d" % c]) for i in (0, 1))
        assert masked < full
    assert all(m == 0 for _, m in waves["all0_1.2"]) and all(m == 0 for _, m in waves["all0_2"])
    # the disc cut by the borders leaves the far corner of every level out
    assert all(m < f for f, m in waves["cutdisc_1.2"])


def test_units_cover_every_influence_sanitized(tmp_path):
    """The same stand-alone program built with ASan + UBSan, run directly."""
    _build_and_run(tmp_path, "pyr_units_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
MIDX = np.array([0, 1, 2, 1, 0], np.int32)


def _frames(seed0):
    from mcs_amd import synth
    imgs = [synth.fisheye_frame(W, H, seed=seed0 + k)[0] for k in range(4)]
    imgs.append(synth.random_frame(W, H, seed0 + 9))     # many weak corners everywhere
    return np.stack(imgs)


class _Batch:
    """One extractor and its device buffers; run(imgs, midx) -> per frame (kps, desc)."""

    def __init__(self, scale, nlevels, F=5):
        import torch
        import mcs_amd
        p = mcs_amd.ExtractorParams(nfeatures=NFEAT, scale_factor=scale, nlevels=nlevels)
        self.ex = mcs_amd.Extractor(p, W, H, max_frames=F)
        self.torch, self.mcs, self.F, self.cap = torch, mcs_amd, F, self.ex.capacity
        self.s = torch.cuda.current_stream().cuda_stream
        self.keep = []

    def set_masks(self, masks):
        if masks is None:
            self.ex.set_masks_device(None, 0, self.s)
            return
        d = self.torch.from_numpy(np.ascontiguousarray(masks)).cuda()
        self.keep.append(d)
        self.ex.set_masks_device(d.data_ptr(), len(masks), self.s)

    def run(self, imgs, midx=None):
        t, F, cap = self.torch, len(imgs), self.cap
        d_img = t.from_numpy(np.ascontiguousarray(imgs)).cuda()
        d_midx = None if midx is None else t.from_numpy(midx).cuda()
        d_kps = t.full((F, cap * 7), -1, dtype=t.int32, device="cuda")
        d_cnt = t.full((F,), -1, dtype=t.int32, device="cuda")
        d_desc = t.zeros((F, cap, 32), dtype=t.uint8, device="cuda")
        self.ex.extract_batch_device(d_img.data_ptr(), F, None if midx is None else d_midx.data_ptr(),
                                     d_kps.data_ptr(), d_cnt.data_ptr(), d_desc.data_ptr(), self.s)
        t.cuda.synchronize()
        self.keep = self.keep[-4:] + [d_img]     # read_stage level 0 reads the input again
        cnt = d_cnt.cpu().numpy()
        kps = d_kps.cpu().numpy().view(self.mcs.KEYPOINT_DTYPE).reshape(F, cap)
        desc = d_desc.cpu().numpy()
        return [(kps[f, :cnt[f]].copy(), desc[f, :cnt[f]].copy()) for f in range(F)]


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for f, ((k, d), (ok, od)) in enumerate(zip(got, exp)):
        assert len(k) == len(ok), (what, f, len(k), len(ok))
        assert np.array_equal(k, ok), (what, f, "keypoints")
        assert np.array_equal(d, od), (what, f, "descriptors")


_REF = {}


def _ref(scale, nlevels):
    """Inputs and oracle outputs of one configuration, computed once and left unchanged."""
    key = (scale, nlevels)
    if key not in _REF:
        imgs, masks = _frames(40), _masks()
        exp = [ob.extract(imgs[f], masks[MIDX[f]], nfeatures=NFEAT, scale=scale, nlevels=nlevels)
               for f in range(5)]
        nomask = [ob.extract(imgs[f], None, nfeatures=NFEAT, scale=scale, nlevels=nlevels)
                  for f in range(5)]
        _REF[key] = (imgs, masks, exp, nomask)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", CONFIGS)
def test_masked_batch_bitexact_over_stale_workspace(gpu, scale, nlevels):
    """Noise, then all-255 frames, extracted without a mask fill every byte of the pyramid and
    blur workspaces; the masked batch after each must equal the oracle (a pixel outside the
    written units that reached an output would differ between the two)."""
    from mcs_amd import synth
    imgs, masks, exp, _ = _ref(scale, nlevels)
    assert min(len(k) for k, _ in exp) > 20 and sum(len(k) for k, _ in exp) > 500
    b = _Batch(scale, nlevels)
    noise = np.stack([synth.random_frame(W, H, 70 + k) for k in range(5)])
    runs = []
    for stale in (noise, np.full((5, H, W), 255, np.uint8)):
        b.set_masks(None)
        b.run(stale)
        b.set_masks(masks)
        runs.append(b.run(imgs, MIDX))
    _same(runs[0], exp, "after noise")
    _same(runs[1], exp, "after all-255")
    b.ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", CONFIGS)
def test_stages_where_the_mask_is_set(gpu, scale, nlevels):
    """With masks registered, stages 0 and 1 hold the pyramid and its blur wherever the level's
    mask is set; after the masks are dropped, everywhere again (same extractor)."""
    imgs, masks, exp, nomask = _ref(scale, nlevels)
    b = _Batch(scale, nlevels)
    b.set_masks(masks)
    _same(b.run(imgs, MIDX), exp, "masked")
    pyr = [ob.pyramid(imgs[f], nlevels, scale) for f in range(5)]
    for f in range(5):
        mk = ob.mask_pyramid(masks[MIDX[f]], nlevels, scale)
        for l in range(nlevels):
            on = mk[l] != 0
            assert np.array_equal(b.ex.read_stage(0, f, l)[on], pyr[f][l][on]), (f, l)
            assert np.array_equal(b.ex.read_stage(1, f, l)[on], ob.box_blur5(pyr[f][l])[on]), (f, l)
    b.set_masks(None)
    _same(b.run(imgs), nomask, "masks dropped")
    for f in range(5):
        for l in range(nlevels):
            assert np.array_equal(b.ex.read_stage(0, f, l), pyr[f][l]), (f, l)
            assert np.array_equal(b.ex.read_stage(1, f, l), ob.box_blur5(pyr[f][l])), (f, l)
    b.ex.close()


@pytest.mark.gpu
def test_empty_and_full_masks(gpu):
    """An all-zero mask gives no keypoints for its frames and leaves its neighbours in the batch
    alone; an all-255 mask gives what no mask gives."""
    scale, nlevels = CONFIGS[0]
    imgs, masks, exp, nomask = _ref(scale, nlevels)
    b = _Batch(scale, nlevels)
    b.set_masks(np.stack([masks[0], np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]))
    midx = np.array([0, 1, 2, 1, 0], np.int32)
    got = b.run(imgs, midx)
    assert len(got[1][0]) == 0 and len(got[3][0]) == 0
    _same([got[0], got[4]], [exp[0], exp[4]], "beside an empty mask")
    _same([got[2]], [nomask[2]], "all-255 mask")
    b.ex.close()
