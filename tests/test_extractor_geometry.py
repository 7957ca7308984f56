"""The extractor at other scale factors, level counts and frame shapes than the production
1.2 / 8 levels / 754x480: every path that those three inputs select in the host plan
(extractor_plan.cpp), in pyr_strips (extractor_kernels.hpp) and in the kernels, compared with
the CPU restatement (oracle/) stage by stage, bit-exact, with no tolerance anywhere.

What the cases reach (CASES below): the wide instantiation k_pyr_rows<true, 3> (scale > 1.5)
with a staged source row above 512 bytes, the last scale of the narrow instantiation, exact 2x
resizing (every alpha / beta 1024), ratios above 2 (source rows loaded and never used), 12
levels (kMaxLevels), one level (no resize), a single FAST cell, octree nIni 1 on portrait
levels and nIni 3..5 on wide ones; the second register pair of the per-segment row tables
(segments above 60 rows, batches of >= 256 frames only); and the plan's rejections.

CPU tests (not marked gpu): the preconditions on the oracle alone that keep the GPU
comparisons from being vacuous, and the bounds of what k_pyr_rows stages per work unit.  The
second drives the library's own build_plan and pyr_strips through tests/cpp/pyr_plan_dump.cpp.
common.hpp holds device helpers next to the host ones, so that program does not compile with
g++; it is compiled with hipcc for the host side only (no device code, no device needed).

Level sizes and the oracle's keypoints per level (fisheye image / random image) that the GPU
parity tests compared when they were written:
  two_strips 245x163 204x136 170x113: 121 100 83 / 119 101 83
  s150, s150up 489x301 326x201 217x134 145x89: 249 167 113 74 / 251 167 113 74
  s110_l12 733x491 666x446 606x406 551x369 501x335 455x305 414x277 376x252 342x229 311x208
      283x189 257x172: 202 182 167 152 137 124 115 103 93 85 78 72 /
      200 182 167 152 137 125 113 104 95 86 77 71
  s200 640x480 320x240 160x120: 516 259 131 / 514 259 130
  s220 537x363 244x165 111x75: 303 138 62 / 302 137 62
  panorama 900x300 750x250 625x208 521x174 434x145 362x121 301x100 251x84:
      219 182 151 127 107 87 74 61 / 219 183 151 127 106 88 73 60
  portrait 300x420 240x336 192x269 154x215: 171 137 109 88 / 169 136 109 88
  one_level 754x480: 1000 / 1001
  one_cell 74x74: 38 / 50
  two_tiny 89x107 74x89: 33 27 / 34 28
"""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_bind as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam-annotation_amd", "csrc")

F32 = np.float32
S150UP = np.nextafter(F32(1.5), F32(2))
S220 = F32(2.2)
S220UP = np.nextafter(F32(2.2), F32(3))

# id, W, H, scale (float32), nlevels, nfeatures
CASES = [
    ("two_strips", 245, 163, F32(1.2), 3, 300),   # smallest width with two column strips
    ("s150", 489, 301, F32(1.5), 4, 600),         # three strips, last scale of the narrow kernel
    ("s150up", 489, 301, S150UP, 4, 600),         # the same geometry through the wide kernel
    ("s110_l12", 733, 491, F32(1.1), 12, 1500),   # kMaxLevels
    ("s200", 640, 480, F32(2.0), 3, 900),         # exact 2x in both axes
    ("s220", 537, 363, S220, 3, 500),             # level 1: one 244-column strip, 537 staged bytes
    ("panorama", 900, 300, F32(1.2), 8, 1000),    # nIni 3, 4, 5
    ("portrait", 300, 420, F32(1.25), 4, 500),    # H > W, nIni 1
    ("one_level", 754, 480, F32(1.2), 1, 1000),   # no resize, the whole budget on level 0
    ("one_cell", 74, 74, F32(1.2), 1, 50),        # a single FAST cell
    ("two_tiny", 89, 107, F32(1.2), 2, 60),       # level 1 is 74x89
]
CASE = {c[0]: c for c in CASES}
IDS = [c[0] for c in CASES]
KINDS = ("fisheye", "random")
FAST_TH = 20

# the tall-segment batch (test_tall_segments_batch_256)
TALL = ("tall", 884, 596, F32(1.2), 2, 1500)
TALL_FRAMES = 256

# plan rejections: W, H, scale, nlevels, error code name, word the message must hold
REJECTS = [
    (754, 480, F32(1.0), 3, "MCS_ERR_ARG", "scale_factor"),
    (754, 480, F32(0.9), 3, "MCS_ERR_ARG", "scale_factor"),
    (754, 480, F32(1.2), 0, "MCS_ERR_ARG", "nlevels"),
    (754, 480, F32(1.2), 13, "MCS_ERR_ARG", "nlevels"),
    (754, 480, S220UP, 3, "MCS_ERR_UNSUPPORTED", "scale_factor"),
    (489, 301, F32(1.6), 4, "MCS_ERR_UNSUPPORTED", "FAST cell"),   # level 3 is 119x73: no cell row
    (300, 500, F32(1.3), 5, "MCS_ERR_UNSUPPORTED", "nIni"),        # nIni == 0 on level 4
]
ERR = {"MCS_ERR_ARG": -1, "MCS_ERR_UNSUPPORTED": -4}


def _images(case, kind):
    from mcs_amd import synth
    _, W, H = case[:3]
    if kind == "fisheye":
        return synth.fisheye_frame(W, H, seed=W + H)
    return synth.random_frame(W, H, seed=1), None


_REF = {}


def _oracle(cid, kind):
    """Everything the oracle says about one case and image, computed once and left unchanged."""
    key = (cid, kind)
    if key not in _REF:
        case = CASE[cid]
        _, W, H, scale, nl, nf = case
        s = float(scale)
        img, mask = _images(case, kind)
        sizes = ob.level_sizes(W, H, nl, s)
        nfl = ob.features_per_level(nf, nl, s)
        pyr = ob.pyramid(img, nl, s)
        mk = ob.mask_pyramid(mask, nl, s) if mask is not None else [None] * nl
        cand = [ob.level_candidates(pyr[l], mk[l], FAST_TH) for l in range(nl)]
        sel = [cand[l][ob.octree(cand[l], pyr[l].shape[1], pyr[l].shape[0], int(nfl[l]))]
               for l in range(nl)]
        kps, desc = ob.extract(img, mask, nfeatures=nf, scale=s, nlevels=nl, fast_th=FAST_TH)
        _REF[key] = dict(img=img, mask=mask, sizes=sizes, nfl=nfl, pyr=pyr,
                         blur=[ob.box_blur5(p) for p in pyr], cand=cand, sel=sel, kps=kps, desc=desc)
    return _REF[key]


# ---------------------------------------------------------------------------
# 1. preconditions on the oracle alone (CPU)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_case_preconditions(built, cid):
    _, W, H, scale, nl, nf = CASE[cid]
    sizes = ob.level_sizes(W, H, nl, float(scale))
    nfl = ob.features_per_level(nf, nl, float(scale))
    assert tuple(sizes[0]) == (W, H)
    for l, (w, h) in enumerate(sizes):
        assert w >= 74 and h >= 74, (cid, l, w, h)
        # round(): half to even, like cvRound
        assert round((int(w) - 44) / (int(h) - 44)) >= 1, (cid, l, w, h)
    assert (nfl <= 1021).all() and (nfl >= 1).all() and nfl.sum() == nf, (cid, nfl)
    for kind in KINDS:
        o = _oracle(cid, kind)
        per_level = np.bincount(o["kps"]["octave"], minlength=nl)
        assert (per_level >= 1).all(), (cid, kind, per_level)
        assert per_level.sum() == len(o["kps"])
        assert np.array_equal(per_level, [len(s) for s in o["sel"]]), (cid, kind)


def test_case_geometry_reached(built):
    """The geometry each case is in the table for, from the oracle's level sizes."""
    def nini(cid):
        _, W, H, s, nl, _ = CASE[cid]
        return [round((int(w) - 44) / (int(h) - 44)) for w, h in ob.level_sizes(W, H, nl, float(s))]
    assert set(nini("panorama")) == {3, 4, 5}
    assert set(nini("portrait")) == {1}
    _, W, H, s, nl, _ = CASE["portrait"]
    assert all(h > w for w, h in ob.level_sizes(W, H, nl, float(s)))
    assert ob.level_sizes(640, 480, 3, 2.0).tolist() == [[640, 480], [320, 240], [160, 120]]
    assert ob.level_sizes(537, 363, 3, float(S220))[1].tolist() == [244, 165]
    assert ob.level_sizes(89, 107, 2, float(F32(1.2)))[1].tolist() == [74, 89]
    assert ob.level_sizes(884, 596, 2, float(F32(1.2)))[1].tolist() == [737, 497]
    assert float(S150UP) > 1.5 and float(F32(1.5)) == 1.5
    assert float(S220) > 2.2   # the documented maximum as a float lies above the double 2.2


def test_s150_and_s150up_same_geometry(built):
    a, b = CASE["s150"], CASE["s150up"]
    assert a[3] != b[3]
    assert np.array_equal(ob.level_sizes(a[1], a[2], a[4], float(a[3])),
                          ob.level_sizes(b[1], b[2], b[4], float(b[3])))
    assert np.array_equal(ob.features_per_level(a[5], a[4], float(a[3])),
                          ob.features_per_level(b[5], b[4], float(b[3])))


# ---------------------------------------------------------------------------
# 2. what k_pyr_rows stages, from the library's own build_plan + pyr_strips (CPU)
# ---------------------------------------------------------------------------
SWEEP_SCALES = [F32(1.1), F32(1.2), F32(1.5), S150UP, F32(1.6), F32(2.0), S220]
SWEEP_WIDTHS = range(100, 1401)


def _pyr_strips(dw, dh, F):
    """pyr_strips (extractor_kernels.hpp) restated -> (core, tiles_x, seg_rows, tiles_y)."""
    n = (dw + 243) // 244
    core = ((dw + n - 1) // n + 3) & ~3
    tiles_x = (dw + core - 1) // core
    F = max(F, 1)
    target = max(8192, 32 * F)
    per_seg = tiles_x * F
    segs = max(1, (target + per_seg - 1) // per_seg)
    rows = min(64, max(8, (dh + segs - 1) // segs))
    return core, tiles_x, rows, (dh + rows - 1) // rows


def _bits(scale):
    return int(np.array(scale, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """Compile tests/cpp/pyr_plan_dump.cpp (host side only) and run it once over every
    configuration of this module -> {(W, H, scale_bits, nlevels, nfeatures): record}."""
    exe = str(tmp_path_factory.mktemp("ppd") / "pyr_plan_dump")
    subprocess.check_call(["hipcc", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tests", "cpp", "pyr_plan_dump.cpp"),
                           os.path.join(CSRC, "extractor_plan.cpp"), "-o", exe])
    cfgs = [(c[1], c[2], _bits(c[3]), c[4], c[5]) for c in CASES + [TALL]]
    cfgs += [(W, H, _bits(s), nl, 500) for W, H, s, nl, _, _ in REJECTS]
    cfgs += [(W, min(W, 480), _bits(s), 2, 500) for s in SWEEP_SCALES for W in SWEEP_WIDTHS]
    text = "".join("%d %d %d %d %d\n" % c for c in cfgs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300,
                         check=True).stdout
    recs, cur = {}, None
    for ln in out.split("\n"):
        f = ln.split()
        if not f:
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "cfg":
            cur = dict(rc=v[5], lvl={}, seg={}, strips={})
            recs[tuple(v[:5])] = cur
        elif f[0] == "lvl":
            cur["lvl"][v[0]] = dict(zip(("w", "h", "nfeat", "nini", "sw", "sh", "amin",
                                         "amax", "bmin", "bmax", "ylo", "yhi"), v[1:]))
        elif f[0] == "seg":
            cur["seg"][(v[0], v[1])] = tuple(v[2:])
        else:
            cur["strips"].setdefault(v[0], []).append(tuple(v[1:]))
    assert len(recs) == len(set(cfgs))
    return recs


def _check_staging(key, rec):
    """The bounds of one accepted configuration; -> its largest staged row (bytes) per NDW."""
    scale = float(np.array(key[2], np.uint32).view(np.float32))
    worst = {1: 0, 2: 0, 3: 0}
    for l, L in rec["lvl"].items():
        ndw = 1 if l == 0 else (2 if scale <= 1.5 else 3)
        strips = rec["strips"][l]
        core, tiles_x = rec["seg"][(l, 1)][:2]
        assert core % 4 == 0 and 4 <= core <= 244 and tiles_x * core >= L["w"], (key, l)
        assert len(strips) == tiles_x and [s[0] for s in strips] == [i * core for i in range(tiles_x)]
        for xs, c_lo, c_hi in strips:
            assert 0 <= c_lo <= c_hi <= L["sw"] - 1, (key, l, xs, c_lo, c_hi)
            nbytes = c_hi - c_lo + 1
            assert 3 + nbytes <= 256 * ndw, (key, l, xs, nbytes)
            # the row starts at byte 0..3 of its first dword, and the resize reads one byte past
            # a pixel's source column: the last staged byte read, inside the NDW dwords per lane
            assert 3 + nbytes - 1 + (1 if l else 0) <= 256 * ndw - 1, (key, l, xs, nbytes)
            worst[ndw] = max(worst[ndw], nbytes)
        for (ll, F), (c, tx, seg_rows, tiles_y) in rec["seg"].items():
            if ll != l:
                continue
            assert (c, tx, seg_rows, tiles_y) == _pyr_strips(L["w"], L["h"], F), (key, l, F)
            assert seg_rows + 4 <= 128 and seg_rows * tiles_y >= L["h"] and seg_rows >= 1, (key, l, F)
        if l > 0:
            # pack_rows: two source rows in 16 + 16 bits; pack_beta and alpha << 4: u16
            assert 0 <= L["ylo"] <= L["yhi"] <= L["sh"] - 1 <= 0xFFFF, (key, l)
            assert 0 <= L["amin"] and L["amax"] <= 2048 and 0 <= L["bmin"] and L["bmax"] <= 2048, (key, l)
    return worst


def test_staged_row_bound_cases(plan_dump):
    for c in CASES + [TALL]:
        key = (c[1], c[2], _bits(c[3]), c[4], c[5])
        rec = plan_dump[key]
        assert rec["rc"] == 0, c[0]
        s = float(c[3])
        assert [[L["w"], L["h"]] for _, L in sorted(rec["lvl"].items())] == \
            ob.level_sizes(c[1], c[2], c[4], s).tolist(), c[0]
        assert [L["nfeat"] for _, L in sorted(rec["lvl"].items())] == \
            ob.features_per_level(c[5], c[4], s).tolist(), c[0]
        _check_staging(key, rec)
    # what single cases are in the table for, as the plan sees it
    rec = plan_dump[(537, 363, _bits(S220), 3, 500)]
    assert rec["strips"][1] == [(0, 0, 536)]                       # 537 bytes > 512: third dword
    assert rec["seg"][(1, 1)][:2] == (244, 1)
    assert len(plan_dump[(245, 163, _bits(F32(1.2)), 3, 300)]["strips"][0]) == 2
    assert len(plan_dump[(489, 301, _bits(F32(1.5)), 4, 600)]["strips"][0]) == 3
    r2 = plan_dump[(640, 480, _bits(F32(2.0)), 3, 900)]
    assert all((L["amin"], L["amax"], L["bmin"], L["bmax"]) == (1024,) * 4
               for l, L in r2["lvl"].items() if l > 0)
    rp = plan_dump[(300, 420, _bits(F32(1.25)), 4, 500)]
    assert all(L["nini"] == 1 and L["h"] > L["w"] for L in rp["lvl"].values())
    assert sorted(set(L["nini"] for L in plan_dump[(900, 300, _bits(F32(1.2)), 8, 1000)]["lvl"].values())) == [3, 4, 5]
    # the tall-segment batch: 8 segments of 63 rows on level 1 at 256 frames, 38 or fewer below
    rt = plan_dump[(TALL[1], TALL[2], _bits(TALL[3]), TALL[4], TALL[5])]
    assert rt["seg"][(1, TALL_FRAMES)] == (188, 4, 63, 8)
    assert rt["seg"][(1, 64)][2] <= 60


def test_staged_row_bound_sweep(plan_dump):
    worst = {1: 0, 2: 0, 3: 0}
    accepted = 0
    for s in SWEEP_SCALES:
        for W in SWEEP_WIDTHS:
            H = min(W, 480)
            key = (W, H, _bits(s), 2, 500)
            rec = plan_dump[key]
            w1, h1 = ob.level_sizes(W, H, 2, float(s))[1]
            # the plan rejects exactly the geometries with a level under one FAST cell
            assert (rec["rc"] == 0) == (w1 >= 74 and h1 >= 74), (key, rec["rc"], w1, h1)
            if rec["rc"] != 0:
                assert rec["rc"] == ERR["MCS_ERR_UNSUPPORTED"]
                continue
            accepted += 1
            for ndw, v in _check_staging(key, rec).items():
                worst[ndw] = max(worst[ndw], v)
    assert accepted > 0.95 * len(SWEEP_SCALES) * len(SWEEP_WIDTHS)
    # the sweep reaches rows that need the last dword of each instantiation
    assert worst[1] > 192 and worst[2] > 256 and worst[3] > 512, worst
    print("largest staged source row (bytes): level 0 %d of 256, narrow %d of 512, wide %d of 768"
          % (worst[1], worst[2], worst[3]))


def test_plan_rejections_host(plan_dump):
    """The rejections of section 5 as build_plan returns them (the GPU test repeats them
    through mcs_extractor_create); 2.2f itself is accepted."""
    for W, H, s, nl, code, _ in REJECTS:
        assert plan_dump[(W, H, _bits(s), nl, 500)]["rc"] == ERR[code], (W, H, float(s), nl)
    assert plan_dump[(537, 363, _bits(S220), 3, 500)]["rc"] == 0


# ---------------------------------------------------------------------------
# 3. GPU parity, stage by stage
# ---------------------------------------------------------------------------
def _params(case):
    import mcs_amd
    return mcs_amd.ExtractorParams(nfeatures=case[5], scale_factor=float(case[3]), nlevels=case[4],
                                   fast_threshold=FAST_TH)


_GPU = {}


def _gpu_run(cid, kind):
    """One extraction of a case on the device -> its levels, the four stages of every level and
    the final keypoints and descriptors (run once per case and image)."""
    key = (cid, kind)
    if key not in _GPU:
        import mcs_amd
        case = CASE[cid]
        img, mask = _images(case, kind)
        ex = mcs_amd.Extractor(_params(case), case[1], case[2], max_frames=1)
        try:
            wh, nfl = ex.levels()
            kps, desc = ex.extract(img, mask)
            stages = [[ex.read_stage(s, 0, l).copy() for s in range(4)] for l in range(case[4])]
        finally:
            ex.close()
        _GPU[key] = dict(wh=wh.copy(), nfl=nfl.copy(), kps=kps, desc=desc, stages=stages)
    return _GPU[key]


def _rows_differ(a, b):
    if a.shape != b.shape:
        return "%d rows vs %d" % (len(a), len(b))
    return "%d of %d rows differ" % (int((a != b).any(axis=1).sum()), len(a))


def _compare_frame(tag, kps, desc, okps, odesc):
    assert len(kps) == len(okps), "%s: %d keypoints, oracle %d" % (tag, len(kps), len(okps))
    for name in okps.dtype.names:
        assert np.array_equal(kps[name], okps[name]), "%s: keypoint field %s differs in %d rows" % (
            tag, name, int((kps[name] != okps[name]).sum()))
    assert np.array_equal(desc, odesc), "%s: descriptors, %s" % (tag, _rows_differ(desc, odesc))


def _check_case(cid, kind):
    o = _oracle(cid, kind)
    g = _gpu_run(cid, kind)
    tag = "%s/%s" % (cid, kind)
    assert np.array_equal(g["wh"], o["sizes"]), "%s: level sizes %s vs oracle %s" % (
        tag, g["wh"].tolist(), o["sizes"].tolist())
    assert np.array_equal(g["nfl"], o["nfl"]), "%s: level budgets %s vs oracle %s" % (
        tag, g["nfl"].tolist(), o["nfl"].tolist())
    for l in range(CASE[cid][4]):
        raw, blur, cand, sel = g["stages"][l]
        assert np.array_equal(raw, o["pyr"][l]), "%s level %d: pyramid differs in %d px" % (
            tag, l, int((raw != o["pyr"][l]).sum()))
        assert np.array_equal(blur, o["blur"][l]), "%s level %d: blur differs in %d px" % (
            tag, l, int((blur != o["blur"][l]).sum()))
        assert np.array_equal(cand, o["cand"][l]), "%s level %d: FAST candidates, %s" % (
            tag, l, _rows_differ(cand, o["cand"][l]))
        assert np.array_equal(sel, o["sel"][l]), "%s level %d: octree selection, %s" % (
            tag, l, _rows_differ(sel, o["sel"][l]))
    _compare_frame(tag, g["kps"], g["desc"], o["kps"], o["desc"])
    print("%s: levels %s keypoints per level %s" % (
        tag, " ".join("%dx%d" % tuple(s) for s in o["sizes"]),
        np.bincount(o["kps"]["octave"], minlength=CASE[cid][4]).tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", IDS)
def test_geometry_parity(gpu, cid, kind):
    _check_case(cid, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_s150_narrow_equals_wide(gpu, kind):
    """Scale 1.5 (k_pyr_rows<true, 2>) and the next float above it (k_pyr_rows<true, 3>) have
    the same level sizes and budgets; the device outputs are then equal byte for byte."""
    a, b = _gpu_run("s150", kind), _gpu_run("s150up", kind)
    for l in range(CASE["s150"][4]):
        for s, name in enumerate(("pyramid", "blur", "FAST candidates", "octree selection")):
            assert np.array_equal(a["stages"][l][s], b["stages"][l][s]), "%s level %d: %s differs" % (
                kind, l, name)
    # size and the octave's scale come from scale_factor itself; everything else is equal
    for name in ("x", "y", "angle", "response", "octave", "class_id"):
        eq = a["kps"][name] == b["kps"][name]
        if name in ("x", "y"):
            eq = eq | (a["kps"]["octave"] > 0)
        assert eq.all(), "%s: keypoint field %s differs" % (kind, name)
    assert np.array_equal(a["desc"], b["desc"]), "%s: descriptors differ" % kind


@pytest.mark.gpu
def test_batch_wide_kernel_with_masks(gpu):
    """s150up as a batch of 5 frames with 2 registered device masks indexed [0, 1, 0, 1, 0]."""
    import torch
    import mcs_amd
    from mcs_amd import synth
    case = CASE["s150up"]
    _, W, H, scale, nl, nf = case
    frames, masks = [], []
    for i in range(5):
        img, mask = synth.fisheye_frame(W, H, seed=100 + i, cam_index=i % 2)
        frames.append(img)
        masks.append(mask)
    midx = [0, 1, 0, 1, 0]
    ex = mcs_amd.Extractor(_params(case), W, H, max_frames=5)
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(np.stack(frames)).to(dev)
    d_mask = torch.from_numpy(np.stack(masks[:2])).to(dev)
    d_midx = torch.tensor(midx, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ex.set_masks_device(d_mask.data_ptr(), 2, s)
    cap = ex.capacity
    d_kps = torch.full((5, cap * 7), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.full((5,), -1, dtype=torch.int32, device=dev)
    d_desc = torch.zeros((5, cap, 32), dtype=torch.uint8, device=dev)
    ex.extract_batch_device(d_img.data_ptr(), 5, d_midx.data_ptr(), d_kps.data_ptr(),
                            d_cnt.data_ptr(), d_desc.data_ptr(), s)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    kp_all = d_kps.cpu().numpy().view(mcs_amd.KEYPOINT_DTYPE).reshape(5, cap)
    de_all = d_desc.cpu().numpy()
    ex.close()
    for f in range(5):
        okps, odesc = ob.extract(frames[f], masks[midx[f]], nfeatures=nf, scale=float(scale),
                                 nlevels=nl, fast_th=FAST_TH)
        assert len(okps) > 0
        assert 0 <= cnt[f] <= cap, (f, cnt[f])
        _compare_frame("s150up batch frame %d" % f, kp_all[f, :cnt[f]], de_all[f, :cnt[f]], okps, odesc)


# ---------------------------------------------------------------------------
# 4. the tall-segment batch: row tables above 64 entries
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_tall_segments_batch_256(gpu):
    """884x596, scale 1.2, 2 levels, 256 frames in one call: pyr_strips cuts level 1 (737x497,
    four strips) into 8 segments of 63 rows, so a wave's row tables hold 67 entries and
    row_tab / row_beta of k_pyr_rows read their second register pair (index >= 64).  Below 256
    frames the segments stay at or under 60 rows and that path is not reached."""
    import time
    import torch
    import mcs_amd
    from mcs_amd import synth
    _, W, H, scale, nl, nf = TALL
    F = TALL_FRAMES
    w1, h1 = ob.level_sizes(W, H, nl, float(scale))[1]
    core, tiles_x, seg_rows, tiles_y = _pyr_strips(int(w1), int(h1), F)
    assert (w1, h1, tiles_x) == (737, 497, 4)
    assert seg_rows > 60, "segments of %d rows: the second register pair is not reached" % seg_rows
    assert min(h1, seg_rows + 2) + 2 > 64   # rows r_begin..r_end of an inner segment

    uniq = [synth.fisheye_frame(W, H, seed=5)[0], synth.random_frame(W, H, seed=2),
            synth.fisheye_frame(W, H, seed=9)[0], synth.random_frame(W, H, seed=3)]
    dev = torch.device("cuda:0")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ex = mcs_amd.Extractor(_params(TALL), W, H, max_frames=F)
    free1 = torch.cuda.mem_get_info()[0]
    print("extractor workspace for %d frames of %dx%d: %.2f GB" % (F, W, H, (free0 - free1) / 1e9))
    cap = ex.capacity
    d_img = torch.from_numpy(np.stack(uniq)).to(dev).repeat(F // 4, 1, 1).contiguous()
    assert d_img.shape == (F, H, W)
    d_kps = torch.full((F, cap * 7), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.full((F,), -1, dtype=torch.int32, device=dev)
    d_desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ex.extract_batch_device(d_img.data_ptr(), F, None, d_kps.data_ptr(), d_cnt.data_ptr(),
                            d_desc.data_ptr(), s)
    torch.cuda.synchronize()
    print("extract_batch_device of %d frames: %.1f ms" % (F, 1e3 * (time.perf_counter() - t0)))
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(mcs_amd.KEYPOINT_DTYPE).reshape(F, cap)
    desc = d_desc.cpu().numpy()
    stage = {f: (ex.read_stage(0, f, 1).copy(), ex.read_stage(1, f, 1).copy())
             for f in (0, 1, 2, 3, F - 4, F - 3, F - 2, F - 1)}
    ex.close()

    for u in range(4):
        ref = ob.pyramid(uniq[u], nl, float(scale))[1]
        rblur = ob.box_blur5(ref)
        for f in (u, F - 4 + u):
            raw, blur = stage[f]
            bad = raw != ref
            assert not bad.any(), "tall frame %d level 1: pyramid differs in %d px (rows %s)" % (
                f, int(bad.sum()), np.flatnonzero(bad.any(axis=1))[:8].tolist())
            assert np.array_equal(blur, rblur), "tall frame %d level 1: blur differs in %d px" % (
                f, int((blur != rblur).sum()))
        okps, odesc = ob.extract(uniq[u], None, nfeatures=nf, scale=float(scale), nlevels=nl,
                                 fast_th=FAST_TH)
        assert len(okps) > 0 and (okps["octave"] == 1).any()
        n = int(cnt[u])
        assert 0 <= n <= cap
        _compare_frame("tall frame %d" % u, kps[u, :n], desc[u, :n], okps, odesc)
        for f in range(u + 4, F, 4):
            assert cnt[f] == n, "tall frame %d: %d keypoints, its first copy %d" % (f, cnt[f], n)
            assert np.array_equal(kps[f, :n], kps[u, :n]), "tall frame %d: keypoints differ from frame %d" % (f, u)
            assert np.array_equal(desc[f, :n], desc[u, :n]), "tall frame %d: descriptors differ from frame %d" % (f, u)


# ---------------------------------------------------------------------------
# 5. rejections (create opens the device first); the oracle is never called on these
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H,scale,nl,code,word", REJECTS,
                         ids=["scale1.0", "scale0.9", "nlevels0", "nlevels13", "scale2.2up",
                              "no_cell_row", "nini0"])
def test_create_rejects(gpu, W, H, scale, nl, code, word):
    import mcs_amd
    p = mcs_amd.ExtractorParams(nfeatures=500, scale_factor=float(scale), nlevels=nl,
                                fast_threshold=FAST_TH)
    with pytest.raises(mcs_amd.McsError) as e:
        mcs_amd.Extractor(p, W, H, max_frames=1)
    assert e.value.code == getattr(mcs_amd, code), str(e.value)
    assert word in str(e.value), str(e.value)
    # the library is still usable: a valid create and an extraction on the same process
    case = CASE["one_cell"]
    ex = mcs_amd.Extractor(_params(case), case[1], case[2], max_frames=1)
    img, _ = _images(case, "random")
    kps, _ = ex.extract(img, None)
    ex.close()
    assert len(kps) == len(_oracle("one_cell", "random")["kps"])


@pytest.mark.gpu
def test_create_accepts_scale_2_2f(gpu):
    """The documented maximum, passed as the float it is ((double)2.2f = 2.2000000477)."""
    import mcs_amd
    case = CASE["s220"]
    ex = mcs_amd.Extractor(_params(case), case[1], case[2], max_frames=1)
    wh, _ = ex.levels()
    ex.close()
    assert wh.tolist() == [[537, 363], [244, 165], [111, 75]]
