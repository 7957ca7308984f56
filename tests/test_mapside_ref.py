"""The map-point refresh and isInFrustum against the reference's OWN text.

tests/golden/mapside_ref.npz holds, evaluated from the reference text by
tests/golden/gen_mapside_ref.py on a scripted map (40 keyframes of the 3-camera Lafida rig,
300 map points) and on 600 points x 3 cameras of one rig pose:
  cMapPoint::ComputeDistinctiveDescriptors  src/cMapPoint.cpp:297-390 (16 / 32 / 64 bytes,
                                            havingMasks false and true)
  cMapPoint::UpdateNormalAndDepth           :453-496, Get{Min,Max}DistanceInvariance :498-508
  cMultiFrame::isInFrustum                  src/cMultiFrame.cpp:218-270 with WorldToCamHom_fast,
                                            invMat, WorldToImg and isPointInMirrorMask
The product takes flat CSR lists (include/mcs_mappoint.h); `flatten` below builds them from the
scripted observation maps by the rule that header words, and the oracle restatements
(oracle/mappoint_oracle.cpp, oracle_is_in_frustum) and the three device entry points are held
to the fixture: chosen descriptor / mask exact, normal and mfMin/MaxDistance bitwise, frustum
flags and levels equal on every (point, camera), projections abs 1e-9 px, viewCos abs 1e-12.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_bind as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mapside_ref.npz")
CONFIGS = [(16, False), (32, False), (64, False), (16, True), (32, True), (64, True)]
DESC_COUNTS = (0, 1, 2, 3, 4, 64, 65, 66, 129, 193)
_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(FIX, allow_pickle=False)
        _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def flatten(z):
    """The scripted map as the CSR arguments of include/mcs_mappoint.h.  Per point, in the order
    of its std::map (keyframe allocation order = the fixture's entry order):
      * a bad point has no entry in either list (both methods return before reading anything);
      * UpdateNormalAndDepth's list holds every keyframe of the map ONCE -- bad or not, however
        many keypoints (cameras) of it see the point, even none;
      * the descriptor list holds, for the keyframes that are not bad, one row per entry of the
        keyframe's index vector, in vector order: (keypoint_to_cam, cont_idx_to_local_cam_idx)
        of the continuous index select the camera's descriptor row;
      * ref_level = octave of the FIRST index the reference keyframe holds, -1 when it is not
        in the map or its index vector is empty."""
    if "flat" in _cache:
        return _cache["flat"]
    P = len(z["map_pt_bad"])
    kp_off, ent_off, idx_off = z["map_kp_off"], z["map_ent_off"], z["map_idx_off"]
    nd_ptr, nd_kf, d_ptr, d_row, ref_level = [0], [], [0], [], []
    for p in range(P):
        lvl = -1
        if not z["map_pt_bad"][p]:
            for e in range(ent_off[p], ent_off[p + 1]):
                k = int(z["map_ent_kf"][e])
                idx = z["map_idx"][idx_off[e]:idx_off[e + 1]]
                nd_kf.append(k)
                if k == z["map_pt_ref"][p] and len(idx):
                    lvl = int(z["map_kp_oct"][kp_off[k] + idx[0]])
                if z["map_kf_bad"][k]:
                    continue
                for l in idx:
                    cam, loc = z["map_kp_cam"][kp_off[k] + l], z["map_kp_local"][kp_off[k] + l]
                    d_row.append(int(z["map_cam_off"][k, cam]) + int(loc))
        nd_ptr.append(len(nd_kf))
        d_ptr.append(len(d_row))
        ref_level.append(lvl)
    i32 = lambda a: np.asarray(a, np.int32)  # noqa: E731
    _cache["flat"] = dict(nd_ptr=i32(nd_ptr), nd_kf=i32(nd_kf), d_ptr=i32(d_ptr), d_row=i32(d_row),
                          ref_level=i32(ref_level), ref_kf=i32(z["map_pt_ref"]))
    return _cache["flat"]


def tagged(z, name):
    return np.nonzero(z["map_pt_tag"] == list(z["map_tag_names"]).index(name))[0]


def _prefix(name, nbytes, masked):
    return "d%d%s_%s" % (nbytes, "m" if masked else "", name)


def frustum_masks(z):
    from mcs_amd import synth
    if "masks" not in _cache:
        _cache["masks"] = np.stack([synth.mirror_mask(c) for c in synth.LAFIDA_CAMS]).astype(np.uint8)
    return _cache["masks"]


# ------------------------------------------------------------------ fixture shape
def test_fixture_shape_map():
    z = fixture()
    f = flatten(z)
    assert int(z["n_statements"]) == 142 and int(z["n_statements_refmath"]) == 80
    assert str(z["tie_convention"]).startswith("pointer order")
    K, P = len(z["map_kf_bad"]), len(z["map_pt_bad"])
    assert (K, P) == (40, 300) and int(z["map_kf_bad"].sum()) == 6
    bad_pt = z["map_pt_bad"] == 1
    assert int(bad_pt.sum()) == 10
    ent_off, idx_off, kp_off = z["map_ent_off"], z["map_idx_off"], z["map_kp_off"]
    ncam = {2: 0, 3: 0}
    dup_idx = empty_entries = bad_observers = all_bad = ref_absent = ref_bad = 0
    for p in range(P):
        kfs = z["map_ent_kf"][ent_off[p]:ent_off[p + 1]]
        assert len(kfs) > 0 and (np.diff(kfs) > 0).all()           # map order, one entry per keyframe
        seen = {2: False, 3: False}
        for e in range(ent_off[p], ent_off[p + 1]):
            idx = z["map_idx"][idx_off[e]:idx_off[e + 1]]
            k = z["map_ent_kf"][e]
            cams = set(z["map_kp_cam"][kp_off[k] + idx].tolist())
            if len(cams) in seen:
                seen[len(cams)] = True
            dup_idx += len(set(idx.tolist())) < len(idx)
            empty_entries += len(idx) == 0
        for n in (2, 3):
            ncam[n] += seen[n]
        if bad_pt[p]:
            continue
        bad_observers += bool(z["map_kf_bad"][kfs].any())
        all_bad += bool(z["map_kf_bad"][kfs].all())
        ref_absent += z["map_pt_ref"][p] not in kfs
        ref_bad += bool(z["map_kf_bad"][z["map_pt_ref"][p]])
    assert ncam[2] >= 20 and ncam[3] >= 10
    assert bad_observers >= 50 and all_bad == 3
    assert ref_bad >= 7 and ref_absent >= 10
    assert dup_idx == 1 and empty_entries == 8
    counts = np.diff(f["d_ptr"])
    assert set(DESC_COUNTS) <= set(counts.tolist())
    assert {-1, 0, 1, 7} <= set(f["ref_level"][~bad_pt].tolist())
    # a keyframe that sees a point in several cameras is one entry of the normal's list
    assert int(np.diff(f["nd_ptr"]).sum()) == int((~bad_pt[np.repeat(np.arange(P), np.diff(ent_off))]).sum())
    assert int(np.diff(f["nd_ptr"]).sum()) < int(counts.sum())
    sn, sd = z["sentinel_normal"], z["sentinel_dist"]
    for p in np.nonzero(bad_pt)[0]:                                 # bad points: untouched by both
        assert np.array_equal(z["nd_normal"][p], sn) and z["nd_min"][p] == sd[0] and z["nd_max"][p] == sd[1]
    upd = ~bad_pt
    assert not (z["nd_normal"][upd] == sn).all(1).any() and (z["nd_min"][upd] > 0).all()
    assert np.array_equal(z["nd_min_inv"][upd], 0.8 * z["nd_min"][upd])
    assert np.array_equal(z["nd_max_inv"][upd], 1.2 * z["nd_max"][upd])
    for nbytes, masked in CONFIGS:
        br = z[_prefix("best_row", nbytes, masked)]
        assert np.array_equal(br >= 0, counts > 0)                  # refreshed iff a descriptor exists
        assert (br[bad_pt] == -1).all() and (br[tagged(z, "all_bad_observers")] == -1).all()
        assert (br[tagged(z, "only_empty_entries")] == -1).all()
        if masked:
            assert np.array_equal(z[_prefix("mask_row", nbytes, masked)], br)
        best = [f["d_row"][f["d_ptr"][p]:f["d_ptr"][p + 1]].tolist().index(br[p]) if br[p] >= 0 else -1
                for p in range(P)]
        # all-equal descriptors: every median 0 -> index 0; complementary (A, ~A, ~A): row 0's
        # median is 8 * bytes, row 1's is 0; the tie (medians 24, 8, 8): the first 8 wins
        for name, want in (("all_equal", 0), ("complementary", 1), ("tie", 1)):
            p = tagged(z, name)
            assert len(p) == 1 and best[p[0]] == want, (name, nbytes, masked)
        p = tagged(z, "complementary")[0]
        rows = f["d_row"][f["d_ptr"][p]:f["d_ptr"][p + 1]]
        d = z["map_desc"][rows][:, :nbytes]
        assert np.unpackbits(d[0] ^ d[1]).sum() == 8 * nbytes and (z["map_dmask"][rows] == 255).all()
    # the same keypoint twice in one index vector; two keypoints with one descriptor
    lists = [f["d_row"][f["d_ptr"][p]:f["d_ptr"][p + 1]].tolist() for p in tagged(z, "twice")]
    assert sorted((len(r), len(set(r))) for r in lists) == [(4, 4), (5, 4)]
    rows = [r for r in lists if len(r) == 4][0]
    same = [(i, j) for i in range(4) for j in range(i + 1, 4)
            if np.array_equal(z["map_desc"][rows[i]], z["map_desc"][rows[j]])]
    assert len(same) == 1


def test_fixture_shape_frustum():
    z = fixture()
    from mcs_amd import synth
    masks = frustum_masks(z)
    assert hashlib.sha256(masks.tobytes()).hexdigest() == str(z["fr_mask_sha"])
    n, C = z["fr_in_view"].shape
    assert (n, C) == (600, 3)
    names = list(z["fr_kind_names"])
    kind, tc, iv, uv = z["fr_kind"], z["fr_target_cam"], z["fr_in_view"], z["fr_uv_all"]
    at = lambda a, s: a[s, tc[s]]  # noqa: E731
    sel = lambda name: np.nonzero(kind == names.index(name))[0]  # noqa: E731
    # no projection near a half pixel: every rounded pixel, and so every flag, is last-ulp proof
    assert (np.abs(np.abs(uv - np.floor(uv)) - 0.5) >= 1e-6).all() and int(z["fr_redrawn"]) >= 0
    for c in range(C):
        r = sel("random")
        assert iv[r, c].sum() >= 50 and (iv[r, c] == 0).sum() >= 50        # inside and outside
    H, W = masks.shape[1:]
    rnd = np.rint(uv).astype(int)
    for name, axis, px, bound in (("row0", 1, 0, 1), ("row1", 1, 1, 0), ("row_last", 1, H - 1, 0),
                                  ("row_rows", 1, H, 1), ("col0", 0, 0, 1), ("col_cols", 0, W, 1)):
        s = sel(name)
        assert len(s) == 12 and (at(rnd[:, :, axis], s) == px).all(), name
        if bound:                                           # on the `<= 0` / `>=` bound: never in view
            assert (at(iv, s) == 0).all(), name
        else:                                               # the last pixel inside: the mask decides
            u, v = at(rnd[:, :, 0], s), at(rnd[:, :, 1], s)
            assert np.array_equal(at(iv, s) == 1, masks[tc[s], v, u] > 0) and at(iv, s).sum() >= 6, name
    for name, inside in (("mask_edge_in", 1), ("mask_edge_out", 0)):
        s = sel(name)
        u, v = at(rnd[:, :, 0], s), at(rnd[:, :, 1], s)
        assert len(s) == 12 and ((masks[tc[s], v, u] > 0) == bool(inside)).all() and (at(iv, s) == inside).all()
        assert ((masks[tc[s], v, u + (-1 if inside else 1)] > 0) != bool(inside)).all()
    s = sel("axis")                                         # norm == 0: the projection is (u0, v0)
    assert len(s) == 6 and (at(iv, s) == 1).all()
    for p in s:
        cam = synth.LAFIDA_CAMS[tc[p]]
        assert tuple(uv[p, tc[p]]) == (cam["u0"], cam["v0"])
    d, lo, hi = z["fr_dist_cam"], 0.8 * z["fr_dist"][:, 0], 1.2 * z["fr_dist"][:, 1]
    for name, ref, ulp, inside in (("dist_min_eq", lo, 0, 1), ("dist_min_out", lo, -1, 0),
                                   ("dist_max_eq", hi, 0, 1), ("dist_max_out", hi, 1, 0)):
        s = sel(name)
        want = ref[s] if ulp == 0 else np.nextafter(ref[s], ulp * np.inf)
        assert len(s) == 18 and np.array_equal(at(d, s), want) and (at(iv, s) == inside).all(), name
    scale = z["scale"]
    s = sel("ratio_eq")
    assert len(s) == int(z["fr_ratio_exact"]) >= 1
    ratio = at(d, s) / lo[s]
    lv = at(z["fr_level"], s)
    assert np.array_equal(ratio, scale[lv]) and set(lv.tolist()) == set(range(1, 8))
    # the nearest ratios on either side of a factor: just below s_k -> level k, just above -> k + 1
    for name, side in (("ratio_below", -1), ("ratio_above", 1)):
        s = sel(name)
        ratio, lv = at(d, s) / lo[s], at(z["fr_level"], s)
        k = lv if side < 0 else np.where(ratio > scale[-1], len(scale) - 1, lv - 1)   # capped above the last
        assert len(s) == 15 and (at(iv, s) == 1).all() and (k >= 1).all(), name
        assert ((ratio - scale[k]) * side > 0).all() and (np.abs(ratio / scale[k] - 1) < 1e-15).all(), name
    # every level in view is lower_bound's: s_(l-1) < ratio <= s_l, or the capped last level
    vis = iv == 1
    ratio, lv = (d / lo[:, None])[vis], z["fr_level"][vis]
    assert (ratio[lv > 0] > scale[lv[lv > 0] - 1]).all()
    assert ((ratio <= scale[lv]) | (lv == len(scale) - 1)).all()
    s = sel("ratio_capped")
    assert len(s) == 18 and (at(d, s) / lo[s] > scale[-1]).all() and (at(z["fr_level"], s) == 7).all()


# ------------------------------------------------------------------ oracle = fixture
def _oracle_distinctive(z, f, nbytes, masked):
    desc = np.ascontiguousarray(z["map_desc"][:, :nbytes])
    dmask = np.ascontiguousarray(z["map_dmask"][:, :nbytes]) if masked else None
    best = np.full(len(f["d_ptr"]) - 1, -7, np.int32)
    ob.lib().oracle_distinctive_descriptors(ob._p(desc), ob._p(dmask), nbytes, ob._p(f["d_ptr"]),
                                            ob._p(f["d_row"]), len(best), ob._p(best))
    return best


def _best_rows(f, best):
    q = np.minimum(f["d_ptr"][:-1] + np.maximum(best, 0), max(len(f["d_row"]) - 1, 0))
    return np.where(best >= 0, f["d_row"][q], -1).astype(np.int32)


@pytest.mark.parametrize("nbytes,masked", CONFIGS)
def test_oracle_distinctive_reproduces_reference_text(built, nbytes, masked):
    z = fixture()
    f = flatten(z)
    best = _oracle_distinctive(z, f, nbytes, masked)
    assert np.array_equal(_best_rows(f, best), z[_prefix("best_row", nbytes, masked)])


def _normal_depth_args(z, f):
    return (np.ascontiguousarray(z["map_pt_pos"]), f["nd_ptr"], f["nd_kf"],
            np.ascontiguousarray(z["map_kf_center"]), f["ref_kf"], f["ref_level"],
            np.ascontiguousarray(z["scale"]))


def _sentinel_outputs(z):
    P = len(z["map_pt_bad"])
    return (np.tile(z["sentinel_normal"], (P, 1)), np.full(P, z["sentinel_dist"][0]),
            np.full(P, z["sentinel_dist"][1]))


def test_oracle_normal_depth_reproduces_reference_text(built):
    z = fixture()
    f = flatten(z)
    pts, ptr, kf, kfc, ref, lvl, scale = _normal_depth_args(z, f)
    on, omin, omax = _sentinel_outputs(z)
    ob.lib().oracle_update_normal_depth(ob._p(pts), len(pts), ob._p(ptr), ob._p(kf), ob._p(kfc), ob._p(ref),
                                        ob._p(lvl), ob._p(scale), len(scale), ob._p(on), ob._p(omin), ob._p(omax))
    assert on.tobytes() == z["nd_normal"].tobytes()              # bitwise, untouched points included
    assert omin.tobytes() == z["nd_min"].tobytes()
    assert omax.tobytes() == z["nd_max"].tobytes()


def _frustum_args(z, cams=None, levels=None, points=None):
    """The fixture's isInFrustum inputs, optionally for a subset of the cameras, the first
    `levels` scale factors and the points [points[0], points[1])."""
    cams = list(range(z["fr_mc"].shape[0])) if cams is None else cams
    scale = z["scale"] if levels is None else z["scale"][:levels]
    pts = slice(None) if points is None else slice(*points)
    return (z["fr_pose"], z["fr_mc"][cams], z["fr_cam"][cams], frustum_masks(z)[cams], z["fr_pts"][pts],
            z["fr_nrm"][pts], z["fr_dist"][pts], scale)


def check_frustum(z, got, cams=None, levels=None, points=None):
    """Flags and levels equal on every (point, camera) -- nothing excluded; projections abs
    1e-9 px and viewCos abs 1e-12 where in view (tests/test_frame.py's tolerances)."""
    iv, pj, lv, vc = got
    cams = list(range(z["fr_in_view"].shape[1])) if cams is None else cams
    pts = slice(None) if points is None else slice(*points)
    e_iv = z["fr_in_view"][pts][:, cams]
    e_lv = z["fr_level"][pts][:, cams]
    if levels is not None:
        e_lv = np.minimum(e_lv, levels - 1)
    assert np.array_equal(iv, e_iv)
    assert np.array_equal(lv, e_lv)
    sel = e_iv == 1
    assert sel.any()
    assert np.abs(pj[sel] - z["fr_proj"][pts][:, cams][sel]).max() < 1e-9
    assert np.abs(vc[sel] - z["fr_view_cos"][pts][:, cams][sel]).max() < 1e-12
    assert not pj[~sel].any() and not vc[~sel].any()             # untouched where not in view


# (cameras, levels, points): all of it; one camera (C = 1); one level (L = 1: every level 0);
# n * C = 1, 255 and 257 (the last thread of a block, the first of the next)
FRUSTUM_SHAPES = [(None, None, None), ([0], None, None), ([1], None, None), ([2], None, None),
                  (None, 1, None), ([0], None, (1, 2)), (None, None, (0, 85)), ([2], None, (0, 257))]


@pytest.mark.parametrize("cams,levels,points", FRUSTUM_SHAPES)
def test_oracle_frustum_reproduces_reference_text(built, cams, levels, points):
    from tests.test_frame import _oracle_frustum
    z = fixture()
    check_frustum(z, _oracle_frustum(*_frustum_args(z, cams, levels, points)), cams, levels, points)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout")
def test_fixture_regenerates_from_reference_text(tmp_path):
    """In the build container the generator re-derives the fixture from the reference text,
    byte for byte."""
    out = tmp_path / "m.npz"
    gen = os.path.join(ROOT, "tests", "golden", "gen_mapside_ref.py")
    subprocess.check_call([sys.executable, gen, "--out", str(out)], timeout=900)
    assert open(out, "rb").read() == open(FIX, "rb").read()


# ------------------------------------------------------------------ device = fixture
def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes,masked", CONFIGS)
def test_gpu_distinctive_reproduces_reference_text(gpu, nbytes, masked):
    import torch
    import mcs_amd
    z = fixture()
    f = flatten(z)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    P = len(f["d_ptr"]) - 1
    d_desc = T(z["map_desc"][:, :nbytes])
    d_mask = T(z["map_dmask"][:, :nbytes]) if masked else None
    d_ptr, d_row = T(f["d_ptr"]), T(f["d_row"])
    d_best = torch.full((P,), -7, dtype=torch.int32, device=dev)
    d_od = torch.full((P, nbytes), 0xA5, dtype=torch.uint8, device=dev)
    d_om = torch.full((P, nbytes), 0xA5, dtype=torch.uint8, device=dev)
    assert mcs_amd.lib().mcs_distinctive_descriptors_device(_P(d_desc), _P(d_mask), nbytes, _P(d_ptr), _P(d_row),
                                                            P, _P(d_best), _P(d_od), _P(d_om), None) == 0
    torch.cuda.synchronize()
    rows = _best_rows(f, d_best.cpu().numpy())
    want = z[_prefix("best_row", nbytes, masked)]
    assert np.array_equal(rows, want)
    has = want >= 0
    od, om = d_od.cpu().numpy(), d_om.cpu().numpy()
    assert np.array_equal(od[has], z["map_desc"][want[has], :nbytes])
    assert (od[~has] == 0xA5).all()                              # mDescriptor left as it was
    if masked:
        assert np.array_equal(om[has], z["map_dmask"][want[has], :nbytes])
        assert (om[~has] == 0xA5).all()
    else:
        assert (om == 0xA5).all()


@pytest.mark.gpu
def test_gpu_normal_depth_reproduces_reference_text(gpu):
    import torch
    import mcs_amd
    z = fixture()
    f = flatten(z)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = [T(a) for a in _normal_depth_args(z, f)]
    out = [T(a) for a in _sentinel_outputs(z)]
    assert mcs_amd.lib().mcs_update_normal_depth_device(
        _P(d[0]), len(z["map_pt_pos"]), _P(d[1]), _P(d[2]), _P(d[3]), _P(d[4]), _P(d[5]), _P(d[6]),
        len(z["scale"]), _P(out[0]), _P(out[1]), _P(out[2]), None) == 0
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == z["nd_normal"].tobytes()
    assert out[1].cpu().numpy().tobytes() == z["nd_min"].tobytes()
    assert out[2].cpu().numpy().tobytes() == z["nd_max"].tobytes()


def gpu_frustum(pose, mc, cam, masks, pts, nrm, dist, scale):
    import torch
    from mcs_amd import lib
    dev = torch.device("cuda", 0)
    T = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)  # noqa: E731
    n, C = len(pts), len(mc)
    d = [T(x, np.float64) for x in (pose, mc, cam)] + [T(masks, np.uint8)] + \
        [T(x, np.float64) for x in (pts, nrm, dist, scale)]
    g_iv = torch.zeros((n, C), dtype=torch.uint8, device=dev)
    g_pj = torch.zeros((n, C, 2), dtype=torch.float64, device=dev)
    g_lv = torch.zeros((n, C), dtype=torch.int32, device=dev)
    g_vc = torch.zeros((n, C), dtype=torch.float64, device=dev)
    assert lib().mcs_is_in_frustum_device(_P(d[0]), _P(d[1]), _P(d[2]), C, _P(d[3]), masks.shape[2],
                                          masks.shape[1], _P(d[4]), _P(d[5]), _P(d[6]), n, _P(d[7]),
                                          len(scale), _P(g_iv), _P(g_pj), _P(g_lv), _P(g_vc), None) == 0
    torch.cuda.synchronize()
    return g_iv.cpu().numpy(), g_pj.cpu().numpy(), g_lv.cpu().numpy(), g_vc.cpu().numpy()


@pytest.mark.gpu
def test_gpu_frustum_reproduces_reference_text(gpu):
    """All 600 x 3; tests/test_frame.py re-runs the cases at C = 1, L = 1 and n * C off the block."""
    z = fixture()
    check_frustum(z, gpu_frustum(*_frustum_args(z)))
