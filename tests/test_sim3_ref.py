"""cORBmatcher::SearchBySim3 (reference src/cORBmatcher.cpp:1721-1988), the parts that need no GPU:

  np_sim3_active      vbAlreadyMatched1/2 (:1758-1774) and the activity flags of both loops
                      (:1784-1788, :1878-1882) from flat stand-ins of the map;
  np_search_by_sim3   a plain NumPy / Python restatement of the whole function for one candidate,
                      in the text's operation order: the Sim3 chain, the rig-frame depth test,
                      WorldToImg, the mirror mask, the distance window, the predicted level,
                      cMultiKeyFrame::GetFeaturesInArea, the best distance of both directions and
                      the agreement check;
  sim3_ref.npz        what the reference TEXT does on six scripted scenarios
                      (tests/golden/gen_sim3_ref.py): the restatement is pinned to it, and the
                      fixture regenerates bit for bit where the reference checkout is present;
  the C ABI           symbols, the struct mirror, MCS_ERR_ARG for every malformed call before any
                      device use, MCS_ERR_NO_DEVICE on a machine without a GPU.

Every floating-point decision of the scripted inputs that depends on atan keeps a margin of 1e-9
(pixels or cells) from its boundary: a projected pixel from a rounding half, a floor / ceil
argument of the cell range from an integer, |dx| - r and |dy| - r from zero.  The rig-z sign test,
the distance window and the level do not pass through atan and are exact without a margin.
"""
import math
import os

import numpy as np
import pytest

from tests.test_fuse_ref import (COLS, INT_MAX, MARGIN, ROWS, W, H, _flip, _int_margin, _inv_mat, _matmul_lr, make_rig,
                                 make_target, np_distance, np_grid)

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "sim3_ref.npz")
SCENARIOS = ["b32", "b16m", "b64", "s17", "s06", "edge"]
CRAFT = ("lower_exact", "lower_ulp_out", "upper_exact", "upper_ulp_out", "ratio_is_scale", "rig_behind_cam_in_mask",
         "rig_front_cam_outside", "levels_and_tie", "two_observations", "first_index_out_of_range")


def th_high(nbytes, masked):
    """TH_HIGH_ of the cORBmatcher ctor (src/cORBmatcher.cpp:46-65)."""
    return int(math.floor(1.5 * nbytes)) if masked else 3 * nbytes


# ----------------------------------------------------------------------------- the restatement
def np_sim3_active(has1, bad1, has2, bad2, matches12, first_idx):
    """:1758-1774 and the skip conditions of both loops.  has / bad: per keypoint slot whether a
    map point is there and whether it isBad(); matches12 [n1]: vpMatches12 as a KF2 keypoint index
    (-1 = NULL); first_idx [n1]: (int)GetIndexInKeyFrame(pKF2)[0] of vpMatches12[i] (-1 when the
    point does not observe KF2, src/cMapPoint.cpp:436-445).
    -> (active1 [n1], active2 [n2], vbAlreadyMatched1, vbAlreadyMatched2) uint8."""
    n1, n2 = len(has1), len(has2)
    am1, am2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    for i in range(n1):
        if matches12[i] >= 0:
            am1[i] = 1
            idx2 = int(first_idx[i])
            if 0 <= idx2 < n2:
                am2[idx2] = 1
    a1 = np.array([has1[i] and not am1[i] and not bad1[i] for i in range(n1)], np.uint8)
    a2 = np.array([has2[i] and not am2[i] and not bad2[i] for i in range(n2)], np.uint8)
    return a1, a2, am1, am2


def _mat_vec_add(A, x, b):
    """cv::Matx33d * cv::Vec3d (s = 0; s += a(i,k) x(k)) + cv::Vec3d."""
    out = []
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += float(A[i][k]) * float(x[k])
        out.append(s + float(b[i]))
    return out


def _world_to_img(cam, x, y, z):
    """cCamModelGeneral_::WorldToImg (src/cam_model_omni.cpp:147-163); cam = c d e u0 v0 invP[12]."""
    norm = math.sqrt(x * x + y * y)
    if norm == 0.0:
        norm = 1e-14
    theta = math.atan(-z / norm)
    rho = 0.0
    for a in cam[5:17][::-1]:
        rho = rho * theta + float(a)
    uu, vv = x / norm * rho, y / norm * rho
    return uu * float(cam[0]) + vv * float(cam[1]) + float(cam[3]), uu * float(cam[2]) + vv + float(cam[4])


def sim3_transforms(kf1, kf2, s12, R12, t12):
    """:1729-1743 -> dict R1w, t1w, R2w, t2w, sR12, sR21, t21, t12."""
    T1, T2 = _inv_mat(np.asarray(kf1["m_t"], np.float64).reshape(4, 4)), _inv_mat(np.asarray(kf2["m_t"], np.float64).reshape(4, 4))
    R12 = np.asarray(R12, np.float64).reshape(3, 3)
    s12 = float(s12)
    sR12 = R12 * s12
    sR21 = R12.T * (1.0 / s12)
    t21 = _matmul_lr(-sR21, np.asarray(t12, np.float64).reshape(3, 1))[:, 0]
    return dict(R1w=T1[:3, :3], t1w=T1[:3, 3], R2w=T2[:3, :3], t2w=T2[:3, 3], sR12=sR12, sR21=sR21, t21=t21,
                t12=np.asarray(t12, np.float64).reshape(3))


def _direction(rig, frm, pts, active, to, Ra, ta, Rb, tb, th, thh, rec):
    """One projection pass (:1779-1872 / :1874-1967): the map points of `frm`'s active slots into
    `to`.  -> (vnMatch, margin); rec gets (keypoint, cam, u, v, radius, list) per GetFeaturesInArea."""
    n = len(frm["kp_xy"])
    C = len(rig["m_c"])
    scale = [float(s) for s in rig["scale"]]
    L = len(scale)
    gp = np.asarray(rig["grid_params"], np.float64)
    mirror = rig["mirror"]
    mh, mw = mirror.shape[1:]
    masked = pts.get("mask") is not None
    grid = np_grid(to["kp_xy"], to["kp_cam"], gp)
    kp_xy = np.asarray(to["kp_xy"], np.float32).reshape(-1, 2).astype(np.float64)
    imc = [_inv_mat(np.asarray(rig["m_c"][c], np.float64).reshape(4, 4)) for c in range(C)]
    match, margin = np.full(n, -1, np.int32), np.inf
    for i in range(n):
        if not active[i]:
            continue
        c = int(frm["kp_cam"][i])
        if c < 0 or c >= C:
            continue
        pa = _mat_vec_add(Ra, pts["pos"][i], ta)
        pb = _mat_vec_add(Rb, pa, tb)
        pc = []
        for r_ in range(3):                       # invMat(M_c) * toVec4d(p): k = 0..3
            s = 0.0
            for k in range(3):
                s += float(imc[c][r_, k]) * pb[k]
            s += float(imc[c][r_, 3]) * 1.0
            pc.append(s)
        if pb[2] < 0.0:                           # the rig-frame z
            continue
        u, v = _world_to_img(np.asarray(rig["cam"][c], np.float64), pc[0], pc[1], pc[2])
        assert math.isfinite(u) and math.isfinite(v)
        margin = min(margin, abs(abs(u - math.floor(u)) - 0.5), abs(abs(v - math.floor(v)) - 0.5))
        ur, vr = int(np.rint(u)), int(np.rint(v))
        if ur >= mw or ur <= 0 or vr >= mh or vr <= 0 or mirror[c][vr, ur] == 0:
            continue
        max_d, min_d = 1.2 * float(pts["dist"][i][1]), 0.8 * float(pts["dist"][i][0])
        d = math.sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2])
        if d < min_d or d > max_d:
            continue
        ratio = d / min_d
        lv = 0
        while lv < L and scale[lv] < ratio:
            lv += 1
        lv = min(lv, L - 1)
        r = th * scale[lv]
        mnx, mny, wi, hi = (float(x) for x in gp[c])
        args = ((u - mnx - r) * wi, (u - mnx + r) * wi, (v - mny - r) * hi, (v - mny + r) * hi)
        margin = min(margin, min(_int_margin(a) for a in args))
        area = []
        rec.append((i, c, u, v, r, lv, area))
        x0 = max(0, math.floor(args[0]))
        if x0 >= COLS:
            continue
        x1 = min(COLS - 1, math.ceil(args[1]))
        if x1 < 0:
            continue
        y0 = max(0, math.floor(args[2]))
        if y0 >= ROWS:
            continue
        y1 = min(ROWS - 1, math.ceil(args[3]))
        if y1 < 0:
            continue
        best, bi = INT_MAX, -1
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for k in grid.get((c, ix, iy), ()):
                    dx, dy = abs(kp_xy[k, 0] - u), abs(kp_xy[k, 1] - v)
                    margin = min(margin, abs(dx - r), abs(dy - r))
                    if not (dx <= r and dy <= r):
                        continue
                    area.append(int(k))
                    oc = int(to["kp_octave"][k])
                    if oc < lv - 1 or oc > lv:
                        continue
                    dist = np_distance(pts["desc"][i], to["desc"][k], pts["mask"][i] if masked else None,
                                       to["mask"][k] if masked else None)
                    if dist < best:
                        best, bi = dist, k
        if best <= thh:
            match[i] = bi
    return match, margin


def np_search_by_sim3(rig, kf1, pts1, kf2, pts2, active1, active2, s12, R12, t12, th, thh):
    """One candidate -> dict: match1 (vnMatch1), match2 (vnMatch2), matches12 (the KF2 keypoint
    whose map point the text writes to vpMatches12[i1], else -1), n_found, margin, and the
    GetFeaturesInArea calls of both directions as (keypoint, cam, u, v, radius, level, list)."""
    x = sim3_transforms(kf1, kf2, s12, R12, t12)
    gfa1, gfa2 = [], []
    m1, g1 = _direction(rig, kf1, pts1, active1, kf2, x["R1w"], x["t1w"], x["sR21"], x["t21"], th, thh, gfa1)
    m2, g2 = _direction(rig, kf2, pts2, active2, kf1, x["R2w"], x["t2w"], x["sR12"], x["t12"], th, thh, gfa2)
    m12 = np.full(len(m1), -1, np.int32)
    for i1, idx2 in enumerate(m1):
        if idx2 >= 0 and m2[idx2] == i1:
            m12[i1] = idx2
    return dict(match1=m1, match2=m2, matches12=m12, n_found=int((m12 >= 0).sum()), margin=min(g1, g2),
                gfa1=gfa1, gfa2=gfa2)


def np_search_batch(rig, kf1, pts1, kf2s, pts2s, active1, active2s, s12, R12, t12, th, thh):
    """The batch the library runs: one np_search_by_sim3 per candidate."""
    rs = [np_search_by_sim3(rig, kf1, pts1, kf2s[t], pts2s[t], active1[t], active2s[t], s12[t], R12[t], t12[t], th, thh)
          for t in range(len(kf2s))]
    return dict(match1=np.stack([r["match1"] for r in rs]), match2=[r["match2"] for r in rs],
                matches12=np.stack([r["matches12"] for r in rs]), n_found=np.array([r["n_found"] for r in rs], np.int32),
                margin=min([r["margin"] for r in rs] + [np.inf]), per=rs)


# ----------------------------------------------------------------------------- scripted inputs
def cayley_rot(c):
    from mcs_amd import fuse
    return fuse.cayley2hom(np.concatenate([np.asarray(c, np.float64), np.zeros(3)]))[:3, :3]


def project_rig(rig, c, p):
    """A rig-frame point into camera c -> (u, v, distance from the camera centre)."""
    imc = np.linalg.inv(np.asarray(rig["m_c"][c], np.float64).reshape(4, 4))
    pc = imc[:3, :3] @ p + imc[:3, 3]
    u, v = _world_to_img(np.asarray(rig["cam"][c], np.float64), float(pc[0]), float(pc[1]), float(pc[2]))
    return u, v, float(np.linalg.norm(pc))


def make_candidate(rig, rng, kf1, pts1, n_per_cam, nbytes, masked, s12, paired=0.65, same_desc=None):
    """A candidate keyframe KF2 for KF1 under a Sim3: for a share of KF1's keypoints the point of
    KF1's slot, taken through the Sim3, lands in the same camera of KF2, where a keypoint of KF2 is
    put (a pixel or two off) whose own map point is the same place in KF2's map; distance ranges
    and descriptors are set so that most such pairs match in both directions, some in one only.
    Fills pts1's dist / desc rows of the paired slots when they are still unset (NaN dist).
    -> (kf2, pts2, s12, R12, t12)."""
    scale = rig["scale"]
    L = len(scale)
    kf2 = make_target(rig, rng, n_per_cam, nbytes, masked)
    if same_desc is not None:
        kf2["desc"][:] = same_desc
    n2 = len(kf2["kp_xy"])
    R12 = cayley_rot(rng.uniform(-0.04, 0.04, 3))
    t12 = rng.uniform(-0.12, 0.12, 3)
    T1 = np.linalg.inv(kf1["m_t"])
    pos2 = np.zeros((n2, 3))
    dist2 = np.zeros((n2, 2))
    desc2 = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
    done = np.zeros(n2, bool)
    for c in range(len(rig["m_c"])):
        i1s, i2s = np.flatnonzero(kf1["kp_cam"] == c), np.flatnonzero(kf2["kp_cam"] == c)
        for i1, i2 in zip(i1s, i2s):
            if rng.random() > paired:
                continue
            p1 = T1[:3, :3] @ pts1["pos"][i1] + T1[:3, 3]
            p2 = (R12.T @ (p1 - t12)) / s12
            u, v, d2 = project_rig(rig, c, p2)
            u, v = u + rng.uniform(-1.5, 1.5), v + rng.uniform(-1.5, 1.5)
            if not (2 < u < W - 2 and 2 < v < H - 2) or rig["mirror"][c][int(round(v)), int(round(u))] == 0:
                continue
            kf2["kp_xy"][i2] = (u, v)
            done[i2] = True
            p2n = p2 + rng.normal(0, 0.002 * d2, 3)
            pos2[i2] = kf2["m_t"][:3, :3] @ p2n + kf2["m_t"][:3, 3]
            _, _, d1 = project_rig(rig, c, s12 * (R12 @ p2n) + t12)
            # levels that let the partner pass: its octave or one above
            l2 = min(int(kf2["kp_octave"][i2]) + int(rng.integers(0, 2)), L - 1) if rng.random() < 0.85 else int(rng.integers(L))
            l1 = min(int(kf1["kp_octave"][i1]) + int(rng.integers(0, 2)), L - 1) if rng.random() < 0.85 else int(rng.integers(L))
            if np.isnan(pts1["dist"][i1][0]):
                dmin = d2 / (0.8 * scale[l2] * rng.uniform(0.86, 0.99))
                pts1["dist"][i1] = (dmin, dmin * rng.uniform(1.5, 12.0))
                pts1["desc"][i1] = _flip(kf2["desc"][i2], int(rng.integers(0, nbytes * 2)), rng)
            dmin = d1 / (0.8 * scale[l1] * rng.uniform(0.86, 0.99))
            dist2[i2] = (dmin, dmin * rng.uniform(1.5, 12.0))
            desc2[i2] = _flip(kf1["desc"][i1], int(rng.integers(0, nbytes * 2)), rng)
    for i2 in np.flatnonzero(~done):              # the rest: somewhere along the keypoint's own ray
        c = int(kf2["kp_cam"][i2])
        M = kf2["m_t"] @ rig["m_c"][c]
        depth = rng.uniform(0.8, 6.0)
        pos2[i2] = M[:3, :3] @ (kf2["rays"][i2] * depth) + M[:3, 3]
        dist2[i2] = (depth / rng.uniform(1.0, 3.0), depth * rng.uniform(1.5, 8.0))
    if same_desc is not None:
        desc2[:] = same_desc
    pts2 = dict(pos=pos2, dist=dist2, desc=desc2,
                mask=rng.integers(0, 256, (n2, nbytes), dtype=np.uint8) if masked else None)
    return kf2, pts2, float(s12), R12, t12


def make_kf1(rig, rng, n_per_cam, nbytes, masked, same_desc=None):
    """KF1 and the map points of its slots, each along its keypoint's ray; dist NaN = not yet set
    (make_candidate sets the paired ones, finish_kf1 the rest)."""
    kf1 = make_target(rig, rng, n_per_cam, nbytes, masked)
    if same_desc is not None:
        kf1["desc"][:] = same_desc
    n1 = len(kf1["kp_xy"])
    pos = np.zeros((n1, 3))
    for i in range(n1):
        M = kf1["m_t"] @ rig["m_c"][int(kf1["kp_cam"][i])]
        pos[i] = M[:3, :3] @ (kf1["rays"][i] * rng.uniform(0.8, 6.0)) + M[:3, 3]
    pts1 = dict(pos=pos, dist=np.full((n1, 2), np.nan), desc=rng.integers(0, 256, (n1, nbytes), dtype=np.uint8),
                mask=rng.integers(0, 256, (n1, nbytes), dtype=np.uint8) if masked else None)
    if same_desc is not None:
        pts1["desc"][:] = same_desc
    return kf1, pts1


def finish_kf1(pts1, rng):
    for i in np.flatnonzero(np.isnan(pts1["dist"][:, 0])):
        d = rng.uniform(0.8, 6.0)
        pts1["dist"][i] = (d / rng.uniform(1.0, 3.0), d * rng.uniform(1.5, 8.0))


def make_case(seed, T=1, n_per_cam=120, nbytes=32, masked=False, s12=1.0, n_cams=3, p_active=0.85, same_desc=False,
              n_per_cam2=None, paired=0.65):
    """-> (rig, kf1, pts1, kf2s, pts2s, active1 [T, n1], active2s, s12 [T], R12 [T, 3, 3], t12 [T, 3])."""
    rng = np.random.default_rng(seed)
    rig = make_rig(n_cams)
    same = rng.integers(0, 256, nbytes, dtype=np.uint8) if same_desc else None
    kf1, pts1 = make_kf1(rig, rng, n_per_cam, nbytes, masked, same)
    n1 = len(kf1["kp_xy"])
    ss = [s12] * T if np.isscalar(s12) else list(s12)
    cands = [make_candidate(rig, rng, kf1, pts1, n_per_cam if n_per_cam2 is None else n_per_cam2, nbytes, masked, ss[t],
                            paired=paired, same_desc=same) for t in range(T)]
    finish_kf1(pts1, rng)
    active1 = (rng.random((T, n1)) < p_active).astype(np.uint8)
    active2s = [(rng.random(len(c[0]["kp_xy"])) < p_active).astype(np.uint8) for c in cands]
    return (rig, kf1, pts1, [c[0] for c in cands], [c[1] for c in cands], active1, active2s,
            np.array([c[2] for c in cands]), np.stack([c[3] for c in cands]) if T else np.zeros((0, 3, 3)),
            np.stack([c[4] for c in cands]) if T else np.zeros((0, 3)))


def coverage(want):
    """The coverage condition of a randomised case: enough mutual matches and a failed agreement."""
    failed = sum(int(((r["match1"] >= 0) & (r["matches12"] < 0)).sum()) for r in want["per"])
    return int(want["n_found"].sum()), failed


# ----------------------------------------------------------------------------- tests (no GPU)
NEW_SYMBOLS = ["mcs_sim3_workspace_create", "mcs_sim3_workspace_destroy", "mcs_search_by_sim3_device",
               "mcs_search_by_sim3"]


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES, s
        assert hasattr(L, s), s


def test_struct_matches_the_header():
    """Field order of the ctypes mirror = the declaration order in include/mcs_matcher.h."""
    import re
    import mcs_amd
    from mcs_amd import sim3_match
    txt = open(os.path.join(mcs_amd.INCLUDE_DIR, "mcs_matcher.h")).read()
    body = re.search(r"typedef struct mcs_sim3_points \{(.*?)\} mcs_sim3_points;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        fields += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    assert fields == [f[0] for f in sim3_match.Sim3Points._fields_]


def test_th_high_is_the_constructor_value():
    from mcs_amd import sim3_match
    for nb in (16, 32, 64):
        for m in (False, True):
            assert sim3_match.th_high(nb, m) == th_high(nb, m)
    assert th_high(32, False) == 96 and th_high(16, True) == 24


def test_active_flags_use_the_first_index_only():
    """:1758-1774 on a hand-written state: a matched point that observes KF2 at keypoints 4 and 7
    marks 4 alone; a first index of -1 (size_t max as int) or >= N2 marks nothing."""
    has1, bad1 = np.array([1, 1, 1, 0, 1], bool), np.array([0, 0, 1, 0, 0], bool)
    has2, bad2 = np.ones(8, bool), np.zeros(8, bool)
    bad2[2] = True
    m12 = np.array([5, -1, -1, -1, 6])
    first = np.array([4, 3, -1, -1, 11])     # row 1 is not matched: its index is never read
    a1, a2, am1, am2 = np_sim3_active(has1, bad1, has2, bad2, m12, first)
    assert am1.tolist() == [1, 0, 0, 0, 1] and am2.tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert a1.tolist() == [0, 1, 0, 0, 0] and a2.tolist() == [1, 1, 0, 1, 0, 1, 1, 1]


CASES = [dict(seed=1, nbytes=32), dict(seed=2, nbytes=16, masked=True), dict(seed=3, nbytes=64),
         dict(seed=4, s12=1.7), dict(seed=5, s12=0.6)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d%s_s%s" % (c.get("nbytes", 32), "m" if c.get("masked") else "",
                                                                    c.get("s12", 1.0)))
def test_restatement_covers_the_branches_with_margin(case):
    """np_search_by_sim3 on the scripted inputs keeps the 1e-9 margin, finds mutual matches, loses
    direction-1 hits to the agreement check, and hits inactive KF2 keypoints."""
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = make_case(**case)
    thh = th_high(case.get("nbytes", 32), case.get("masked", False))
    r = np_search_by_sim3(rig, kf1, pts1, kf2s[0], pts2s[0], a1[0], a2s[0], s12[0], R12[0], t12[0], 10.0, thh)
    assert r["margin"] > MARGIN
    assert r["n_found"] >= 20
    hit = r["match1"] >= 0
    assert (hit & (r["matches12"] < 0)).sum() >= 5
    assert (a2s[0][r["match1"][hit]] == 0).sum() >= 3
    assert len({g[5] for g in r["gfa1"]}) >= 5           # predicted levels spread over the pyramid
    assert (r["match2"] >= 0).sum() > r["n_found"]


def test_rig_frame_depth_test_is_not_the_camera_depth():
    """The Lafida cameras look sideways: points in front of their camera with a negative rig-frame
    z are dropped by :1798, which the restatement reproduces (no window is opened for them)."""
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = make_case(seed=1)
    x = sim3_transforms(kf1, kf2s[0], s12[0], R12[0], t12[0])
    r = np_search_by_sim3(rig, kf1, pts1, kf2s[0], pts2s[0], a1[0], a2s[0], s12[0], R12[0], t12[0], 10.0, 96)
    opened = {g[0] for g in r["gfa1"]}
    n_neg = 0
    for i in np.flatnonzero(a1[0]):
        pb = _mat_vec_add(x["sR21"], _mat_vec_add(x["R1w"], pts1["pos"][i], x["t1w"]), x["t21"])
        if pb[2] < 0.0:
            n_neg += 1
            assert i not in opened and r["match1"][i] == -1
    assert n_neg > 20


# ----------------------------------------------------------------------------- the C ABI without a GPU
def _host_call(edit_arrays=None, edit_structs=None, T=2):
    """mcs_search_by_sim3 through ctypes on a small case -> the return code.  edit_arrays(packed
    arrays by name) runs before the structs are made, edit_structs(k1, p1, k2, p2, pointers by
    name) after."""
    import ctypes
    import mcs_amd
    from mcs_amd import sim3_match as sm
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = make_case(seed=7, T=T, n_per_cam=12)
    nbytes = kf1["desc"].shape[1]
    pk1, pp1, pk2, pp2, A1, A2, S, R, Tt = sm.pack_call(rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12, nbytes, False)
    if edit_arrays:
        edit_arrays(dict(pk1=pk1, pp1=pp1, pk2=pk2, pp2=pp2))
    k1, p1, keep1 = sm.host_sets(pk1, pp1)
    k2, p2, keep2 = sm.host_sets(pk2, pp2)
    n1, n2 = pk1["n_kp_total"], pk2["n_kp_total"]
    m1, m2, m12, nf = np.zeros((T, n1), np.int32), np.zeros(n2, np.int32), np.zeros((T, n1), np.int32), np.zeros(T, np.int32)
    ptrs = dict(a1=A1.ctypes.data, a2=A2.ctypes.data, s=S.ctypes.data, R=R.ctypes.data, t=Tt.ctypes.data,
                m12=m12.ctypes.data, nf=nf.ctypes.data)
    if edit_structs:
        edit_structs(k1, p1, k2, p2, ptrs)
    return mcs_amd.lib().mcs_search_by_sim3(0, ctypes.byref(k1), ctypes.byref(p1), ctypes.byref(k2), ctypes.byref(p2),
                                            ptrs["a1"], ptrs["a2"], ptrs["s"], ptrs["R"], ptrs["t"], 10.0, 96,
                                            m1.ctypes.data, m2.ctypes.data, ptrs["m12"], ptrs["nf"])


def test_host_entry_without_a_device(built):
    import mcs_amd
    if mcs_amd.device_count() > 0:
        pytest.skip("a device is visible")
    assert _host_call() == mcs_amd.MCS_ERR_NO_DEVICE


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


STRUCT_CASES = {
    "bytes_24": lambda k1, p1, k2, p2, a: (_set(k1, bytes=24), _set(k2, bytes=24)),
    "nine_cameras": lambda k1, p1, k2, p2, a: (_set(k1, n_cams=9), _set(k2, n_cams=9)),
    "mask_on_kf1_only": lambda k1, p1, k2, p2, a: _set(k1, mask=k1.desc),
    "mask_on_points_only": lambda k1, p1, k2, p2, a: (_set(p1, mask=p1.desc), _set(p2, mask=p2.desc)),
    "kf1_of_two": lambda k1, p1, k2, p2, a: _set(k1, n_targets=2),
    "kf1_2_pow_19": lambda k1, p1, k2, p2, a: (_set(k1, n_kp_total=1 << 19), _set(p1, n=1 << 19)),
    "null_pos": lambda k1, p1, k2, p2, a: _set(p2, pos=None),
    "null_scale": lambda k1, p1, k2, p2, a: _set(k1, scale=None),
    "null_active1": lambda k1, p1, k2, p2, a: a.__setitem__("a1", None),
    "null_R12": lambda k1, p1, k2, p2, a: a.__setitem__("R", None),
    "null_matches12": lambda k1, p1, k2, p2, a: a.__setitem__("m12", None),
    "n_cams_differ": lambda k1, p1, k2, p2, a: _set(k2, n_cams=2),
    "bytes_differ": lambda k1, p1, k2, p2, a: _set(k2, bytes=64),
    "n_levels_differ": lambda k1, p1, k2, p2, a: _set(k2, n_levels=7),
    "mirror_size_differs": lambda k1, p1, k2, p2, a: _set(k2, mirror_w=700),
    "points_count_differs": lambda k1, p1, k2, p2, a: _set(p2, n=p2.n - 1),
}
ARRAY_CASES = {       # what only the host entry can see: the offsets and the cameras
    "off_decreases": lambda arr: arr["pk2"]["off"].__setitem__(1, arr["pk2"]["off"][2] + 1),
    "off_0_not_zero": lambda arr: arr["pk2"]["off"].__setitem__(0, 1),
    "kp_cam_minus_1": lambda arr: arr["pk1"]["kp_cam"].__setitem__(3, -1),
    "kp_cam_n_cams": lambda arr: arr["pk2"]["kp_cam"].__setitem__(5, 3),
}
ARG_CASES = dict(STRUCT_CASES, **ARRAY_CASES)


@pytest.mark.parametrize("name", sorted(ARG_CASES))
def test_argument_errors_come_before_any_device_use(built, name):
    """Every malformed call returns MCS_ERR_ARG, also on a machine without a device (where a call
    that got as far as the device would return MCS_ERR_NO_DEVICE)."""
    import mcs_amd
    rc = _host_call(edit_arrays=ARRAY_CASES.get(name), edit_structs=STRUCT_CASES.get(name))
    assert rc == mcs_amd.MCS_ERR_ARG, mcs_amd.lib().mcs_last_error()


def test_candidate_of_2_pow_19_keypoints_is_rejected(built):
    import mcs_amd
    from mcs_amd import sim3_match as sm
    rig, kf1, pts1, kf2s, pts2s, a1, a2s, s12, R12, t12 = make_case(seed=7, T=1, n_per_cam=4)
    n = 1 << 19
    big = dict(kf2s[0], kp_xy=np.zeros((n, 2), np.float32), kp_octave=np.zeros(n, np.int32), kp_cam=np.zeros(n, np.int32),
               desc=np.zeros((n, 32), np.uint8), rays=None)
    pbig = dict(pos=np.zeros((n, 3)), dist=np.ones((n, 2)), desc=np.zeros((n, 32), np.uint8), mask=None)
    with pytest.raises(mcs_amd.McsError) as e:
        sm.search_by_sim3(rig, kf1, pts1, [big], [pbig], a1, [np.zeros(n, np.uint8)], s12, R12, t12, 10.0, 96)
    assert e.value.code == mcs_amd.MCS_ERR_ARG and b"2^19" in mcs_amd.lib().mcs_last_error()


# ----------------------------------------------------------------------------- the reference text
def load_scenario(name):
    """One scenario of tests/golden/sim3_ref.npz (written by tests/golden/gen_sim3_ref.py from the
    reference text) -> dict with the inputs in the shapes of this module and the text's records."""
    z = np.load(FIX)
    p = name + "_"
    nbytes, masked, thh = (int(x) for x in z[p + "config"])
    rig = make_rig(3)
    if p + "grid_params" in z.files:
        rig["grid_params"] = z[p + "grid_params"]
    kfs, pts = [], []
    for q in ("k1_", "k2_"):
        kfs.append({k: z[p + q + k] for k in ("kp_xy", "kp_octave", "kp_cam", "desc", "m_t")})
        kfs[-1]["mask"] = z[p + q + "mask"] if masked else None
        pts.append({k: z[p + q + "mp_" + k] for k in ("pos", "dist", "desc")})
        pts[-1]["mask"] = z[p + q + "mp_mask"] if masked else None
    s = dict(name=name, nbytes=nbytes, masked=bool(masked), th_high=thh, th=float(z[p + "th"]), rig=rig, kf1=kfs[0], kf2=kfs[1],
             pts1=pts[0], pts2=pts[1], s12=float(z[p + "s12"]), R12=z[p + "R12"], t12=z[p + "t12"],
             margin=float(z[p + "margin"]))
    for k in ("has1", "bad1", "has2", "bad2", "kp2_mp", "matches12_in", "first_idx", "obs2_ptr", "obs2_idx", "match1",
              "match2", "matches12_out", "n_found", "gfa_key", "gfa_xyr", "gfa_ptr", "gfa_list"):
        s[k] = z[p + k]
    if p + "crafted" in z.files:
        s["crafted"] = {CRAFT[k]: int(i) for i, k in z[p + "crafted"]}
    s["active1"], s["active2"], s["am1"], s["am2"] = np_sim3_active(s["has1"], s["bad1"], s["has2"], s["bad2"],
                                                                    s["matches12_in"], s["first_idx"])
    return s


def restate(s):
    return np_search_by_sim3(s["rig"], s["kf1"], s["pts1"], s["kf2"], s["pts2"], s["active1"], s["active2"], s["s12"],
                             s["R12"], s["t12"], s["th"], s["th_high"])


def expected_matches12(s, matches12):
    """vpMatches12 after the call as the fixture keeps it, map-point ids (kp2_mp: the id in each
    KF2 slot, -1 = NULL): the entries at entry, overwritten by the agreed matches."""
    idx = s["matches12_in"].copy()
    idx[matches12 >= 0] = matches12[matches12 >= 0]
    return np.where(idx >= 0, s["kp2_mp"][np.maximum(idx, 0)], -1).astype(np.int32)


def test_fixture_shape_and_conditions():
    """The fixture is the reference's own result; a scenario that matches nothing proves nothing."""
    z = np.load(FIX)
    assert z["scenarios"].tolist() == SCENARIOS and int(z["n_statements"]) > 100
    assert os.path.getsize(FIX) <= os.path.getsize(os.path.join(HERE, "golden", "fuse_ref.npz"))
    cfg = {n: load_scenario(n) for n in SCENARIOS}
    assert (cfg["b32"]["nbytes"], cfg["b16m"]["nbytes"], cfg["b64"]["nbytes"]) == (32, 16, 64)
    assert cfg["b16m"]["masked"] and not cfg["b32"]["masked"]
    assert cfg["s17"]["s12"] == 1.7 and cfg["s06"]["s12"] == 0.6
    for name, s in cfg.items():
        assert s["margin"] > MARGIN
        assert s["th_high"] == th_high(s["nbytes"], s["masked"])
        assert s["n_found"] == ((s["match1"] >= 0) & (s["match2"][np.maximum(s["match1"], 0)] == np.arange(len(s["match1"])))).sum()
        if name == "edge":
            continue
        assert len(s["kf1"]["kp_xy"]) > 280 and s["n_found"] >= 20
        hit = s["match1"] >= 0
        agreed = hit & (s["match2"][np.maximum(s["match1"], 0)] == np.arange(len(hit)))
        assert (hit & ~agreed).sum() >= 5
        assert (s["active2"][s["match1"][hit]] == 0).sum() >= 3
        assert not np.allclose(s["R12"], np.eye(3)) and np.abs(s["t12"]).min() > 0


def test_edge_scenario_takes_the_intended_branches():
    """What the TEXT did with the crafted slots of KF1 (direction 1) of the edge scenario."""
    s = load_scenario("edge")
    c = s["crafted"]
    assert sorted(c) == sorted(CRAFT)
    calls = {}
    for (d, i, cam), xyr, lo, hi in zip(s["gfa_key"], s["gfa_xyr"], s["gfa_ptr"][:-1], s["gfa_ptr"][1:]):
        if d == 1:
            calls[int(i)] = (xyr, s["gfa_list"][lo:hi].tolist())
    sc, th = s["rig"]["scale"], s["th"]
    # exactly on a bound: inside; one ulp outside: no window
    assert c["lower_exact"] in calls and calls[c["lower_exact"]][0][2] == th * sc[0]
    assert c["upper_exact"] in calls
    assert c["lower_ulp_out"] not in calls and c["upper_ulp_out"] not in calls
    # dist3D / minDistance == scaleFactors[3]: lower_bound stops there
    assert calls[c["ratio_is_scale"]][0][2] == th * sc[3]
    # rig-frame z < 0 although the camera-frame projection is inside the mask: dropped; the converse
    # (rig-frame z >= 0, projection outside the mask): dropped by the mask
    assert c["rig_behind_cam_in_mask"] not in calls and c["rig_front_cam_outside"] not in calls
    x = sim3_transforms(s["kf1"], s["kf2"], s["s12"], s["R12"], s["t12"])
    for key, neg in (("rig_behind_cam_in_mask", True), ("rig_front_cam_outside", False)):
        i = c[key]
        assert s["active1"][i]
        pb = _mat_vec_add(x["sR21"], _mat_vec_add(x["R1w"], s["pts1"]["pos"][i], x["t1w"]), x["t21"])
        assert (pb[2] < 0.0) == neg
        u, v, _ = project_rig(s["rig"], int(s["kf1"]["kp_cam"][i]), np.array(pb))
        inside = 0 < round(u) < W and 0 < round(v) < H and s["rig"]["mirror"][int(s["kf1"]["kp_cam"][i])][round(v), round(u)] > 0
        assert inside == neg
    # octaves level - 2 .. level + 1 in one window, the two admissible ones tie: the first wins
    xyr, lst = calls[c["levels_and_tie"]]
    assert xyr[2] == th * sc[3] and lst[:4] == [0, 1, 2, 3] and len(lst) == 4
    assert s["kf2"]["kp_octave"][:4].tolist() == [1, 2, 3, 4]
    qd = s["pts1"]["desc"][c["levels_and_tie"]]
    dist = [np_distance(qd, s["kf2"]["desc"][k]) for k in range(4)]
    assert dist[0] == 0 and dist[3] == 0 and dist[1] == dist[2] > 0
    assert s["match1"][c["levels_and_tie"]] == 1
    # a matched point observing KF2 at two keypoints: the first is marked, the second stays active
    i = c["two_observations"]
    obs = s["obs2_idx"][s["obs2_ptr"][i]:s["obs2_ptr"][i + 1]].tolist()
    assert len(obs) == 2 and s["matches12_in"][i] >= 0 and s["first_idx"][i] == obs[0]
    assert s["am2"][obs[0]] == 1 and s["am2"][obs[1]] == 0 and s["active2"][obs[1]] == 1
    assert any(d == 2 and k == obs[1] for d, k, _ in s["gfa_key"])      # the text did search from it
    assert not any(d == 2 and k == obs[0] for d, k, _ in s["gfa_key"])
    # a first index outside [0, N2): nothing marked
    i = c["first_index_out_of_range"]
    assert s["matches12_in"][i] >= 0 and not (0 <= s["first_idx"][i] < len(s["has2"]))
    assert s["am1"][i] == 1 and s["am2"].sum() == len({int(f) for f, m in zip(s["first_idx"], s["matches12_in"])
                                                         if m >= 0 and 0 <= f < len(s["has2"])})


@pytest.mark.parametrize("name", SCENARIOS)
def test_restatement_equals_the_text(name):
    """np_search_by_sim3 == the fixture on every array: vnMatch1, vnMatch2, vpMatches12 after the
    call, nFound, and every GetFeaturesInArea call with the list it returned."""
    s = load_scenario(name)
    r = restate(s)
    assert r["margin"] > MARGIN
    assert np.array_equal(r["match1"], s["match1"]) and np.array_equal(r["match2"], s["match2"])
    assert r["n_found"] == int(s["n_found"])
    assert np.array_equal(expected_matches12(s, r["matches12"]), s["matches12_out"])
    mine = [(1,) + g for g in r["gfa1"]] + [(2,) + g for g in r["gfa2"]]
    assert [(d, i, c) for d, i, c, *_ in mine] == [tuple(k) for k in s["gfa_key"].tolist()]
    for (d, i, c, u, v, rad, lv, lst), xyr, lo, hi in zip(mine, s["gfa_xyr"], s["gfa_ptr"][:-1], s["gfa_ptr"][1:]):
        assert abs(u - xyr[0]) < 1e-9 and abs(v - xyr[1]) < 1e-9 and rad == xyr[2]
        assert lst == s["gfa_list"][lo:hi].tolist()


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout")
def test_fixture_regenerates_from_reference_text(tmp_path):
    import subprocess
    import sys
    out = str(tmp_path / "sim3_ref.npz")
    gen = os.path.join(HERE, "golden", "gen_sim3_ref.py")
    subprocess.check_call([sys.executable, gen, "--out", out], stdout=subprocess.DEVNULL)
    a, b = np.load(FIX), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
