"""cLocalMapping::CreateNewMapPoints (reference src/cLocalMapping.cpp:224-386), the parts that need
no GPU:

  np_new_points       a plain Python / NumPy restatement of the per-match loop (:272-364,
                      triangulate_point src/misc.cpp:26-51) plus the admit step (:365-377) for one
                      (KF1, KF2) pair, every operation in the text's order; the 2 x 2 inverse in
                      either form (multiply the adjugate by 1 / det, or divide it by det);
  make_scene          scripted keyframes of the Lafida rig: true 3-D points seen from both keyframes
                      with sub-pixel noise, and the crafted rows of the verdicts 2-7;
  newpoints_ref.npz   what the reference TEXT does on the scenarios of SCENARIOS
                      (tests/golden/gen_newpoints_ref.py): the restatement equals it;
  the C ABI           symbols, struct mirror, MCS_ERR_ARG before any device use,
                      MCS_ERR_NO_DEVICE on a machine without a GPU.

Exact and not exact.  Everything up to x3D (the parallax gate, triangulate_point, Tcw1 * x3D4, the
distances) is plain +, -, *, /, sqrt in a fixed order and is compared bit for bit.  The pixel errors
pass through atan (WorldToImg) and are compared to MARGIN.  A decision is UNSURE when its quantity
lies within relative MARGIN of its threshold (absolute for the thresholds at 0) or when the two
inverse forms give different verdicts; unsure rows are left out of exact comparisons and may make
up at most UNSURE_CAP of the matches of any case.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.test_fuse_ref import MARGIN, _flip, _inv_mat, _matmul_lr, _project, make_rig
from tests.test_sim3solver_ref import _w2i

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "newpoints_ref.npz")
W, H = 754, 480
COS_THRESH = math.cos(3.0 * 3.14159265358979323846 / 180.0)      # src/cLocalMapping.cpp:39
MAX_DIST, MAX_ERR = 25.0, 4.0                                     # :43, :332 / :346
UNSURE_CAP = 0.01
NONE, CREATED, PARALLAX, BEHIND1, REPROJ1, BEHIND2, REPROJ2, DISTANCE = range(8)
QUANTITIES = ("cos", "z1", "err1", "z2", "err2", "dist1", "dist2")
ATAN_QUANTITIES = ("err1", "err2")
# x3D: the largest relative difference between the two 2 x 2 inverse forms over every match of the
# fixture is 1.2325e-14 (test_x3d_tolerance_is_ten_times_the_cpu_spread prints and bounds it; the
# constant is rounded up; the worst rows are the points between the two camera centres).  The device evaluates the stated form in the stated order, so the only
# other difference is its division and square root, which are correctly rounded: 10 x.
CPU_SPREAD = 1.3e-14
TOL_X = 10 * CPU_SPREAD


# ----------------------------------------------------------------------------- the restatement
def _dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s += float(x) * float(y)
    return s


def _norm(a):
    return math.sqrt(_dot(a, a))


def _mv(A, x):
    """cv::Matx * Vec: s = 0; s += a(i,k) * x(k), k ascending."""
    return [_dot(A[i], x) for i in range(len(A))]


def np_triangulate(t12, R12, v1, v2, inv_form="mul"):
    """triangulate_point (src/misc.cpp:26-51).  Matx22d::inv() is OpenCV's: d = 1 / det and the
    adjugate times d (`mul`, what the library and the fixture's stand-in use), a zero matrix when
    det == 0; `div` divides the adjugate by det instead and serves to measure the spread."""
    f2 = _mv(R12, v2)
    b = [_dot(t12, v1), _dot(t12, f2)]
    A00, A10 = _dot(v1, v1), _dot(v1, f2)
    A01, A11 = -A10, -_dot(f2, f2)
    det = A00 * A11 - A01 * A10
    if det == 0.0:
        inv = [[0.0, 0.0], [0.0, 0.0]]
    elif inv_form == "mul":
        d = 1.0 / det
        inv = [[A11 * d, -A01 * d], [-A10 * d, A00 * d]]
    else:
        inv = [[A11 / det, -A01 / det], [-A10 / det, A00 / det]]
    lam = _mv(inv, b)
    return [((v1[i] * lam[0]) + (t12[i] + f2[i] * lam[1])) / 2.0 for i in range(3)]


def _rel_close(x, th):
    return abs(x - th) <= MARGIN * abs(th) if th != 0.0 else abs(x) <= MARGIN


def np_match(T1, T1i, T2, T2i, cam1, cam2, Ow1, Ow2, ray1, ray2, kp1, kp2, inv_form="mul"):
    """:287-364 for one match -> (verdict, x3D or None, the compared quantities, unsure).  T* are
    Get_MtMc (camera -> world, the text calls them Tcw) and their invMat, as 4 x 4 arrays."""
    q = dict.fromkeys(QUANTITIES, float("nan"))
    unsure = False
    with np.errstate(all="ignore"):
        Rcw1, Rcw2 = T1[:3, :3], T2[:3, :3]
        rr1, rr2 = _mv(Rcw1, ray1), _mv(Rcw2, ray2)
        den = _norm(rr1) * _norm(rr2)
        q["cos"] = cosp = _dot(rr1, rr2) / den if den != 0.0 else float("nan")
        unsure |= _rel_close(cosp, 0.0) or _rel_close(cosp, COS_THRESH)
        if cosp < 0 or cosp > COS_THRESH:
            return PARALLAX, None, q, unsure
        rel = _matmul_lr(T1i, T2)
        x3 = np_triangulate([float(rel[i, 3]) for i in range(3)], rel[:3, :3], ray1, ray2, inv_form)
        x4 = _mv(T1, x3 + [1.0])                       # x3D4 = Tcw1 * x3D4, fourth row 0 0 0 1
        X = x4[:3]
        for tag, Ti, cam, kp, behind, reproj in (("1", T1i, cam1, kp1, BEHIND1, REPROJ1), ("2", T2i, cam2, kp2, BEHIND2, REPROJ2)):
            pr = _mv(Ti, x4)
            q["z" + tag] = pr[2]
            unsure |= _rel_close(pr[2], 0.0)
            if pr[2] <= 0.0:
                return behind, X, q, unsure
            u, v = _w2i(cam, pr[0], pr[1], pr[2])
            ex, ey = float(u) - float(np.float32(kp[0])), float(v) - float(np.float32(kp[1]))
            q["err" + tag] = err = math.sqrt(ex * ex + ey * ey)
            unsure |= _rel_close(err, MAX_ERR)
            if err > MAX_ERR:
                return reproj, X, q, unsure
        q["dist1"] = d1 = _norm([X[i] - float(Ow1[i]) for i in range(3)])
        q["dist2"] = d2 = _norm([X[i] - float(Ow2[i]) for i in range(3)])
        unsure |= _rel_close(d1, MAX_DIST) or _rel_close(d2, MAX_DIST) or _rel_close(d1, 0.0) or _rel_close(d2, 0.0)
        if d1 == 0 or d2 == 0 or d1 > MAX_DIST or d2 > MAX_DIST:
            return DISTANCE, X, q, unsure
    return CREATED, X, q, unsure


def np_admit(X, Ow1, Ow2, kf2_first, level, scale):
    """UpdateNormalAndDepth (src/cMapPoint.cpp:453-496) for the observations {KF1, KF2} in the
    map's order, reference keyframe KF1 -> (normal, mfMinDistance, mfMaxDistance)."""
    normal = [0.0, 0.0, 0.0]
    for O in ((Ow2, Ow1) if kf2_first else (Ow1, Ow2)):
        ni = [X[i] - float(O[i]) for i in range(3)]
        ia = 1.0 / _norm(ni)
        normal = [normal[i] + ni[i] * ia for i in range(3)]
    dist = _norm([X[i] - float(Ow1[i]) for i in range(3)])
    sf = float(scale[level])
    half = 1.0 / 2
    return [x * half for x in normal], (1.0 / sf) * dist / sf, sf * dist * float(scale[len(scale) - 1 - level])


def np_new_points(rig, kf1, kf2, matches12, kf2_first, inv_form="mul"):
    """The per-match loop and the admit step for one neighbour -> dict: verdict uint8 [n1], x3d
    [n1, 3] and q [n1, 7] (NaN where the text does not get there), unsure bool [n1], and the created
    points in idx1 order: kp1, kp2, pos, normal, min_dist, max_dist, desc, mask."""
    n1, n2, C = len(kf1["kp_xy"]), len(kf2["kp_xy"]), len(rig["m_c"])
    Mt1, Mt2 = (np.asarray(k["m_t"], np.float64).reshape(4, 4) for k in (kf1, kf2))
    Mc = [np.asarray(m, np.float64).reshape(4, 4) for m in rig["m_c"]]
    T1 = [_matmul_lr(Mt1, m) for m in Mc]
    T2 = [_matmul_lr(Mt2, m) for m in Mc]
    T1i, T2i = [_inv_mat(m) for m in T1], [_inv_mat(m) for m in T2]
    Ow1, Ow2 = Mt1[:3, 3], Mt2[:3, 3]
    out = dict(verdict=np.zeros(n1, np.uint8), x3d=np.full((n1, 3), np.nan), q=np.full((n1, len(QUANTITIES)), np.nan),
               unsure=np.zeros(n1, bool))
    pts = {k: [] for k in ("kp1", "kp2", "pos", "normal", "min_dist", "max_dist", "desc", "mask")}
    scale, L = rig["scale"], len(rig["scale"])
    for i1 in range(n1):
        m = int(matches12[i1])
        if m < 0 or m >= n2:
            continue
        c1, c2 = int(kf1["kp_cam"][i1]), int(kf2["kp_cam"][m])
        if not (0 <= c1 < C and 0 <= c2 < C):
            continue
        v, X, q, unsure = np_match(T1[c1], T1i[c1], T2[c2], T2i[c2], rig["cam"][c1], rig["cam"][c2], Ow1, Ow2,
                                   [float(x) for x in kf1["rays"][i1]], [float(x) for x in kf2["rays"][m]],
                                   kf1["kp_xy"][i1], kf2["kp_xy"][m], inv_form)
        out["verdict"][i1], out["unsure"][i1] = v, unsure
        out["q"][i1] = [q[k] for k in QUANTITIES]
        if X is not None:
            out["x3d"][i1] = X
        if v != CREATED:
            continue
        level = min(max(int(kf1["kp_octave"][i1]), 0), L - 1)
        normal, dmin, dmax = np_admit(X, Ow1, Ow2, kf2_first, level, scale)
        src, row = (kf2, m) if kf2_first else (kf1, i1)
        for k, val in (("kp1", i1), ("kp2", m), ("pos", X), ("normal", normal), ("min_dist", dmin), ("max_dist", dmax),
                       ("desc", src["desc"][row]), ("mask", src["mask"][row] if src.get("mask") is not None else None)):
            pts[k].append(val)
    nb = np.asarray(kf1["desc"]).shape[1]
    out.update(kp1=np.array(pts["kp1"], np.int32), kp2=np.array(pts["kp2"], np.int32),
               pos=np.array(pts["pos"], np.float64).reshape(-1, 3), normal=np.array(pts["normal"], np.float64).reshape(-1, 3),
               min_dist=np.array(pts["min_dist"], np.float64), max_dist=np.array(pts["max_dist"], np.float64),
               desc=np.array(pts["desc"], np.uint8).reshape(-1, nb),
               mask=np.array(pts["mask"], np.uint8).reshape(-1, nb) if kf1.get("mask") is not None else None)
    return out


def np_both_forms(rig, kf1, kf2, matches12, kf2_first):
    """The restatement under both inverse forms -> (result of `mul` with the rows whose verdict
    differs under `div` marked unsure, the largest relative difference of x3D between the forms)."""
    a = np_new_points(rig, kf1, kf2, matches12, kf2_first, "mul")
    b = np_new_points(rig, kf1, kf2, matches12, kf2_first, "div")
    a["unsure"] = a["unsure"] | (a["verdict"] != b["verdict"])
    both = np.isfinite(a["x3d"]).all(1) & np.isfinite(b["x3d"]).all(1)
    spread = 0.0
    if both.any():
        d = np.abs(a["x3d"][both] - b["x3d"][both]).max(1) / np.abs(a["x3d"][both]).max(1)
        spread = float(d.max())
    return a, spread


# ----------------------------------------------------------------------------- scripted scenes
# the fixture's scenarios: (name, seed, keypoints per camera, bytes, masked, neighbour kinds, kf2_first)
SCENARIOS = [("orb", 11, 80, 32, False, ("normal", "short", "wide"), (0, 1, 0)),
             ("m16", 12, 60, 16, True, ("normal", "wide"), (1, 0)),
             ("b64", 13, 120, 64, False, ("wide", "normal"), (0, 1))]
KINDS = ("true", "far", "mirror1", "mirror2", "noise1", "noise2", "beyond")
# neighbour kinds: translation of the neighbour's rig centre from the current keyframe's (metres)
BASELINES = {"normal": 0.45, "short": 0.04, "wide": 2.0}


def _pose(rng, centre):
    return np.concatenate([rng.uniform(-0.03, 0.03, 3), centre])


def _pixels(rig, rng, c, n):
    """n pixels inside camera c's mirror mask and the image, as make_target draws them."""
    ang, rad = rng.uniform(0, 2 * np.pi, n), 200.0 * np.sqrt(rng.uniform(0.02, 1.0, n))
    p = np.stack([rig["cams"][c]["u0"] + rad * np.cos(ang), rig["cams"][c]["v0"] + rad * np.sin(ang)], 1)
    return p[(p[:, 0] > 12) & (p[:, 0] < W - 12) & (p[:, 1] > 12) & (p[:, 1] < H - 12)]


def _rays(rig, c, xy):
    from mcs_amd import synth
    xy = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    return np.stack(synth.img_to_world(rig["cams"][c], xy[:, 0], xy[:, 1]), 1).reshape(-1, 3)


def make_scene(seed, n_per_cam=40, nbytes=32, masked=False, neighbours=("normal", "wide"), n_cams=3, tracked=0.0,
               kinds=KINDS, only_cam=None, fill=0.35):
    """A current keyframe and its neighbours with known correspondences.

    Every KF1 keypoint stands for a 3-D point along its bearing ray; what is put into a neighbour
    depends on the keypoint's kind:
      true     depth 0.8 .. 6 m, projected into the neighbour with sub-pixel noise
      far      depth 60 .. 200 m: no parallax on a `normal` or `short` baseline (verdict 2)
      mirror1  the point mirrored through camera 1's centre, seen by the neighbour through ITS
               centre: both rays point away from it (verdict 3)
      mirror2  a point between camera 1's centre and the `wide` (else the last) neighbour's, whose
               keypoint there is the projection of the point mirrored through that neighbour's
               camera centre: the rays still enclose an angle below 90 degrees, the point lies in
               front of camera 1 and, where the neighbour is ahead, behind camera 2 (verdict 5)
      noise1   6 pixels of noise on KF1's keypoint only; with the point nearer to the neighbour the
               midpoint's error is larger in the neighbour (verdict 6)
      noise2   6 pixels of noise on the neighbour's keypoint only (verdict 4 likewise)
      beyond   depth 26 .. 40 m, which a `wide` (2 m) baseline still triangulates (verdict 7)
    -> (rig, kf1, kf2s, truth) with truth[t] int32 [n1]: the neighbour's keypoint of KF1's keypoint
    i, -1 where the point does not fall into the neighbour's image.  Keyframes are the dicts of
    mcs_amd.fuse plus pose6 (the Cayley 6-vector) and has_mp (uint8, `tracked` of them set)."""
    from mcs_amd import fuse
    rng = np.random.default_rng(seed)
    rig = make_rig(n_cams)
    C = n_cams
    cam_d = [np.asarray(rig["cam"][c], np.float64) for c in range(C)]
    pose1 = _pose(rng, rng.uniform(-0.05, 0.05, 3))
    Mt1 = fuse.cayley2hom(pose1)
    poses2 = []
    for kind in neighbours:
        direction = rng.normal(size=3)
        poses2.append(_pose(rng, pose1[3:] + BASELINES[kind] * direction / np.linalg.norm(direction)))
    t_mirror = neighbours.index("wide") if "wide" in neighbours else len(neighbours) - 1
    Mt_mirror = fuse.cayley2hom(poses2[t_mirror])
    xy1, cam1, kind1 = [], [], []
    for c in range(C):
        if only_cam is not None and c != only_cam:
            continue
        p = _pixels(rig, rng, c, n_per_cam)
        xy1.append(p)
        cam1.append(np.full(len(p), c, np.int32))
        kind1.append(rng.choice(len(kinds), len(p), p=_kind_weights(kinds)))
    xy1, cam1 = np.concatenate(xy1), np.concatenate(cam1)
    kind1 = np.array([KINDS.index(kinds[k]) for k in np.concatenate(kind1)], np.int32)
    n1 = len(xy1)
    K = {k: KINDS.index(k) for k in KINDS}
    depth = rng.uniform(0.8, 6.0, n1)
    depth = np.where(kind1 == K["far"], rng.uniform(60, 200, n1), depth)
    depth = np.where(kind1 == K["beyond"], rng.uniform(26, 40, n1), depth)
    depth = np.where(np.isin(kind1, (K["noise1"], K["noise2"])), rng.uniform(0.7, 2.2, n1), depth)
    P = np.zeros((n1, 3))
    for c in range(C):
        s = cam1 == c
        M = Mt1 @ rig["m_c"][c]
        d = np.where(kind1[s] == K["mirror1"], -depth[s], depth[s])
        P[s] = (_rays(rig, c, xy1[s]) * d[:, None]) @ M[:3, :3].T + M[:3, 3]
        for i in np.flatnonzero(s & (kind1 == K["mirror2"])):      # a point between the two camera centres
            C1, C2 = M[:3, 3], (Mt_mirror @ rig["m_c"][c])[:3, 3]
            off = rng.normal(size=3)
            X = (C1 + C2) / 2 + 0.35 * np.linalg.norm(C2 - C1) * rng.uniform(0.2, 1.0) * off / np.linalg.norm(off)
            u, v = _project(M, cam_d[c], X[None])
            if _inside(rig, c, np.stack([u, v], 1))[0]:
                xy1[i], P[i] = (u[0], v[0]), X
            else:
                kind1[i] = K["true"]
    noisy1 = kind1 == K["noise1"]
    ang = rng.uniform(0, 2 * np.pi, n1)
    xy1 = np.where(noisy1[:, None], xy1 + 6.0 * np.stack([np.cos(ang), np.sin(ang)], 1), xy1).astype(np.float32)
    rays1 = np.concatenate([_rays(rig, c, xy1[cam1 == c]) for c in range(C)]) if n1 else np.zeros((0, 3))
    desc1 = rng.integers(0, 256, (n1, nbytes), dtype=np.uint8)
    kf1 = dict(kp_xy=xy1, kp_octave=rng.integers(0, 8, n1).astype(np.int32), kp_cam=cam1, desc=desc1,
               mask=_masks(rng, n1, nbytes) if masked else None, rays=rays1, m_t=Mt1, pose6=pose1,
               has_mp=(rng.random(n1) < tracked).astype(np.uint8), kind=kind1)
    kf2s, truth = [], []
    for t, pose2 in enumerate(poses2):
        Mt2 = fuse.cayley2hom(pose2)
        xy2, cam2, desc2, src = [], [], [], []
        for c in range(C):
            s = np.flatnonzero(cam1 == c)
            M = Mt2 @ rig["m_c"][c]
            Pc = P[s].copy()
            flip = (kind1[s] == K["mirror1"]) | ((kind1[s] == K["mirror2"]) & (t == t_mirror))
            Pc[flip] = 2.0 * M[:3, 3] - Pc[flip]
            u, v = _project(M, cam_d[c], Pc) if len(s) else (np.zeros(0), np.zeros(0))
            a = rng.uniform(0, 2 * np.pi, len(s))
            r = np.where(kind1[s] == K["noise2"], 6.0, rng.uniform(0.0, 0.6, len(s)))
            uv = np.stack([u + r * np.cos(a), v + r * np.sin(a)], 1)
            ok = _inside(rig, c, uv)
            extra = _pixels(rig, rng, c, int(fill * n_per_cam)) if only_cam is None or c == only_cam else np.zeros((0, 2))
            rows = np.concatenate([uv[ok], extra])
            d = np.concatenate([np.stack([_flip(desc1[i], int(rng.integers(0, 5)), rng) for i in s[ok]]).reshape(-1, nbytes),
                                rng.integers(0, 256, (len(extra), nbytes), dtype=np.uint8)])
            origin = np.concatenate([s[ok], np.full(len(extra), -1)])
            order = rng.permutation(len(rows))
            xy2.append(rows[order])
            cam2.append(np.full(len(rows), c, np.int32))
            desc2.append(d[order])
            src.append(origin[order])
        xy2 = np.concatenate(xy2).astype(np.float32)
        cam2, desc2, src = np.concatenate(cam2), np.concatenate(desc2), np.concatenate(src)
        n2 = len(xy2)
        rays2 = np.concatenate([_rays(rig, c, xy2[cam2 == c]) for c in range(C)]) if n2 else np.zeros((0, 3))
        m2 = None
        if masked:                      # the matched rows share most of their mask with KF1's row
            m2 = _masks(rng, n2, nbytes)
            for k in np.flatnonzero(src >= 0):
                m2[k] = _flip(kf1["mask"][src[k]], 2, rng)
        kf2s.append(dict(kp_xy=xy2, kp_octave=rng.integers(0, 8, n2).astype(np.int32), kp_cam=cam2, desc=desc2, mask=m2,
                         rays=rays2, m_t=Mt2, pose6=pose2, has_mp=(rng.random(n2) < tracked).astype(np.uint8)))
        t = np.full(n1, -1, np.int32)
        t[src[src >= 0]] = np.flatnonzero(src >= 0)
        truth.append(t)
    return rig, kf1, kf2s, truth


def _kind_weights(kinds):
    w = np.array([5.0 if k == "true" else 1.0 for k in kinds])
    return w / w.sum()


def _inside(rig, c, uv):
    """uv [n, 2] finite, 8 pixels inside the image and on camera c's mirror mask."""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(uv).all(1) & (uv[:, 0] > 8) & (uv[:, 0] < W - 8) & (uv[:, 1] > 8) & (uv[:, 1] < H - 8)
    ok[ok] &= rig["mirror"][c][np.rint(uv[ok, 1]).astype(int), np.rint(uv[ok, 0]).astype(int)] > 0
    return ok


def _masks(rng, n, nbytes, keep=0.85):
    return np.packbits((rng.random((n, nbytes * 8)) < keep).astype(np.uint8), axis=1)


# ----------------------------------------------------------------------------- the fixture and the GPU cases
_CACHE = {}


def fixture():
    if "fix" not in _CACHE:
        _CACHE["fix"] = dict(np.load(FIX))
    return _CACHE["fix"]


def load_scenario(name):
    """-> (rig, kf1, kf2s, truth, rows per neighbour, kf2_first) of a fixture scenario."""
    z = fixture()
    p = name + "_"
    _, _, nbytes, masked, T = (int(x) for x in z[p + "config"])
    keys = ("kp_xy", "kp_octave", "kp_cam", "desc", "rays", "m_t", "pose6", "has_mp") + (("mask",) if masked else ())
    kf = lambda tag: dict({k: z[p + tag + k] for k in keys}, mask=z[p + tag + "mask"] if masked else None)  # noqa: E731
    return (make_rig(3), kf("k1_"), [kf("k2_%d_" % t) for t in range(T)], [z[p + "truth_%d" % t] for t in range(T)],
            [z[p + "rows_%d" % t] for t in range(T)], z[p + "kf2_first"])


# name -> what make_scene is called with; every case is one (KF1, KF2) pair with its match list
GPU_CASES = {
    "c3x40": dict(seed=21, n_per_cam=40),                                   # less than one block
    "c3x120": dict(seed=22, n_per_cam=120, neighbours=("wide", "normal")),  # crosses a block of the compaction
    "no_match": dict(seed=23, n_per_cam=40, matches="none"),
    "all_created": dict(seed=24, n_per_cam=60, kinds=("true",), matches="created"),
    "last_cam": dict(seed=25, n_per_cam=60, matches="last_cam"),
    "m16": dict(seed=26, n_per_cam=50, nbytes=16, masked=True),
    "b64": dict(seed=27, n_per_cam=50, nbytes=64),
}


def gpu_case(name):
    """-> dict: rig, kf1, kf2, matches12, kf2_first and `want` = the restatement (both forms, unsure
    rows marked), computed once per session and shared."""
    if ("case", name) in _CACHE:
        return _CACHE["case", name]
    kw = dict(GPU_CASES[name])
    how = kw.pop("matches", "truth")
    rig, kf1, kf2s, truth = make_scene(**kw)
    t = len(kf2s) - 1
    kf2, m12 = kf2s[t], truth[t].copy()
    kf2_first = int(kw["seed"] % 2)
    if how == "none":
        m12[:] = -1
    elif how == "last_cam":
        m12[kf1["kp_cam"] != len(rig["m_c"]) - 1] = -1
    elif how == "created":
        m12[np_new_points(rig, kf1, kf2, m12, kf2_first)["verdict"] != CREATED] = -1
    want, spread = np_both_forms(rig, kf1, kf2, m12, kf2_first)
    c = dict(rig=rig, kf1=kf1, kf2=kf2, matches12=m12, kf2_first=kf2_first, want=want, spread=spread)
    _CACHE["case", name] = c
    return c


# the full loop: T = 3 neighbours, the second skipped, 30 % of the keypoints tracked already
LOOP_CASE = dict(seed=31, n_per_cam=70, neighbours=("normal", "normal", "wide"), tracked=0.3)
LOOP_SKIP, LOOP_KF2_FIRST, EPI_THRESH = (0, 1, 0), (1, 0, 0), 1e-2


def th_low(nbytes, masked):
    return nbytes if masked else 2 * nbytes


def np_loop(rig, kf1, kf2s, skip, kf2_first, update_flags=True):
    """The neighbour loop (:241-384) evaluated sequentially on the CPU: the matcher oracle
    (tests/oracle_bind.py), then the restatement, then the flag update, neighbour by neighbour.
    update_flags=False searches every neighbour with the flags at entry (two independent passes).
    -> (points: list of (neighbour, restatement dict), has_mp per keyframe, matches12 [T, n1])."""
    import ctypes as ct
    from tests import oracle_bind as ob
    from mcs_amd import synth
    p = ob._p
    C, nb = len(rig["m_c"]), kf1["desc"].shape[1]
    masked = kf1.get("mask") is not None
    has = [kf1["has_mp"].copy()] + [k["has_mp"].copy() for k in kf2s]
    n1 = len(kf1["kp_xy"])
    out, m12s = [], np.full((len(kf2s), n1), -1, np.int32)
    mc6 = np.array(synth.LAFIDA_MC[:C], np.float64)
    c_ = lambda a, dt: np.ascontiguousarray(a, dt)  # noqa: E731
    for t, kf2 in enumerate(kf2s):
        if skip[t]:
            continue
        E = ob.compute_e_rig(kf1["pose6"], kf2["pose6"], mc6)
        ref = np.zeros(n1, np.int32)
        h1 = has[0] if update_flags else kf1["has_mp"]
        ob.lib().oracle_search_for_triangulation_raw_ex(
            p(c_(kf1["desc"], np.uint8)), p(c_(kf1["mask"], np.uint8)) if masked else None, n1,
            p(c_(kf2["desc"], np.uint8)), p(c_(kf2["mask"], np.uint8)) if masked else None, len(kf2["kp_xy"]), nb,
            p(c_(kf1["kp_cam"], np.int32)), p(c_(kf2["kp_cam"], np.int32)), p(c_(h1, np.uint8)), p(c_(has[t + 1], np.uint8)),
            p(c_(kf1["rays"], np.float64)), p(c_(kf2["rays"], np.float64)), p(c_(E, np.float64)),
            ct.c_double(EPI_THRESH), C, p(ref))
        m12s[t] = ref
        r, _ = np_both_forms(rig, kf1, kf2, ref, kf2_first[t])
        out.append((t, r))
        has[0][r["kp1"]] = 1
        has[t + 1][r["kp2"]] = 1
    return out, has, m12s


def loop_case():
    if "loop" not in _CACHE:
        rig, kf1, kf2s, _ = make_scene(**LOOP_CASE)
        pts, has, m12 = np_loop(rig, kf1, kf2s, LOOP_SKIP, LOOP_KF2_FIRST)
        _CACHE["loop"] = dict(rig=rig, kf1=kf1, kf2s=kf2s, points=pts, has=has, matches12=m12)
    return _CACHE["loop"]


# ----------------------------------------------------------------------------- tests (no GPU)
@pytest.mark.parametrize("name", [s[0] for s in SCENARIOS])
def test_scenes_regenerate_and_fixture_holds_them(name):
    sc = next(s for s in SCENARIOS if s[0] == name)
    rig, kf1, kf2s, truth = make_scene(sc[1], n_per_cam=sc[2], nbytes=sc[3], masked=sc[4], neighbours=sc[5])
    _, f1, f2s, ftruth, rows, kf2_first = load_scenario(name)
    for a, b in [(kf1, f1)] + list(zip(kf2s, f2s)):
        for k in ("kp_xy", "kp_octave", "kp_cam", "desc", "rays", "m_t"):
            assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(truth, ftruth)) and tuple(kf2_first) == sc[6]
    for kf2 in kf2s:
        per_cam = np.bincount(kf2["kp_cam"], minlength=3)
        assert (per_cam >= 40).all() and (np.bincount(kf1["kp_cam"]) <= 120).all()


def test_fixture_covers_every_branch():
    seen, firsts, masked16, b64 = np.zeros(8, np.int64), set(), False, False
    for name, _, _, nbytes, masked, _, kf2_first in SCENARIOS:
        rows = load_scenario(name)[4]
        for r in rows:
            seen += np.bincount(r[:, 2].astype(int), minlength=8)
        firsts |= set(kf2_first)
        masked16 |= masked and nbytes == 16
        b64 |= nbytes == 64
    print("verdict counts 0..7 over the fixture:", seen.tolist())
    assert (seen[1:] > 0).all() and seen[0] == 0
    assert firsts == {0, 1} and masked16 and b64


@pytest.mark.parametrize("name", [s[0] for s in SCENARIOS])
def test_restatement_equals_the_text(name):
    """Every verdict; x3D and the quantities that do not pass through atan bit for bit; the pixel
    errors to MARGIN.  Unsure rows are left out (none may be needed: the generator keeps 1e-6)."""
    rig, kf1, kf2s, truth, rows, kf2_first = load_scenario(name)
    for t, kf2 in enumerate(kf2s):
        r, _ = np_both_forms(rig, kf1, kf2, truth[t], kf2_first[t])
        i1 = rows[t][:, 0].astype(int)
        assert np.array_equal(i1, np.flatnonzero(truth[t] >= 0)) and np.array_equal(rows[t][:, 1].astype(int), truth[t][i1])
        sure = ~r["unsure"][i1]
        assert (~sure).sum() <= UNSURE_CAP * len(i1)
        assert np.array_equal(r["verdict"][i1][sure], rows[t][:, 2].astype(np.uint8)[sure])
        assert r["x3d"][i1][sure].tobytes() == rows[t][:, 10:13][sure].tobytes()
        for k, col in zip(QUANTITIES, range(3, 10)):
            got, want = r["q"][i1, QUANTITIES.index(k)][sure], rows[t][:, col][sure]
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            ok = ~np.isnan(want)
            if k in ATAN_QUANTITIES:
                assert np.all(np.abs(got[ok] - want[ok]) <= MARGIN * np.maximum(1.0, np.abs(want[ok]))), k
            else:
                assert got[ok].tobytes() == want[ok].tobytes(), k


def test_x3d_tolerance_is_ten_times_the_cpu_spread():
    """The two 2 x 2 inverse forms over every match of the fixture."""
    worst = 0.0
    for name in (s[0] for s in SCENARIOS):
        rig, kf1, kf2s, truth, _, kf2_first = load_scenario(name)
        for t, kf2 in enumerate(kf2s):
            worst = max(worst, np_both_forms(rig, kf1, kf2, truth[t], kf2_first[t])[1])
    print("largest relative difference of x3D between the inverse forms: %.3g" % worst)
    assert 0.0 < worst <= CPU_SPREAD and CPU_SPREAD <= 2.0 * worst
    assert TOL_X == 10 * CPU_SPREAD


def test_unsure_rows_stay_under_the_cap():
    """The fixture and every GPU case's restatement, each on its own."""
    for name in (s[0] for s in SCENARIOS):
        rig, kf1, kf2s, truth, _, kf2_first = load_scenario(name)
        for t, kf2 in enumerate(kf2s):
            r, _ = np_both_forms(rig, kf1, kf2, truth[t], kf2_first[t])
            n = int((truth[t] >= 0).sum())
            print("fixture", name, t, "unsure", int(r["unsure"].sum()), "of", n)
            assert r["unsure"].sum() <= UNSURE_CAP * n
    for name in GPU_CASES:
        c = gpu_case(name)
        n = int((c["matches12"] >= 0).sum())
        print("case", name, "unsure", int(c["want"]["unsure"].sum()), "of", n, "spread %.3g" % c["spread"])
        assert c["want"]["unsure"].sum() <= UNSURE_CAP * n
        assert c["spread"] <= TOL_X            # the tolerance covers what the inverse form changes on the case
    lc = loop_case()
    for t, r in lc["points"]:
        n = int((lc["matches12"][t] >= 0).sum())
        print("loop neighbour", t, "unsure", int(r["unsure"].sum()), "of", n)
        assert r["unsure"].sum() <= UNSURE_CAP * n


def test_gpu_cases_have_the_shapes_they_are_for():
    a, b = gpu_case("c3x40"), gpu_case("c3x120")
    assert len(a["kf1"]["kp_xy"]) < 256 and len(a["want"]["kp1"]) > 10
    n1 = len(b["kf1"]["kp_xy"])
    assert n1 > 256 and n1 % 64 != 0 and n1 % 256 != 0
    kp1 = b["want"]["kp1"]
    assert (kp1 < 256).any() and (kp1 >= 256).any()            # survivors on both sides of the block boundary
    assert set(np.unique(b["want"]["verdict"])) >= {0, 1, 2, 3}
    assert (gpu_case("no_match")["matches12"] < 0).all()
    c = gpu_case("all_created")
    assert (c["want"]["verdict"][c["matches12"] >= 0] == CREATED).all() and (c["matches12"] >= 0).sum() > 50
    c = gpu_case("last_cam")
    assert (c["kf1"]["kp_cam"][c["matches12"] >= 0] == 2).all() and (c["matches12"] >= 0).sum() > 20
    assert gpu_case("m16")["kf1"]["mask"] is not None and gpu_case("b64")["kf1"]["desc"].shape[1] == 64


def test_admit_step_equals_the_mapside_restatements(built):
    """Normal, min_dist, max_dist, descriptor and mask of every created point against the existing
    restatements of UpdateNormalAndDepth / ComputeDistinctiveDescriptors (the oracle of
    tests/test_mapside_ref.py) on the two-observation lists in the map's order."""
    from tests import oracle_bind as ob
    for name in ("c3x120", "m16", "b64"):
        c = gpu_case(name)
        w, kf1, kf2 = c["want"], c["kf1"], c["kf2"]
        P = len(w["kp1"])
        assert P > 10
        n1, nb = len(kf1["kp_xy"]), kf1["desc"].shape[1]
        masked = kf1["mask"] is not None
        first, second = ((n1 + w["kp2"], w["kp1"]) if c["kf2_first"] else (w["kp1"], n1 + w["kp2"]))
        rows = np.ascontiguousarray(np.stack([first, second], 1).reshape(-1).astype(np.int32))
        ptr = np.arange(0, 2 * P + 1, 2, dtype=np.int32)
        desc = np.ascontiguousarray(np.concatenate([kf1["desc"], kf2["desc"]]))
        dmask = np.ascontiguousarray(np.concatenate([kf1["mask"], kf2["mask"]])) if masked else None
        best = np.full(P, -7, np.int32)
        ob.lib().oracle_distinctive_descriptors(ob._p(desc), ob._p(dmask) if masked else None, nb, ob._p(ptr), ob._p(rows), P,
                                                ob._p(best))
        assert (best == 0).all()
        assert np.array_equal(w["desc"], desc[rows[ptr[:-1] + best]])
        if masked:
            assert np.array_equal(w["mask"], dmask[rows[ptr[:-1] + best]])
        kfc = np.ascontiguousarray(np.stack([kf1["m_t"][:3, 3], kf2["m_t"][:3, 3]]))
        obs_kf = np.ascontiguousarray(np.tile([1, 0] if c["kf2_first"] else [0, 1], P).astype(np.int32))
        ref_kf = np.zeros(P, np.int32)
        lvl = np.ascontiguousarray(kf1["kp_octave"][w["kp1"]].astype(np.int32))
        scale = np.ascontiguousarray(c["rig"]["scale"], np.float64)
        pts = np.ascontiguousarray(w["pos"])
        on, omin, omax = np.zeros((P, 3)), np.zeros(P), np.zeros(P)
        ob.lib().oracle_update_normal_depth(ob._p(pts), P, ob._p(ptr), ob._p(obs_kf), ob._p(kfc), ob._p(ref_kf), ob._p(lvl),
                                            ob._p(scale), len(scale), ob._p(on), ob._p(omin), ob._p(omax))
        assert on.tobytes() == w["normal"].tobytes()
        assert omin.tobytes() == w["min_dist"].tobytes() and omax.tobytes() == w["max_dist"].tobytes()


def test_loop_case_shows_the_flag_hand_over():
    """A KF1 keypoint whose point is created with the first neighbour and which would otherwise have
    matched in the last: with the flags at entry it matches there, with the updated ones it does
    not."""
    lc = loop_case()
    _, _, m12_entry = np_loop(lc["rig"], lc["kf1"], lc["kf2s"], LOOP_SKIP, LOOP_KF2_FIRST, update_flags=False)
    created0 = dict(lc["points"])[0]["kp1"]
    taken = [i for i in created0 if m12_entry[2][i] >= 0]
    assert len(taken) > 5 and all(lc["matches12"][2][i] < 0 for i in taken)
    assert (lc["matches12"][1] < 0).all() and [t for t, _ in lc["points"]] == [0, 2]
    assert lc["kf1"]["has_mp"].sum() > 0.2 * len(lc["kf1"]["has_mp"])
    assert all(len(r["kp1"]) > 10 for _, r in lc["points"])


NEW_SYMBOLS = ["mcs_newpts_workspace_create", "mcs_newpts_workspace_destroy", "mcs_new_points_pair_device",
               "mcs_create_new_map_points_device", "mcs_create_new_map_points", "mcs_compute_e_rig_hom"]


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES, s
        assert hasattr(L, s), s


def test_struct_matches_the_header():
    import re
    import mcs_amd
    from mcs_amd import new_points
    txt = open(os.path.join(mcs_amd.INCLUDE_DIR, "mcs_newpoints.h")).read()
    body = re.search(r"typedef struct mcs_new_points \{(.*?)\} mcs_new_points;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        fields += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    assert fields == [f[0] for f in new_points.NewPoints._fields_]
    for k, v in (("NONE", 0), ("CREATED", 1), ("PARALLAX", 2), ("BEHIND1", 3), ("REPROJ1", 4), ("BEHIND2", 5),
                 ("REPROJ2", 6), ("DISTANCE", 7)):
        assert int(re.search(r"#define MCS_NP_%s (\d+)" % k, txt).group(1)) == v == getattr(new_points, k)


def test_compute_e_rig_from_matrices_equals_the_cayley_form(built):
    import mcs_amd
    from mcs_amd import synth
    rig, kf1, kf2s, _ = make_scene(5, n_per_cam=10)
    mc6 = np.ascontiguousarray(synth.LAFIDA_MC[:3], np.float64)
    a, b = np.zeros((3, 3, 9)), np.zeros((3, 3, 9))
    L = mcs_amd.lib()
    p = lambda x: np.ascontiguousarray(x, np.float64).ctypes.data  # noqa: E731
    m1, m2, mc = (np.ascontiguousarray(x, np.float64) for x in (kf1["m_t"], kf2s[0]["m_t"], rig["m_c"]))
    assert L.mcs_compute_e_rig(p(kf1["pose6"]), p(kf2s[0]["pose6"]), mc6.ctypes.data, 3, a.ctypes.data) == 0
    assert L.mcs_compute_e_rig_hom(m1.ctypes.data, m2.ctypes.data, mc.ctypes.data, 3, b.ctypes.data) == 0
    assert a.tobytes() == b.tobytes()
    assert L.mcs_compute_e_rig_hom(None, m2.ctypes.data, mc.ctypes.data, 3, b.ctypes.data) == mcs_amd.MCS_ERR_ARG


# ----------------------------------------------------------------------------- the C ABI without a GPU
def _host_call(rig=None, cap=None, device=0, **edit):
    """mcs_create_new_map_points on the c3x40 case with the packed set edited -> status."""
    import mcs_amd
    from mcs_amd import fuse, new_points as npz
    c = gpu_case("c3x40")
    rig = dict(c["rig"]) if rig is None else rig
    nb = c["kf1"]["desc"].shape[1]
    pk = fuse.pack_targets(rig, [c["kf1"], c["kf2"]], nb, False)
    masked_out = edit.pop("masked_out", pk["mask"] is not None)
    pk.update({k: v for k, v in edit.items() if k in pk})
    ks, keep = npz.host_set(pk)
    n1 = len(c["kf1"]["kp_xy"])
    cap = n1 if cap is None else cap
    o, arrs = npz.NewPoints(), {}
    o.cap = cap
    for k, (dt, shp) in npz.out_shapes(max(cap, 1), nb, masked_out).items():
        arrs[k] = np.zeros(shp, dt)
        setattr(o, k, arrs[k].ctypes.data)
    for k in edit.get("null_out", ()):
        setattr(o, k, None)
    E = np.zeros((1, 3, 3, 9))
    has = np.zeros(pk["n_kp_total"], np.uint8)
    one = np.zeros(1, np.uint8)
    return mcs_amd.lib().mcs_create_new_map_points(device, ctypes.byref(ks), one.ctypes.data, one.ctypes.data, E.ctypes.data,
                                                   None if edit.get("null_has") else has.ctypes.data, 64, EPI_THRESH,
                                                   None, None, ctypes.byref(o))


def test_host_entry_without_a_device(built):
    import mcs_amd
    if mcs_amd.device_count() > 0:
        pytest.skip("a device is visible")
    assert _host_call() == mcs_amd.MCS_ERR_NO_DEVICE


def _nine_cams():
    rig = make_rig(3)
    for k in ("m_c", "cam", "mirror", "grid_params"):
        rig[k] = np.concatenate([rig[k]] * 3)
    return rig


@pytest.mark.parametrize("kw", [dict(rig="nine"), dict(bytes=24), dict(bytes=0), dict(masked_out=True), dict(cap=-1),
                                dict(null_out=("count",)), dict(null_out=("pos",)), dict(null_has=True), dict(device=-1),
                                dict(off=np.array([0, 5, 3], np.int32)), dict(n_levels=0), dict(rays=None),
                                dict(kp_cam="bad")],
                         ids=lambda k: "_".join("%s" % (x,) for x in k))
def test_argument_errors_come_before_any_device_use(built, kw):
    import mcs_amd
    kw = dict(kw)
    if kw.get("rig") == "nine":
        kw["rig"] = _nine_cams()
    if isinstance(kw.get("kp_cam"), str):
        c = gpu_case("c3x40")
        cams = np.concatenate([c["kf1"]["kp_cam"], c["kf2"]["kp_cam"]]).astype(np.int32)
        cams[3] = 3
        kw["kp_cam"] = cams
    assert _host_call(**kw) == mcs_amd.MCS_ERR_ARG, mcs_amd.lib().mcs_last_error()
    assert len(mcs_amd.lib().mcs_last_error()) > 10


def test_device_entries_reject_bad_arguments_without_a_device(built):
    """i1 == i2, n1 above the workspace, a null workspace, a mask on one side only: the checks of the
    device entries run before anything touches a device (the workspace here is never created)."""
    import mcs_amd
    from mcs_amd import fuse, new_points as npz
    c = gpu_case("c3x40")
    nb = c["kf1"]["desc"].shape[1]
    pk = fuse.pack_targets(c["rig"], [c["kf1"], c["kf2"]], nb, False)
    ks, keep = npz.host_set(pk)
    o = npz.NewPoints()
    o.cap = 0
    cnt = np.zeros(1, np.int32)
    o.count = cnt.ctypes.data
    L = mcs_amd.lib()
    one = np.zeros(4, np.int32)
    # the pair entry: argument checks precede the workspace's use, so a null workspace is reported last
    for i1, i2 in ((0, 0), (0, 2), (-1, 1)):
        assert L.mcs_new_points_pair_device(None, ctypes.byref(ks), i1, i2, 4, 0, one.ctypes.data, 0, one.ctypes.data,
                                            one.ctypes.data, None, ctypes.byref(o), None) == mcs_amd.MCS_ERR_ARG
        assert b"two different keyframes" in L.mcs_last_error()
    assert L.mcs_new_points_pair_device(None, ctypes.byref(ks), 0, 1, 4, 0, one.ctypes.data, 0, one.ctypes.data,
                                        one.ctypes.data, None, ctypes.byref(o), None) == mcs_amd.MCS_ERR_ARG
    assert b"null workspace" in L.mcs_last_error()
    h = ctypes.c_void_p()
    assert L.mcs_newpts_workspace_create(0, 0, ctypes.byref(h)) == mcs_amd.MCS_ERR_ARG
    assert L.mcs_newpts_workspace_create(-1, 10, ctypes.byref(h)) == mcs_amd.MCS_ERR_ARG
    assert L.mcs_create_new_map_points_device(None, None, ctypes.byref(ks), None, None, None, None, None, 64, EPI_THRESH,
                                              None, None, ctypes.byref(o), None) == mcs_amd.MCS_ERR_ARG


def build_demo(tmp_path):
    import subprocess
    lib = os.path.join(ROOT, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "newpoints_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "newpoints_demo.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib, "-lmcs_amd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_demo_compiles_against_adapter_header(built, tmp_path):
    assert os.path.exists(build_demo(tmp_path))


def test_cpu_baseline_of_the_bench_tool_equals_the_restatement(tmp_path):
    """tests/cpp/newpoints_cpu.cpp (the bench tool's host loop) on one case: verdicts and points."""
    import subprocess
    so = str(tmp_path / "libnewpoints_cpu.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "newpoints_cpu.cpp"), "-o", so])
    from tools.bench_new_points import cpu_pair
    c = gpu_case("c3x120")
    got = cpu_pair(ctypes.CDLL(so), c["rig"], c["kf1"], c["kf2"], c["matches12"], c["kf2_first"], 0,
                   c["kf1"]["has_mp"].copy(), c["kf2"]["has_mp"].copy())
    w = c["want"]
    sure = ~w["unsure"]
    assert np.array_equal(got["verdict"][sure], w["verdict"][sure])
    assert np.array_equal(got["kp1"], w["kp1"]) and np.array_equal(got["kp2"], w["kp2"])
    assert got["pos"].tobytes() == w["pos"].tobytes() and got["normal"].tobytes() == w["normal"].tobytes()
    assert got["min_dist"].tobytes() == w["min_dist"].tobytes() and np.array_equal(got["desc"], w["desc"])


def test_fixture_regenerates_from_reference_text(tmp_path):
    ref = "/root/reference"
    if not os.path.isdir(ref):
        pytest.skip("no reference checkout on this machine")
    import subprocess
    import sys
    out = str(tmp_path / "again.npz")
    subprocess.check_call([sys.executable, os.path.join(os.path.dirname(FIX), "gen_newpoints_ref.py"), "--ref", ref,
                           "--out", out])
    a, b = np.load(FIX), np.load(out)
    assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a.files)
