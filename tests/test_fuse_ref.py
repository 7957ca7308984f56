"""cORBmatcher::Fuse (reference src/cORBmatcher.cpp:1265-1719), the parts that need no GPU:

  np_fuse_candidates  a plain NumPy / Python restatement of the device part of mcs_fuse_device:
                      per (target, query, camera) the projection (WorldToCamHom_fast), the
                      mirror mask, the distance window with rules 0 / 1 rounding dist3D to float,
                      the predicted level, cMultiKeyFrame::GetFeaturesInArea and the best
                      distance (rule 1 as written: bestDist stays 0), plus the E12 and
                      CheckDistEpipolarLine of rule 0;
  np_fuse_select      the state-dependent tails (:1379-1415, :1536-1563, :1692-1715) over a small
                      object model that keeps cMapPoint::mObservations and
                      cMultiKeyFrame::mvpMapPoints as the text does (Replace, AddObservation,
                      IsInKeyFrame, AddMapPoint, EraseMapPointMatch, ReplaceMapPointMatch,
                      GetMapPoints);
  mcs_fuse_select     the library's flat-array form of the same tail, through ctypes, against
                      np_fuse_select on scripted states and on random ones;
  fuse_ref.npz        what the reference TEXT does on seven scripted scenarios
                      (tests/golden/gen_fuse_ref.py): both restatements, the library's tail and
                      the whole multi-target sequence with its re-run are pinned to it, and the
                      fixture regenerates bit for bit where the reference checkout is present.

Every floating-point decision of the scripted inputs keeps a margin of 1e-9 (pixels or cells)
from its boundary: a projected pixel from a rounding half, a floor / ceil argument of the cell
range from an integer, |dx| - r and |dy| - r from zero.  The device's atan may differ from
libm's in the last ulp; with the margin no decision can flip, so all comparisons are exact.
The distance and level boundaries do not pass through atan and are exact without a margin.
"""
import math

import numpy as np
import pytest

MARGIN = 1e-9
INT_MAX = 2 ** 31 - 1
COLS, ROWS = 64, 48
W, H = 754, 480
ADD, REPLACE = 0, 1


# ----------------------------------------------------------------------------- the device part
def _matmul_lr(A, B):
    """cv::Matx product: s = 0; s += a(i,k) * b(k,j), k ascending."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((A.shape[0], B.shape[1]))
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            s = 0.0
            for k in range(A.shape[1]):
                s += float(A[i, k]) * float(B[k, j])
            out[i, j] = s
    return out


def _inv_mat(M):
    """cConverter::invMat (src/cConverter.cpp:31-44): R' = R^T, t' = -R' t."""
    O = np.eye(4)
    Rt = M[:3, :3].T.copy()
    O[:3, :3] = Rt
    O[:3, 3] = _matmul_lr(-Rt, M[:3, 3:4])[:, 0]
    return O


def _compute_e(Trel):
    """ComputeE(Trel) (include/misc.h:235-243)."""
    R = Trel[:3, :3]
    t = [float(x) for x in Trel[:3, 3]]
    s = 0.0
    for x in t:
        s += x * x
    ia = 1.0 / math.sqrt(s)
    t = [x * ia for x in t]
    S = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return _matmul_lr(S, R)


def _epi_check(r1, r2, E, thresh=1e-2):
    """CheckDistEpipolarLine (src/misc.cpp:54-70)."""
    r1, r2 = [float(x) for x in r1], [float(x) for x in r2]
    E = [[float(x) for x in row] for row in E]
    Ex1 = [E[r][0] * r1[0] + E[r][1] * r1[1] + E[r][2] * r1[2] for r in range(3)]
    Etx2 = [r2[0] * E[0][r] + r2[1] * E[1][r] + r2[2] * E[2][r] for r in range(3)]
    nom = Etx2[0] * r1[0] + Etx2[1] * r1[1] + Etx2[2] * r1[2]
    den = Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1] + Ex1[2] * Ex1[2] + Etx2[0] * Etx2[0] + \
        Etx2[1] * Etx2[1] + Etx2[2] * Etx2[2]
    if den == 0.0:
        return False
    return (nom * nom) / den < thresh


def _project(M, cam, X):
    """WorldToCamHom_fast (src/cam_system_omni.cpp:92-112) + WorldToImg (src/cam_model_omni.cpp
    :147-163), vectorised over X [n, 3]; every elementwise operation in the text's order."""
    R, t = M[:3, :3], M[:3, 3]
    Xc = []
    for i in range(3):
        ti = (-R[0, i]) * t[0] + (-R[1, i]) * t[1] + (-R[2, i]) * t[2]
        Xc.append(R[0, i] * X[:, 0] + R[1, i] * X[:, 1] + R[2, i] * X[:, 2] + ti * 1.0)
    x, y, z = Xc
    norm = np.sqrt(x * x + y * y)
    norm = np.where(norm == 0.0, 1e-14, norm)
    theta = np.arctan(-z / norm)
    rho = np.zeros_like(theta)
    for a in cam[5:17][::-1]:
        rho = rho * theta + a
    uu, vv = x / norm * rho, y / norm * rho
    return uu * cam[0] + vv * cam[1] + cam[3], uu * cam[2] + vv + cam[4]


def np_grid(kp_xy, kp_cam, gp):
    """The keyframe's feature grid: PosInGrid (src/cMultiFrame.cpp:342-353) per keypoint in index
    order -> dict (cam, ix, iy) -> [keypoint indices]."""
    cells = {}
    for i, (xy, c) in enumerate(zip(np.asarray(kp_xy, np.float32), kp_cam)):
        fx = np.float32(xy[0]) - np.float32(gp[c][0])
        fy = np.float32(xy[1]) - np.float32(gp[c][1])
        px = int(np.rint(np.float64(fx) * gp[c][2]))
        py = int(np.rint(np.float64(fy) * gp[c][3]))
        if px < 0 or px >= COLS or py < 0 or py >= ROWS:
            continue
        cells.setdefault((int(c), px, py), []).append(i)
    return cells


def _popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a, np.uint8)).sum())


def np_distance(d1, d2, m1=None, m2=None):
    """DescriptorDistance64 / DescriptorDistance64Masked (src/cORBmatcher.cpp:2443-2477)."""
    x = np.bitwise_xor(d1, d2)
    if m1 is None:
        return _popcount(x)
    return (_popcount(x & m1) + _popcount(x & m2)) // 2


def _int_margin(x):
    return abs(x - round(x))


def np_fuse_candidates(rule, rig, targets, q, th, th_low, flags=0, q_skip=None):
    """-> dict: best_kp, best_dist [T, nq, C] int32, epi_ok uint8 (rule 0, else None), and the
    intermediate values: u, v, level (-1 where the camera was left before the window), radius,
    area (dict (t, i, c) -> what GetFeaturesInArea returns), cand (the same after the level test, with
    distances),
    margin = the smallest distance of any atan-dependent decision from its boundary."""
    T, nq, C = len(targets), len(q["pos"]), len(rig["m_c"])
    scale = [float(s) for s in rig["scale"]]
    L = len(scale)
    gp = np.asarray(rig["grid_params"], np.float64)
    mirror = rig["mirror"]
    mh, mw = mirror.shape[1:]
    use_dist = rule != 1 or (flags & 1)
    masked = q.get("mask") is not None
    pos = np.asarray(q["pos"], np.float64).reshape(nq, 3)
    out = dict(best_kp=np.full((T, nq, C), -1, np.int32), best_dist=np.full((T, nq, C), INT_MAX, np.int32),
               epi_ok=np.zeros((T, nq, C), np.uint8) if rule == 0 else None,
               u=np.zeros((T, nq, C)), v=np.zeros((T, nq, C)), level=np.full((T, nq, C), -1, np.int32),
               radius=np.zeros((T, nq, C)), cand={}, area={}, margin=np.inf)
    margin = np.inf
    for t, tg in enumerate(targets):
        Mt = np.asarray(tg["m_t"], np.float64).reshape(4, 4)
        Ow = Mt[:3, 3]
        grid = np_grid(tg["kp_xy"], tg["kp_cam"], gp)
        kp_xy = np.asarray(tg["kp_xy"], np.float32).reshape(-1, 2).astype(np.float64)
        PO = pos - Ow
        dist3 = np.sqrt(PO[:, 0] * PO[:, 0] + PO[:, 1] * PO[:, 1] + PO[:, 2] * PO[:, 2])
        if rule != 2:
            dist3 = dist3.astype(np.float32).astype(np.float64)   # `const float dist3D`
        for c in range(C):
            M = _matmul_lr(Mt, np.asarray(rig["m_c"][c], np.float64).reshape(4, 4))
            us, vs = _project(M, np.asarray(rig["cam"][c], np.float64), pos)
            out["u"][t, :, c], out["v"][t, :, c] = us, vs
            E = None
            if rule == 0:
                T1 = _inv_mat(_matmul_lr(np.asarray(q["m_t"], np.float64).reshape(4, 4),
                                         np.asarray(rig["m_c"][c], np.float64).reshape(4, 4)))
                E = _compute_e(_matmul_lr(T1, M))
            for i in range(nq):
                if q_skip is not None and q_skip[t][i]:
                    continue
                u, v = float(us[i]), float(vs[i])
                assert math.isfinite(u) and math.isfinite(v)
                margin = min(margin, abs(abs(u - math.floor(u)) - 0.5), abs(abs(v - math.floor(v)) - 0.5))
                ur, vr = int(np.rint(u)), int(np.rint(v))
                if ur >= mw or ur <= 0 or vr >= mh or vr <= 0 or mirror[c][vr, ur] == 0:
                    continue
                max_d, min_d = 1.2 * float(q["dist"][i][1]), 0.8 * float(q["dist"][i][0])
                d = float(dist3[i])
                if d < min_d or d > max_d:
                    continue
                ratio = d / min_d
                lv = 0
                while lv < L and scale[lv] < ratio:
                    lv += 1
                lv = min(lv, L - 1)
                r = th * scale[lv]
                out["level"][t, i, c], out["radius"][t, i, c] = lv, r
                mnx, mny, wi, hi = (float(x) for x in gp[c])
                args = ((u - mnx - r) * wi, (u - mnx + r) * wi, (v - mny - r) * hi, (v - mny + r) * hi)
                margin = min(margin, min(_int_margin(a) for a in args))
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
                cand, best, bi = [], INT_MAX, -1
                area = out["area"].setdefault((t, i, c), [])
                for ix in range(x0, x1 + 1):
                    for iy in range(y0, y1 + 1):
                        for k in grid.get((c, ix, iy), ()):
                            dx, dy = abs(kp_xy[k, 0] - u), abs(kp_xy[k, 1] - v)
                            margin = min(margin, abs(dx - r), abs(dy - r))
                            if not (dx <= r and dy <= r):
                                continue
                            area.append(int(k))
                            lvl = int(tg["kp_octave"][k])
                            if lvl < lv - 1 or lvl > lv:
                                continue
                            dist = 0
                            if use_dist:
                                dist = np_distance(q["desc"][i], tg["desc"][k],
                                                   q["mask"][i] if masked else None,
                                                   tg["mask"][k] if masked else None)
                            cand.append((k, dist))
                            if dist < best:
                                best, bi = dist, k
                out["cand"][(t, i, c)] = cand
                if bi < 0:
                    continue
                out["best_dist"][t, i, c] = best
                if best <= th_low:
                    out["best_kp"][t, i, c] = bi
                    if rule == 0:
                        out["epi_ok"][t, i, c] = _epi_check(q["rays"][i], tg["rays"][bi], E)
    out["margin"] = margin
    return out


# ----------------------------------------------------------------------------- the tail
class _MP:
    def __init__(self, mid, bad):
        self.id, self.bad, self.obs = mid, bool(bad), {}

    def is_in_kf(self, kf):                       # cMapPoint::IsInKeyFrame (:447-451)
        return kf in self.obs

    def add_observation(self, kf, idx):           # :90-96
        self.obs.setdefault(kf, []).append(idx)

    def replace(self, other):                     # cMapPoint::Replace (:208-250)
        if other.id == self.id:
            return
        obs, self.obs, self.bad = self.obs, {}, True
        for kf, idxs in obs.items():
            for idx in idxs:
                if not other.is_in_kf(kf):
                    kf.slots[idx] = other          # ReplaceMapPointMatch
                    other.add_observation(kf, idx)
                else:
                    kf.slots[idx] = None           # EraseMapPointMatch


class _KF:
    def __init__(self, n):
        self.slots = [None] * n


def np_fuse_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp, get=None):
    """-> (actions [n, 4], n_fused, requery ids, mp_bad, mp_in_kf, kp_mp after the call).
    get: a list that receives (map point, keypoint) of every GetMapPoint(bestIdx) of the tail."""
    mps = [_MP(m, b) for m, b in enumerate(mp_bad)]
    kf = _KF(len(kp_mp))
    for k, m in enumerate(kp_mp):
        if m >= 0:
            kf.slots[k] = mps[m]
            if mp_in_kf[m]:
                mps[m].add_observation(kf, k)
    for m, f in enumerate(mp_in_kf):
        if f and kf not in mps[m].obs:
            mps[m].obs[kf] = []                   # in the keyframe's map without a slot
    found = {s for s in kf.slots if s is not None and not s.bad}      # GetMapPoints (:291-304)
    queries = {m for m in q_mp if m >= 0}
    actions, n_fused, requery = [], 0, []
    for i, m in enumerate(q_mp):
        if m < 0:
            continue
        mp = mps[m]
        if mp.bad or (mp in found if rule == 2 else mp.is_in_kf(kf)):
            continue
        best = [(c, int(k)) for c, k in enumerate(best_kp[i]) if k >= 0]
        for c, k in best:
            if get is not None:
                get.append((int(m), k))
            in_kf = kf.slots[k]
            if in_kf is not None:
                if not in_kf.bad and (rule != 0 or epi_ok[i][c]):
                    mp.replace(in_kf)
                    n_fused += 1
                    actions.append((REPLACE, i, k, in_kf.id))
                    if in_kf.id != mp.id and in_kf.id in queries and in_kf.id not in requery:
                        requery.append(in_kf.id)
            else:
                mp.add_observation(kf, k)
                kf.slots[k] = mp
                actions.append((ADD, i, k, mp.id))
    return (np.array(actions, np.int32).reshape(-1, 4), n_fused, np.array(requery, np.int32),
            np.array([p.bad for p in mps], np.uint8), np.array([p.is_in_kf(kf) for p in mps], np.uint8),
            np.array([-1 if s is None else s.id for s in kf.slots], np.int32))


def np_sim3_to_mt(Scw):
    """Rule 2's pose (:1576-1585): M_t = invMat(Rt2Hom(sRcw / s, tcw / s)), in the text's order."""
    Scw = np.asarray(Scw, np.float64).reshape(4, 4)
    dot = 0.0
    for j in range(3):
        dot += float(Scw[0, j]) * float(Scw[0, j])
    inv = 1.0 / math.sqrt(dot)
    M = np.eye(4)
    M[:3, :3] = Scw[:3, :3] * inv
    M[:3, 3] = Scw[:3, 3] * inv
    return _inv_mat(M)


def np_fuse_sequence(rule, rig, targets, q, q_mp, mp_bad, in_kf, kp_mp, new_desc, th, th_low, select=None, candidates=None):
    """The whole call over a map stand-in, as mcs::Fuse of host/mcs_multicol.hpp runs it: the
    device part for the remaining targets, the tail target by target, Replace replayed onto the
    other keyframes, and after a Replace whose survivor is a query that query's descriptor rows
    refreshed and the remaining targets run again.  in_kf / kp_mp: one array per target.
    -> (n_fused per target, actions [(t, kind, query, keypoint, other)], refreshed ids, mp_bad,
    kp_mp per target, per target the state right after its tail (kp_mp[t], mp_bad, in_kf[t]),
    per target what the device part gave for it: the candidates dict, its row index in it, the
    skip row at the target's entry and the GetMapPoint calls of its tail)."""
    T = len(targets)
    q = dict(q, desc=q["desc"].copy())
    mp_bad, in_kf, kp_mp = mp_bad.copy(), [a.copy() for a in in_kf], [a.copy() for a in kp_mp]
    n_fused, actions, refreshed, t0 = [0] * T, [], [], 0
    after, views = [None] * T, [None] * T
    while t0 < T:
        skip = np.zeros((T - t0, len(q_mp)), np.uint8)
        for t in range(t0, T):
            found = np.zeros(len(mp_bad), bool)
            slots = kp_mp[t][kp_mp[t] >= 0]
            found[slots[mp_bad[slots] == 0]] = True
            for i, m in enumerate(q_mp):
                skip[t - t0, i] = m < 0 or mp_bad[m] or (found[m] if rule == 2 else in_kf[t][m])
        cand = (candidates or np_fuse_candidates)(rule, rig, targets[t0:], q, th, th_low, q_skip=skip)
        assert cand["margin"] > MARGIN
        nxt = T
        for t in range(t0, T):
            ep = cand["epi_ok"][t - t0] if rule == 0 else None
            found = np.zeros(len(mp_bad), bool)
            slots = kp_mp[t][kp_mp[t] >= 0]
            found[slots[mp_bad[slots] == 0]] = True
            entry = np.array([m < 0 or mp_bad[m] or (found[m] if rule == 2 else in_kf[t][m]) for m in q_mp], bool)
            assert not (skip[t - t0].astype(bool) & ~entry).any()    # a snapshot never skips more than the entry state
            get = []
            np_fuse_select(rule, q_mp, cand["best_kp"][t - t0], ep, mp_bad, in_kf[t], kp_mp[t], get=get)
            views[t] = (cand, t - t0, entry, get)
            a, nf, req, mp_bad, in_kf[t], kp_mp[t] = (select or np_fuse_select)(rule, q_mp, cand["best_kp"][t - t0], ep,
                                                                    mp_bad, in_kf[t], kp_mp[t])
            n_fused[t] = nf
            after[t] = (kp_mp[t].copy(), mp_bad.copy(), in_kf[t].copy())
            for kind, i, k, other in a.tolist():
                actions.append((t, kind, i, k, other))
                src = int(q_mp[i])
                if kind != REPLACE or src == other:
                    continue
                for u in range(T):                   # Replace in the other keyframes
                    if u == t or not in_kf[u][src]:
                        continue
                    for s_ in np.flatnonzero(kp_mp[u] == src):
                        if not in_kf[u][other]:
                            kp_mp[u][s_], in_kf[u][other] = other, 1
                        else:
                            kp_mp[u][s_] = -1
                    in_kf[u][src] = 0
            if len(req) and t + 1 < T:
                for m in req:
                    q["desc"][np.flatnonzero(q_mp == m)] = new_desc[m]
                    refreshed.append(int(m))
                nxt = t + 1
                break
        t0 = nxt
    return n_fused, actions, refreshed, mp_bad, kp_mp, after, views


# ----------------------------------------------------------------------------- scripted inputs
def scale_factors(n=8):
    """mvScaleFactors as the cMultiFrame ctor builds them: s_i = s_{i-1} * (double)(float)1.2."""
    return np.cumprod([1.0] + [float(np.float32(1.2))] * (n - 1))


def make_rig(n_cams=3):
    from mcs_amd import ba, fuse, synth, window
    cams = synth.LAFIDA_CAMS[:n_cams]
    return dict(m_c=np.stack([fuse.cayley2hom(np.array(m)) for m in synth.LAFIDA_MC[:n_cams]]),
                cam=np.stack([ba.cam_vec(c) for c in cams]),
                mirror=np.stack([synth.mirror_mask(c) for c in cams]).astype(np.uint8),
                grid_params=window.grid_params([[0, 0]] * n_cams, [[W, H]] * n_cams),
                scale=scale_factors(), cams=cams)


def _flip(d, nbits, rng):
    d = d.copy()
    bits = rng.choice(d.size * 8, nbits, replace=False)
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def make_target(rig, rng, n_per_cam, nbytes, masked, pose=None, cluster=None, same_desc=False):
    """One keyframe: keypoints inside the mirror masks, camera by camera.  n_per_cam: int or a
    list per camera.  cluster: (cam, x, y) puts that camera's keypoints within one grid cell."""
    from mcs_amd import fuse, synth
    C = len(rig["m_c"])
    n_per_cam = [n_per_cam] * C if np.isscalar(n_per_cam) else list(n_per_cam)
    xy, cam, rays = [], [], []
    for c in range(C):
        n = n_per_cam[c]
        if cluster is not None and cluster[0] == c:
            p = np.array(cluster[1:], np.float64) + rng.uniform(-2.0, 2.0, (n, 2))
        else:
            ang, rad = rng.uniform(0, 2 * np.pi, n), 215.0 * np.sqrt(rng.uniform(0.02, 1.0, n))
            p = np.stack([rig["cams"][c]["u0"] + rad * np.cos(ang), rig["cams"][c]["v0"] + rad * np.sin(ang)], 1)
            p = p[(p[:, 0] > 2) & (p[:, 0] < W - 2) & (p[:, 1] > 2) & (p[:, 1] < H - 2)] if n else p.reshape(0, 2)
        p = p.astype(np.float32)
        xy.append(p)
        cam.append(np.full(len(p), c, np.int32))
        x, y, z = synth.img_to_world(rig["cams"][c], p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))
        rays.append(np.stack([x, y, z], 1).reshape(-1, 3))
    xy, cam, rays = np.concatenate(xy), np.concatenate(cam), np.concatenate(rays)
    n = len(xy)
    desc = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    if same_desc:
        desc[:] = desc[:1] if n else desc
    if pose is None:
        pose = np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.05, 0.05, 3)])
    return dict(kp_xy=xy, kp_octave=rng.integers(0, 8, n).astype(np.int32), kp_cam=cam, desc=desc,
                mask=rng.integers(0, 256, (n, nbytes), dtype=np.uint8) if masked else None, rays=rays,
                m_t=fuse.cayley2hom(pose))


def make_queries(rig, targets, rng, nq, nbytes, masked, jitter=3.0, same_desc=None):
    """Map points placed along rays of target keypoints (so that they project near them, in
    several targets and cameras), some far outside, with distance ranges that spread the
    predicted level over the pyramid and put some queries outside their range."""
    from mcs_amd import fuse
    scale = rig["scale"]
    pos, dist, desc = np.zeros((nq, 3)), np.zeros((nq, 2)), rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    have = [t for t in targets if len(t["kp_xy"])]
    cur = fuse.cayley2hom(np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.05, 0.05, 3)]))
    rays = rng.normal(size=(nq, 3))
    for i in range(nq):
        lvl = rng.integers(0, len(scale))
        if not have or rng.random() < 0.08:
            pos[i] = rng.uniform(-6, 6, 3)
        else:
            tg = have[rng.integers(len(have))]
            k = rng.integers(len(tg["kp_xy"]))
            M = tg["m_t"] @ rig["m_c"][tg["kp_cam"][k]]
            depth = rng.uniform(0.8, 6.0)
            pos[i] = M[:3, :3] @ (tg["rays"][k] * depth) + M[:3, 3] + rng.normal(0, jitter * depth / 300.0, 3)
            desc[i] = _flip(tg["desc"][k], int(rng.integers(0, nbytes * 3)), rng)
            if rng.random() < 0.7:    # the bearing of the point in curKF's camera: the epipolar test can hold
                Mc = cur @ rig["m_c"][tg["kp_cam"][k]]
                rays[i] = Mc[:3, :3].T @ (pos[i] - Mc[:3, 3])
            if rng.random() < 0.75:   # a level that lets this keypoint pass: its octave or one above
                lvl = min(int(tg["kp_octave"][k]) + int(rng.integers(0, 2)), len(scale) - 1)
        d = np.linalg.norm(pos[i] - (have[0]["m_t"][:3, 3] if have else 0.0))
        dmin = d / (0.8 * scale[lvl] * rng.uniform(0.86, 0.99))
        dist[i] = (dmin, dmin * rng.uniform(1.5, 12.0)) if rng.random() > 0.06 else (d * 2.0, d * 3.0)
    if same_desc is not None:
        desc[:] = same_desc
    q = dict(pos=pos, dist=dist, desc=desc, mask=rng.integers(0, 256, (nq, nbytes), dtype=np.uint8) if masked else None,
             rays=rays, m_t=cur)
    q["rays"] /= np.linalg.norm(q["rays"], axis=1, keepdims=True)
    return q


def make_case(seed, T=1, nq=64, n_per_cam=120, nbytes=32, masked=False, n_cams=3, **kw):
    rng = np.random.default_rng(seed)
    rig = make_rig(n_cams)
    tk = {k: kw[k] for k in ("cluster", "same_desc") if k in kw}
    targets = [make_target(rig, rng, n_per_cam, nbytes, masked, **tk) for _ in range(T)]
    same = targets[0]["desc"][0].copy() if kw.get("same_desc") else None
    if same is not None:      # one descriptor everywhere: every candidate is at distance 0
        for t in targets:
            t["desc"][:] = same
    q = make_queries(rig, targets, rng, nq, nbytes, masked, same_desc=same)
    return rig, targets, q


def th_low(nbytes, masked):
    """TH_LOW_ of the cORBmatcher ctor (src/cORBmatcher.cpp:46-65)."""
    return int(math.floor(nbytes)) if masked else 2 * nbytes


# ----------------------------------------------------------------------------- tests (no GPU)
NEW_SYMBOLS = ["mcs_fuse_workspace_create", "mcs_fuse_workspace_destroy", "mcs_fuse_device", "mcs_fuse",
               "mcs_fuse_select"]


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES, s
        assert hasattr(L, s), s


def test_structs_match_the_header():
    """Field order of the ctypes mirrors = the declaration order in include/mcs_matcher.h."""
    import os
    import re
    import mcs_amd
    from mcs_amd import fuse
    txt = open(os.path.join(mcs_amd.INCLUDE_DIR, "mcs_matcher.h")).read()
    for name, cls in (("mcs_fuse_targets", fuse.FuseTargets), ("mcs_fuse_queries", fuse.FuseQueries)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            names = re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
            fields += names
        assert fields == [f[0] for f in cls._fields_], name


def _check_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp):
    from mcs_amd import fuse
    want = np_fuse_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp)
    bad, inkf, slots = mp_bad.copy(), mp_in_kf.copy(), kp_mp.copy()
    actions, nf, req = fuse.fuse_select(rule, q_mp, best_kp, epi_ok, bad, inkf, slots)
    assert np.array_equal(actions, want[0]), (actions, want[0])
    assert nf == want[1]
    assert np.array_equal(req, want[2])
    assert np.array_equal(bad, want[3]) and np.array_equal(inkf, want[4]) and np.array_equal(slots, want[5])
    return actions, nf, req, bad, inkf, slots


def _state(n_mp, n_kp, slots, bad=()):
    """Consistent map state: slots {keypoint: map point}; a point in a slot observes the target
    unless it is bad (SetBadFlag / Replace clear the observations)."""
    mp_bad, mp_in_kf, kp_mp = np.zeros(n_mp, np.uint8), np.zeros(n_mp, np.uint8), np.full(n_kp, -1, np.int32)
    for b in bad:
        mp_bad[b] = 1
    for k, m in slots.items():
        kp_mp[k] = m
        if not mp_bad[m]:
            mp_in_kf[m] = 1
    return mp_bad, mp_in_kf, kp_mp


@pytest.mark.parametrize("rule", [0, 1, 2])
def test_select_scripted_cases(built, rule):
    """The branches of the tail, each on a hand-written state (3 cameras, 10 keypoints)."""
    ones = np.ones((8, 3), np.uint8)
    none = [-1, -1, -1]
    # an empty slot adds; a later query that hits the filled slot fuses into the first
    a, nf, req, bad, inkf, slots = _check_select(
        rule, np.array([0, 1]), np.array([[4, -1, -1], [4, -1, -1]]), ones, *_state(3, 10, {}))
    assert a.tolist() == [[ADD, 0, 4, 0], [REPLACE, 1, 4, 0]] and nf == 1 and req.tolist() == [0]
    assert bad.tolist() == [0, 1, 0] and slots[4] == 0
    # a query adds in camera 0 and fuses in camera 1: Replace erases the slot it gained, because
    # the survivor is already in the keyframe; camera 2 then adds the (now bad) query again
    a, nf, req, bad, inkf, slots = _check_select(
        rule, np.array([0]), np.array([[2, 5, 7]]), ones, *_state(3, 10, {5: 1}))
    assert a.tolist() == [[ADD, 0, 2, 0], [REPLACE, 0, 5, 1], [ADD, 0, 7, 0]] and nf == 1
    assert slots[2] == -1 and slots[5] == 1 and slots[7] == 0 and bad[0] == 1 and inkf[0] == 1
    # the same map point at two query positions: rules 0 / 1 skip the second (IsInKeyFrame),
    # rule 2 looks at the set taken before the loop and processes it again
    a, nf, *_ = _check_select(rule, np.array([0, 0]), np.array([[1, -1, -1], [-1, 3, -1]]), ones,
                              *_state(2, 10, {}))
    assert a.tolist() == ([[ADD, 0, 1, 0], [ADD, 1, 3, 0]] if rule == 2 else [[ADD, 0, 1, 0]])
    # an occupied slot whose point is bad: neither fused nor overwritten
    a, nf, *_ = _check_select(rule, np.array([0]), np.array([[6, -1, -1]]), ones, *_state(2, 10, {6: 1}, bad=[1]))
    assert a.tolist() == [] and nf == 0
    # rule 0: the epipolar test fails -> no fusion; rules 1 / 2 do not look at it
    zeros = np.zeros((8, 3), np.uint8)
    a, nf, *_ = _check_select(rule, np.array([0]), np.array([[6, -1, -1]]), zeros, *_state(2, 10, {6: 1}))
    assert (a.tolist(), nf) == (([], 0) if rule == 0 else ([[REPLACE, 0, 6, 1]], 1))
    # NULL, bad and in-keyframe queries are skipped; equal ids count as fused without an effect
    st = _state(4, 10, {0: 2, 9: 3}, bad=[1])
    st[1][3] = 0   # point 3 sits in slot 9 but does not observe the keyframe: not skipped by rules 0 / 1
    a, nf, req, bad, *_ = _check_select(rule, np.array([-1, 1, 2, 3]),
                                        np.array([none, [4, -1, -1], [5, -1, -1], [9, -1, -1]]), ones, *st)
    assert a.tolist() == ([] if rule == 2 else [[REPLACE, 3, 9, 3]]) and nf == (0 if rule == 2 else 1)
    assert bad[3] == 0 and req.tolist() == []


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("seed", range(6))
def test_select_random_states(built, rule, seed):
    """Random hits on random states: dense enough that chains (add, then fused into, then the
    survivor replaced in turn) occur."""
    rng = np.random.default_rng(100 * rule + seed)
    n_mp, n_kp, nq, C = 40, 30, 60, 3
    slots = {int(k): int(rng.integers(n_mp)) for k in rng.choice(n_kp, 12, replace=False)}
    mp_bad, mp_in_kf, kp_mp = _state(n_mp, n_kp, slots, bad=rng.choice(n_mp, 5, replace=False))
    q_mp = rng.integers(-1, n_mp, nq).astype(np.int32)
    best_kp = np.where(rng.random((nq, C)) < 0.5, rng.integers(0, n_kp, (nq, C)), -1).astype(np.int32)
    epi = (rng.random((nq, C)) < 0.7).astype(np.uint8)
    a, nf, *_ = _check_select(rule, q_mp, best_kp, epi, mp_bad, mp_in_kf, kp_mp)
    assert len(a) > 10 and nf > 0 and (a[:, 0] == ADD).any()


def test_select_rejects_bad_arguments(built):
    import mcs_amd
    from mcs_amd import fuse
    st = _state(2, 4, {})
    with pytest.raises(mcs_amd.McsError) as e:
        fuse.fuse_select(3, np.array([0]), np.array([[0, -1, -1]]), None, *st)
    assert e.value.code == mcs_amd.MCS_ERR_ARG
    with pytest.raises(mcs_amd.McsError):
        fuse.fuse_select(1, np.array([2]), np.array([[0, -1, -1]]), None, *st)      # id >= n_mp
    with pytest.raises(mcs_amd.McsError):
        fuse.fuse_select(1, np.array([0]), np.array([[4, -1, -1]]), None, *st)      # keypoint >= n_kp
    with pytest.raises(mcs_amd.McsError):
        fuse.fuse_select(0, np.array([0]), np.array([[0, -1, -1]]), None, *st)      # rule 0 needs epi_ok


CASES = [dict(seed=1, T=2, nq=120, nbytes=32), dict(seed=2, T=1, nq=90, nbytes=16, masked=True),
         dict(seed=3, T=1, nq=90, nbytes=64)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d%s" % (c["nbytes"], "m" if c.get("masked") else ""))
def test_restatement_covers_the_branches_with_margin(case):
    """np_fuse_candidates on the scripted inputs: every decision keeps the 1e-9 margin, and the
    inputs reach every exit of the per-camera body (mask, distance, empty window, level filter,
    above TH_LOW, hit) as well as the float / double distance difference between the rules."""
    rig, targets, q = make_case(**case)
    tl = th_low(case["nbytes"], case.get("masked", False))
    r = {rule: np_fuse_candidates(rule, rig, targets, q, 3.0, tl) for rule in (0, 1, 2)}
    for rule in (0, 1, 2):
        assert r[rule]["margin"] > MARGIN
        bk, bd, lv = r[rule]["best_kp"], r[rule]["best_dist"], r[rule]["level"]
        assert (bk >= 0).sum() > 20 and (lv < 0).sum() > 20
        assert ((lv >= 0) & (bd == INT_MAX)).any()              # window empty or all levels filtered
        assert len(np.unique(lv[lv >= 0])) >= 6
    assert ((r[0]["best_dist"] > tl) & (r[0]["best_dist"] < INT_MAX)).any()
    assert r[0]["epi_ok"].any() and (r[0]["epi_ok"][r[0]["best_kp"] >= 0] == 0).any()
    # rule 1 as written: distance 0 and the first level-passing candidate
    hit = r[1]["best_kp"] >= 0
    assert (r[1]["best_dist"][hit] == 0).all()
    for key, cand in r[1]["cand"].items():
        if cand:
            assert r[1]["best_kp"][key] == cand[0][0]
    assert (r[1]["best_kp"] != r[0]["best_kp"]).any()
    # with MCS_FUSE_USE_DISTANCE rule 1 selects as rule 0 does
    u = np_fuse_candidates(1, rig, targets, q, 3.0, tl, flags=1)
    assert np.array_equal(u["best_kp"], r[0]["best_kp"]) and np.array_equal(u["best_dist"], r[0]["best_dist"])


def test_float_distance_flips_a_bound_between_the_rules():
    """`const float dist3D` (:1306, :1464) against `const double` (:1623): a distance whose float
    rounding crosses the lower bound is inside for rule 2 and outside for rules 0 / 1, and the
    other way round; a distance exactly on a bound is inside for all.  No atan is involved."""
    rig, targets, q = make_case(seed=5, T=1, nq=40)
    base = np_fuse_candidates(2, rig, targets, q, 3.0, 64)
    i = int(np.argwhere((base["level"][0] >= 0).any(axis=1))[0, 0])
    PO =q["pos"][i] - targets[0]["m_t"][:3, 3]
    d = math.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
    df = float(np.float32(d))
    assert df != d
    lo, hi = (df, d) if df < d else (d, df)
    mid = lo + (hi - lo) / 2

    def levels(rule, dmin):
        q2 = dict(q, dist=q["dist"].copy())
        q2["dist"][i] = (dmin, 1e9)
        return np_fuse_candidates(rule, rig, targets, q2, 3.0, 64)["level"][0, i]

    # 0.8 * dmin == mid is not exactly reachable in general: search dmin with lo < 0.8 dmin <= hi
    dmin = mid / 0.8
    for _ in range(8):
        if lo < 0.8 * dmin <= hi:
            break
        dmin = np.nextafter(dmin, 0.0 if 0.8 * dmin > hi else np.inf)
    assert lo < 0.8 * dmin <= hi
    inside_double, inside_float = d >= 0.8 * dmin, df >= 0.8 * dmin
    assert inside_double != inside_float
    assert ((levels(2, dmin) >= 0).any()) == inside_double
    assert ((levels(0, dmin) >= 0).any()) == inside_float and ((levels(1, dmin) >= 0).any()) == inside_float
    # exactly on the lower bound (0.8 * dmin == d after rounding): inside, level 0
    dm = d / 0.8
    for cand in (dm, np.nextafter(dm, 0), np.nextafter(dm, np.inf)):
        if 0.8 * cand == d:
            lv = levels(2, cand)
            assert (lv >= 0).any() and lv.max() == 0
            break


def build_fuse_demo(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "fuse_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(root, "tests", "cpp", "fuse_demo.cpp"),
                           "-I", os.path.join(root, "include"), "-L", lib, "-lmcs_amd",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_demo_compiles_against_adapter_header(built, tmp_path):
    import os
    assert os.path.exists(build_fuse_demo(tmp_path))


def test_sim3_pose_with_scale():
    """Scw = s [R | t] with s != 1: the recovered M_t is the inverse of [R | t] to rounding, and
    its rotation rows are unit length (the scale is gone)."""
    from mcs_amd import fuse
    Tcw = fuse.cayley2hom(np.array([0.02, -0.01, 0.03, 0.4, -0.2, 0.1]))
    Scw = Tcw.copy()
    Scw[:3] *= 1.7
    Mt = np_sim3_to_mt(Scw)
    np.testing.assert_allclose(Mt @ Tcw, np.eye(4), atol=1e-14)
    np.testing.assert_allclose(np.linalg.norm(Mt[:3, :3], axis=1), 1.0, atol=1e-15)


# ----------------------------------------------------------------------------- the reference text
FIX = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden",
                                 "fuse_ref.npz")
SCENARIOS = ["r0", "r1", "r2", "r0m16", "r0b64", "e0", "e2"]
CRAFT = ("lower_exact", "lower_ulp_out", "upper_exact", "upper_ulp_out", "float_flip", "ratio_is_scale", "behind",
         "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "outside", "levels_and_tie")


def load_scenario(name):
    """One scenario of tests/golden/fuse_ref.npz (written by tests/golden/gen_fuse_ref.py from the
    reference text) -> dict with the inputs in the shapes of this module and the text's records."""
    z = np.load(FIX)
    p = name + "_"
    rule, T, nq, nbytes, masked, tl = (int(x) for x in z[p + "config"])
    rig = make_rig(3)
    if p + "grid_params" in z.files:
        rig["grid_params"] = z[p + "grid_params"]
    keys = ("kp_xy", "kp_octave", "kp_cam", "desc", "rays", "m_t") + (("mask",) if masked else ())
    targets = [dict({k: z[p + "t%d_%s" % (t, k)] for k in keys}, mask=z[p + "t%d_mask" % t] if masked else None)
               for t in range(T)]
    q = {k: z[p + "q_" + k] for k in ("pos", "dist", "desc", "rays", "m_t")}
    q["mask"] = z[p + "q_mask"] if masked else None
    return dict(rule=rule, T=T, nq=nq, nbytes=nbytes, masked=bool(masked), th_low=tl, th=float(z[p + "th"]), rig=rig,
                targets=targets, q=q, q_mp=z[p + "q_mp"], mp_bad=z[p + "mp_bad"], new_desc=z[p + "new_desc"],
                kp_mp=[z[p + "t%d_kp_mp" % t] for t in range(T)], in_kf=[z[p + "t%d_in_kf" % t] for t in range(T)],
                scw=[z[p + "t%d_scw" % t] for t in range(T)], n_fused=z[p + "n_fused"].tolist(),
                actions=[tuple(a) for a in z[p + "actions"].tolist()], get=z[p + "get"],
                gfa_key=z[p + "gfa_key"], gfa_xyr=z[p + "gfa_xyr"], gfa_ptr=z[p + "gfa_ptr"], gfa_list=z[p + "gfa_list"],
                end=[(z[p + "end%d_slots" % t], z[p + "end%d_bad" % t], z[p + "end%d_in_kf" % t]) for t in range(T)],
                margin=float(z[p + "margin"]))


def check_sequence_against_text(s, got):
    """got = np_fuse_sequence's result; equal to what the reference text did: nFused, the ordered
    AddObservation / Replace calls, and after every target its slots, the bad flags and the
    in-keyframe flags."""
    n_fused, actions, _, mp_bad, kp_mp, after, _ = got
    assert list(n_fused) == s["n_fused"]
    assert [(t, kind, int(s["q_mp"][i]), k, other) for t, kind, i, k, other in actions] == s["actions"]
    for t in range(s["T"]):
        slots, bad, in_kf = s["end"][t]
        assert np.array_equal(after[t][0], slots), t
        assert np.array_equal(after[t][1], bad), t
        assert np.array_equal(after[t][2], in_kf), t
    assert np.array_equal(mp_bad, s["end"][-1][1]) and np.array_equal(kp_mp[-1], s["end"][-1][0])


def test_fixture_margin_and_shape():
    z = np.load(FIX)
    assert z["scenarios"].tolist() == SCENARIOS and int(z["n_statements"]) > 250
    kinds = set()
    for name in SCENARIOS:
        s = load_scenario(name)
        assert s["margin"] > MARGIN
        assert len(s["gfa_key"]) > 50 and len(s["actions"]) > 15 and sum(s["n_fused"]) > 0
        kinds |= {a[1] for a in s["actions"]}
        assert s["th_low"] == th_low(s["nbytes"], s["masked"])
    assert kinds == {ADD, REPLACE}
    assert load_scenario("r2")["T"] == 3 and load_scenario("r0m16")["masked"]


def test_text_at_the_distance_and_level_boundaries():
    """Scenarios e0 (rule 0, `const float dist3D`) and e2 (rule 2, double) share keyframes and
    seven crafted queries.  What the TEXT did with them: a distance exactly on a bound is inside
    for the double rule, one ulp outside is outside for both, a lower bound between the
    float-rounded and the double distance separates the rules, a double dist3D / minDistance equal
    to scaleFactors[3] predicts level 3 (lower_bound; the float one level 3 or 4), a point behind the cameras opens no window.
    (That the restatement and the device agree with the text on all of them is what the window
    and sequence tests of these two scenarios check.)"""
    z = np.load(FIX)
    n = {}
    for name in ("e0", "e2"):
        s = load_scenario(name)
        assert [CRAFT[k] for _, k in z[name + "_crafted"]] == list(CRAFT)
        n[name] = {CRAFT[k]: (s["gfa_key"][:, 1] == s["q_mp"][i]).sum() for i, k in z[name + "_crafted"]}
        i = int(z[name + "_crafted"][CRAFT.index("ratio_is_scale")][0])
        r = s["gfa_xyr"][s["gfa_key"][:, 1] == s["q_mp"][i], 2]
        sc = s["rig"]["scale"]
        if name == "e2":       # the ratio is exactly scaleFactors[3]: lower_bound stops there
            assert len(r) and (r == s["th"] * sc[3]).all()
        else:                  # the float-rounded distance lands on either side of it
            assert len(r) and all(x in (s["th"] * sc[3], s["th"] * sc[4]) for x in r)
    assert n["e2"]["lower_exact"] >= 1 and n["e2"]["upper_exact"] >= 1
    s = load_scenario("e2")      # on the lower bound the ratio is 1: level 0, whose window admits octave 0 alone
    i = int(z["e2_crafted"][CRAFT.index("lower_exact")][0])
    assert (s["gfa_xyr"][s["gfa_key"][:, 1] == s["q_mp"][i], 2] == s["th"] * s["rig"]["scale"][0]).all()
    for name in ("e0", "e2"):
        assert n[name]["lower_ulp_out"] == 0 and n[name]["upper_ulp_out"] == 0 and n[name]["behind"] == 0
    assert (n["e0"]["float_flip"] == 0) != (n["e2"]["float_flip"] == 0)


@pytest.mark.parametrize("name", ["e0", "e2"])
def test_text_at_the_window_boundaries(name):
    """The crafted windows of e0 / e2, read from the text's records: a window clamped at each of
    the four grid edges (the floor / ceil argument lies outside [0, cols - 1] or [0, rows - 1]
    and the call still returned), a window fully outside the grid (the call returned nothing
    because nMaxCellX < 0), and a window holding keypoints at level - 2, level - 1, level and
    level + 1 where the two admissible ones have equal distance: the first in cell order wins
    although the inadmissible ones are at distance 0."""
    z = np.load(FIX)
    s = load_scenario(name)
    crafted = {CRAFT[k]: int(i) for i, k in z[name + "_crafted"]}
    gp = s["rig"]["grid_params"][0]

    def calls(kind):
        m = s["q_mp"][crafted[kind]]
        sel = (s["gfa_key"][:, 1] == m) & (s["gfa_key"][:, 2] == 0) & (s["gfa_key"][:, 0] == 0)
        return [(x, y, r, s["gfa_list"][lo:hi].tolist()) for (x, y, r), lo, hi in
                zip(s["gfa_xyr"][sel], s["gfa_ptr"][:-1][sel], s["gfa_ptr"][1:][sel])]
    (x, y, r, _), = calls("clamp_left")
    assert (x - gp[0] - r) * gp[2] < 0 and (x - gp[0] + r) * gp[2] > 0
    (x, y, r, _), = calls("clamp_right")
    assert (x - gp[0] + r) * gp[2] > COLS - 1 and (x - gp[0] - r) * gp[2] < COLS
    (x, y, r, _), = calls("clamp_top")
    assert (y - gp[1] - r) * gp[3] < 0 and (y - gp[1] + r) * gp[3] > 0
    (x, y, r, _), = calls("clamp_bottom")
    assert (y - gp[1] + r) * gp[3] > ROWS - 1 and (y - gp[1] - r) * gp[3] < ROWS
    (x, y, r, lst), = calls("outside")
    assert (x - gp[0] + r) * gp[2] < 0 and lst == []
    (x, y, r, lst), = calls("levels_and_tie")
    level = 3
    assert r == s["th"] * s["rig"]["scale"][level] and lst[:4] == [0, 1, 2, 3]
    tg, qd = s["targets"][0], s["q"]["desc"][crafted["levels_and_tie"]]
    assert tg["kp_octave"][:4].tolist() == [level - 2, level - 1, level, level + 1]
    dist = [np_distance(qd, tg["desc"][k]) for k in range(4)]
    assert dist[0] == 0 and dist[3] == 0 and dist[1] == dist[2] > 0
    assert all(np_distance(qd, tg["desc"][k]) > dist[1] for k in lst[4:])
    m = s["q_mp"][crafted["levels_and_tie"]]
    got = [int(k) for t, mm, k in s["get"] if mm == m and tg["kp_cam"][k] == 0]
    assert got == [1]


@pytest.mark.parametrize("name", SCENARIOS)
def test_restatement_reproduces_the_text_windows(name):
    """Every GetFeaturesInArea call of the text, for every target of the scenario: the
    restatement projects to the same pixel (1e-9), computes the same radius (exact) and lists the
    same keypoints; the (map point, camera) pairs the text leaves before the window are left by
    the restatement too; the GetMapPoint(bestIdx) calls of the tails are the restatement's, in
    order.  Later targets are taken at the map state the sequence has reached (skip conditions at
    the target's entry, refreshed descriptors)."""
    s = load_scenario(name)
    got = np_fuse_sequence(s["rule"], s["rig"], s["targets"], s["q"], s["q_mp"], s["mp_bad"], s["in_kf"], s["kp_mp"],
                           s["new_desc"], s["th"], s["th_low"])
    n_windows = 0
    for t in range(s["T"]):
        w, row, entry, get = got[6][t]
        sel = s["gfa_key"][:, 0] == t
        rows_of = {}
        for i, m in enumerate(s["q_mp"]):
            if not entry[i]:
                rows_of.setdefault(int(m), []).append(i)
        seen = set()
        for (_, m, c), (x, y, r), lo, hi in zip(s["gfa_key"][sel], s["gfa_xyr"][sel], s["gfa_ptr"][:-1][sel],
                                                s["gfa_ptr"][1:][sel]):
            assert int(m) in rows_of, (t, m)
            for i in rows_of[int(m)]:      # a point listed twice has the same position and range in both rows
                assert abs(w["u"][row, i, c] - x) < 1e-9 and abs(w["v"][row, i, c] - y) < 1e-9
                assert w["radius"][row, i, c] == r and w["level"][row, i, c] >= 0
                assert w["area"][(row, i, int(c))] == s["gfa_list"][lo:hi].tolist()
            seen.add((int(m), int(c)))
            n_windows += 1
        reached = {(int(s["q_mp"][i]), c) for i in range(s["nq"]) for c in range(3)
                   if not entry[i] and w["level"][row, i, c] >= 0}
        assert reached == seen, t
        g = s["get"][s["get"][:, 0] == t]
        assert [(int(m), int(k)) for _, m, k in g] == get, t
    assert n_windows == len(s["gfa_key"]) or s["rule"] == 2   # rule 2 opens a repeated point's windows twice
    assert n_windows >= len({tuple(k) for k in s["gfa_key"].tolist()})


@pytest.mark.parametrize("name", SCENARIOS)
def test_sequence_reproduces_the_text(built, name):
    """The whole call over all targets (device part restated, tails by np_fuse_select, Replace
    replayed onto the other keyframes, refreshed descriptors, re-run) gives the text's nFused,
    its ordered AddObservation / Replace calls and its end state."""
    s = load_scenario(name)
    got = np_fuse_sequence(s["rule"], s["rig"], s["targets"], s["q"], s["q_mp"], s["mp_bad"], s["in_kf"], s["kp_mp"],
                           s["new_desc"], s["th"], s["th_low"])
    check_sequence_against_text(s, got)
    if name == "r0":
        assert got[2], "the rule-0 sequence must hold a Replace survivor that is a later query (the re-run path)"


@pytest.mark.parametrize("name", SCENARIOS)
def test_library_select_reproduces_the_text(built, name):
    """The same sequence with mcs_fuse_select (through ctypes) as the tail."""
    from mcs_amd import fuse

    def lib_select(rule, q_mp, best_kp, epi_ok, mp_bad, mp_in_kf, kp_mp):
        bad, inkf, slots = mp_bad.copy(), mp_in_kf.copy(), kp_mp.copy()
        a, nf, req = fuse.fuse_select(rule, q_mp, best_kp, epi_ok, bad, inkf, slots)
        return a, nf, req, bad, inkf, slots
    s = load_scenario(name)
    got = np_fuse_sequence(s["rule"], s["rig"], s["targets"], s["q"], s["q_mp"], s["mp_bad"], s["in_kf"], s["kp_mp"],
                           s["new_desc"], s["th"], s["th_low"], select=lib_select)
    check_sequence_against_text(s, got)


@pytest.mark.skipif(not __import__("os").path.isdir("/root/reference"), reason="needs the reference checkout")
def test_fixture_regenerates_from_reference_text(tmp_path):
    import os
    import subprocess
    import sys
    out = str(tmp_path / "fuse_ref.npz")
    gen = os.path.join(os.path.dirname(FIX), "gen_fuse_ref.py")
    subprocess.check_call([sys.executable, gen, "--out", out], stdout=subprocess.DEVNULL)
    a, b = np.load(FIX), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
