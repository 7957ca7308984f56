"""Synthetic MultiCol BA problems and maps (re-exported by mcs_amd.ba).

Synthetic problems follow SURVEY.md §8(d): Lafida 3-camera rig (M_c from
MultiCamSys_Calibration.yaml), MultiKeyFrames along a smooth trajectory, points sampled on
camera rays, observations = WorldToImg of visible points, octave ~ per-level budget,
pixel noise sigma = 0.5*1.2^octave, a few outliers, perturbed initial poses / points.
"""
import numpy as np

from . import synth

HUBER_GLOBAL = float(np.sqrt(5.991))     # cOptimizer::BundleAdjustment thHuber (src/cOptimizer.cpp:161)


# ---------------------------------------------------------------------------
# numpy restatement of the projection (generator only)
# ---------------------------------------------------------------------------
def cay2rot(c):
    c = np.asarray(c, np.float64)
    c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2]
    s = 1 + c1 * c1 + c2 * c2 + c3 * c3
    R = np.stack([1 + c1 * c1 - c2 * c2 - c3 * c3, 2 * (c1 * c2 - c3), 2 * (c1 * c3 + c2),
                  2 * (c1 * c2 + c3), 1 - c1 * c1 + c2 * c2 - c3 * c3, 2 * (c2 * c3 - c1),
                  2 * (c1 * c3 - c2), 2 * (c2 * c3 + c1), 1 - c1 * c1 - c2 * c2 + c3 * c3], -1)
    return (R / s[..., None]).reshape(c.shape[:-1] + (3, 3))


def rot2cay(R):
    C = (R - np.eye(3)) @ np.linalg.inv(R + np.eye(3))
    return np.array([-C[1, 2], C[0, 2], -C[0, 1]])


def cam_vec(cam):
    return np.array([cam["c"], cam["d"], cam["e"], cam["u0"], cam["v0"]] + list(cam["pol"]))


def project(pose, mc, camv, X):
    """X_c = (M_t M_c)^-1 X, then WorldToImg; vectorised over X [...,3]."""
    Rt, Rc = cay2rot(pose[:3]), cay2rot(mc[:3])
    R = Rt @ Rc
    t = Rt @ mc[3:] + pose[3:]
    Xc = (X - t) @ R
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    rho = np.sqrt(x * x + y * y)
    rho = np.where(rho == 0, 1e-14, rho)
    th = np.arctan(-z / rho)
    r = np.zeros_like(th)
    for a in camv[5:][::-1]:
        r = r * th + a
    uu, vv = x / rho * r, y / rho * r
    return np.stack([uu * camv[0] + vv * camv[1] + camv[3], uu * camv[2] + vv + camv[4]], -1), Xc


def make_problem(n_local=10, n_fixed=3, n_points=3000, target_edges=20000, seed=0,
                 outlier_frac=0.02, noise_scale=0.5, pose_noise=(0.005, 0.02),
                 point_noise=0.05, cams=None, mcs=None, nfeatures=2000, huber_delta=1.345 * 2):
    """Config C-style LocalBA problem (10 local MKF + fixed observers, ~3k points, ~20k edges)."""
    rng = np.random.default_rng(seed)
    cams = cams or synth.LAFIDA_CAMS
    mcs = np.array(mcs or synth.LAFIDA_MC, np.float64)
    ncam = len(cams)
    camv = np.stack([cam_vec(c) for c in cams])
    masks = [synth.mirror_mask(c) for c in cams]
    nk = n_fixed + n_local
    # smooth trajectory: yaw sweep + forward motion
    gt_poses = np.zeros((nk, 6))
    for k in range(nk):
        yaw = 0.02 * k
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        gt_poses[k, :3] = rot2cay(R)
        gt_poses[k, 3:] = [0.12 * k, 0.02 * np.sin(k), 0.01 * k]
    # points on rays of random (kf, cam, pixel)
    pts = np.zeros((n_points, 3))
    i = 0
    while i < n_points:
        k = rng.integers(nk)
        c = rng.integers(ncam)
        u = rng.uniform(40, cams[c]["Iw"] - 40)
        v = rng.uniform(40, cams[c]["Ih"] - 40)
        if masks[c][int(v), int(u)] == 0:
            continue
        x, y, z = synth.img_to_world(cams[c], np.array(u), np.array(v))
        d = rng.uniform(1.5, 8.0)
        Rt, Rc = cay2rot(gt_poses[k, :3]), cay2rot(mcs[c, :3])
        R = Rt @ Rc
        t = Rt @ mcs[c, 3:] + gt_poses[k, 3:]
        pts[i] = R @ (np.array([float(x), float(y), float(z)]) * d) + t
        i += 1
    # visibility of every point in every (kf, cam)
    vis = []
    for k in range(nk):
        for c in range(ncam):
            uv, Xc = project(gt_poses[k], mcs[c], camv[c], pts)
            ok = np.isfinite(uv).all(-1)
            ui = np.round(uv[:, 0]).astype(int)
            vi = np.round(uv[:, 1]).astype(int)
            ok &= (ui > 30) & (vi > 30) & (ui < cams[c]["Iw"] - 30) & (vi < cams[c]["Ih"] - 30)
            idx = np.where(ok)[0]
            ok2 = np.zeros(n_points, bool)
            if len(idx):
                ok2[idx] = masks[c][vi[idx], ui[idx]] > 0
                # ray consistency: ImgToWorld(uv) must point along X_c
                rx, ry, rz = synth.img_to_world(cams[c], uv[idx, 0], uv[idx, 1])
                dirn = Xc[idx] / np.linalg.norm(Xc[idx], axis=1, keepdims=True)
                cosang = rx * dirn[:, 0] + ry * dirn[:, 1] + rz * dirn[:, 2]
                ok2[idx] &= cosang > 0.9999
            vis.append((k, c, ok2, uv))
    V = np.stack([v[2] for v in vis], 1)  # [n_points, nk*ncam]
    # subsample observations to hit the target edge count (keep >= 2 per point)
    nobs = V.sum(1)
    keep_p = np.minimum(1.0, target_edges / max(1, V.sum()))
    sel = V & (rng.random(V.shape) < keep_p)
    for p in range(n_points):
        if sel[p].sum() < 2 and V[p].sum() >= 2:
            cand = np.where(V[p])[0]
            sel[p, rng.choice(cand, 2, replace=False)] = True
    good = sel.sum(1) >= 2
    # octave distribution ~ per-level budget
    lev = np.array([434, 362, 302, 251, 209, 175, 145, 122], np.float64)
    lev /= lev.sum()
    e_pose, e_pt, e_cam, e_meas, e_info = [], [], [], [], []
    new_id = -np.ones(n_points, int)
    npts = 0
    for p in range(n_points):
        if not good[p]:
            continue
        new_id[p] = npts
        for j in np.where(sel[p])[0]:
            k, c = divmod(j, ncam)
            uv = vis[j][3][p]
            o = rng.choice(8, p=lev)
            sig = noise_scale * 1.2 ** o
            meas = uv + rng.normal(0, sig, 2)
            if rng.random() < outlier_frac:
                meas = np.array([rng.uniform(40, cams[c]["Iw"] - 40), rng.uniform(40, cams[c]["Ih"] - 40)])
            e_pose.append(k)
            e_pt.append(npts)
            e_cam.append(c)
            e_meas.append(meas)
            e_info.append(1.0 / (1.2 ** (2 * o)))
        npts += 1
    gt_pts = pts[good]
    poses0 = gt_poses.copy()
    pose_fixed = np.zeros(nk, np.uint8)
    pose_fixed[:n_fixed] = 1
    for k in range(n_fixed, nk):
        poses0[k, :3] += rng.normal(0, pose_noise[0], 3)
        poses0[k, 3:] += rng.normal(0, pose_noise[1], 3)
    pts0 = gt_pts + rng.normal(0, point_noise, gt_pts.shape)
    return dict(poses=poses0, pose_fixed=pose_fixed, points=pts0, mc=mcs, cam=camv,
                edge_pose=np.array(e_pose, np.int32), edge_point=np.array(e_pt, np.int32),
                edge_cam=np.array(e_cam, np.int32), edge_meas=np.array(e_meas, np.float64),
                edge_info=np.array(e_info, np.float64), huber_delta=huber_delta,
                gt_poses=gt_poses, gt_points=gt_pts)


def make_pose_problem(seed=0, n_points=1500, target_edges=5000, outlier_frac=0.05,
                      noise_scale=0.5, pose_noise=(0.01, 0.05), huber_multiplier=2.0):
    """PoseOptimization problem (src/cOptimizer.cpp:264-486): the current MultiFrame's pose
    (perturbed) and its 2D-3D correspondences to fixed map points (true positions), with
    information invSigma2(octave) and Huber delta 1.345 * huberMultiplier (:344)."""
    pr = make_problem(n_local=2, n_fixed=0, n_points=n_points, target_edges=target_edges,
                      seed=seed, outlier_frac=outlier_frac, noise_scale=noise_scale,
                      pose_noise=pose_noise, point_noise=0.0)
    sel = pr["edge_pose"] == 0
    used = np.unique(pr["edge_point"][sel])
    remap = -np.ones(len(pr["points"]), np.int64)
    remap[used] = np.arange(len(used))
    return dict(poses=pr["poses"][:1].copy(), pose_fixed=np.zeros(1, np.uint8),
                points=pr["gt_points"][used].copy(), mc=pr["mc"], cam=pr["cam"],
                edge_pose=np.zeros(int(sel.sum()), np.int32),
                edge_point=remap[pr["edge_point"][sel]].astype(np.int32),
                edge_cam=pr["edge_cam"][sel].copy(), edge_meas=pr["edge_meas"][sel].copy(),
                edge_info=pr["edge_info"][sel].copy(), huber_delta=1.345 * huber_multiplier,
                gt_pose=pr["gt_poses"][0].copy())


def make_map(n_kf=16, n_points=2500, target_edges=14000, seed=0, bad_kf=(), bad_points=0.01,
             zero_id_kf=None, unmatched_frac=0.1, covis_th=15):
    """Synthetic MultiKeyFrame map for LocalBundleAdjustment assembly: keyframes with mnId,
    isBad, map-point matches (with NULL entries), points with isBad and observations in
    keyframe order (the std::map iteration order of the reference with pointer order taken as
    keyframe order).  Geometry and observations from make_problem.  Returns the map dict;
    covisibles(m, k) gives GetVectorCovisibleKeyFrames (shared >= covis_th, weight order)."""
    rng = np.random.default_rng(seed + 17)
    pr = make_problem(n_local=n_kf, n_fixed=0, n_points=n_points, target_edges=target_edges,
                      seed=seed)
    nk, npt = len(pr["poses"]), len(pr["points"])
    ids = np.sort(rng.choice(np.arange(1, 10 * nk), nk, replace=False)).astype(np.int64)
    if zero_id_kf is not None:
        ids[zero_id_kf] = 0
    kf_bad = np.zeros(nk, np.uint8)
    kf_bad[list(bad_kf)] = 1
    pt_bad = (rng.random(npt) < bad_points).astype(np.uint8)
    order = np.lexsort((np.arange(len(pr["edge_pose"])), pr["edge_pose"], pr["edge_point"]))
    e_kf, e_pt = pr["edge_pose"][order], pr["edge_point"][order]
    obs_kf = e_kf.astype(np.int32)
    pt_obs_off = np.zeros(npt + 1, np.int32)
    np.add.at(pt_obs_off, e_pt + 1, 1)
    pt_obs_off = np.cumsum(pt_obs_off).astype(np.int32)
    # keyframe map-point matches: each observation is a keypoint of its keyframe, plus NULLs
    kf_lists = [[] for _ in range(nk)]
    for k, p in zip(e_kf, e_pt):
        kf_lists[k].append(int(p))
    kf_mp, kf_mp_off = [], [0]
    for k in range(nk):
        lst = kf_lists[k] + [-1] * int(unmatched_frac * len(kf_lists[k]))
        rng.shuffle(lst)
        kf_mp += lst
        kf_mp_off.append(len(kf_mp))
    return dict(kf_id=ids, kf_bad=kf_bad, kf_mp_off=np.array(kf_mp_off, np.int32),
                kf_mp=np.array(kf_mp, np.int32), pt_bad=pt_bad, pt_obs_off=pt_obs_off,
                obs_kf=obs_kf, obs_cam=pr["edge_cam"][order], obs_meas=pr["edge_meas"][order],
                obs_info=pr["edge_info"][order], kf_pose=pr["poses"], pt_pos=pr["points"],
                mc=pr["mc"], cam=pr["cam"], covis_th=covis_th)


def covisibles(m, k):
    """GetVectorCovisibleKeyFrames of keyframe k: keyframes sharing >= covis_th good map
    points, by decreasing weight (ties by index)."""
    nk = len(m["kf_id"])
    w = np.zeros(nk, np.int64)
    for p in range(len(m["pt_bad"])):
        if m["pt_bad"][p]:
            continue
        ks = set(m["obs_kf"][m["pt_obs_off"][p]:m["pt_obs_off"][p + 1]].tolist())
        if k in ks:
            for j in ks:
                if j != k:
                    w[j] += 1
    cand = [j for j in range(nk) if w[j] >= m["covis_th"]]
    return np.array(sorted(cand, key=lambda j: (-w[j], j)), np.int32)


def ring_rig(ncams=8, size=1024, radius=0.12, phase_deg=10.0):
    """Config D/E rig: `ncams` Lafida-polynomial fisheyes scaled to size x size, optical axes
    horizontal and evenly spread in yaw, mounted on a ring of the given radius."""
    cam = synth.scaled_cam(synth.LAFIDA_CAMS[0], size, size)
    cams, mcs = [], []
    for c in range(ncams):
        ph = np.deg2rad(phase_deg + 360.0 * c / ncams)
        ax = np.array([np.cos(ph), np.sin(ph), 0.0])
        xc = np.array([-np.sin(ph), np.cos(ph), 0.0])
        yc = np.array([0.0, 0.0, -1.0])
        R = np.stack([xc, yc, -ax], 1)           # columns: camera axes in the body frame
        mcs.append(np.concatenate([rot2cay(R), radius * ax]))
        cams.append(dict(cam))
    return cams, np.array(mcs)


def make_global_problem(n_kf=200, n_points=50000, target_edges=400000, ncams=8, size=1024,
                        seed=0, outlier_frac=0.02, noise_scale=0.5, pose_noise=(0.003, 0.01),
                        point_noise=0.05, step=0.15, max_range=8.0):
    """Config E: GlobalBA over n_kf MultiKeyFrames of an ncams ring rig, ~n_points points and
    ~target_edges observations (vectorised generator).  BundleAdjustment semantics:
    information = I (:209), Huber sqrt(5.991) (:161), keyframe 0 fixed (:119-120)."""
    rng = np.random.default_rng(seed)
    cams, mcs = ring_rig(ncams, size)
    camv = np.stack([cam_vec(c) for c in cams])
    cam = cams[0]
    mask = synth.mirror_mask(cam)
    # smooth planar trajectory (slow yaw drift), body z up
    k = np.arange(n_kf)
    yaw = 0.6 * np.sin(k / 40.0)
    gt_poses = np.zeros((n_kf, 6))
    pos = np.zeros(3)
    for i in range(n_kf):
        R = np.array([[np.cos(yaw[i]), -np.sin(yaw[i]), 0], [np.sin(yaw[i]), np.cos(yaw[i]), 0],
                      [0, 0, 1]])
        gt_poses[i, :3] = rot2cay(R)
        gt_poses[i, 3:] = pos
        pos = pos + step * np.array([np.cos(yaw[i]), np.sin(yaw[i]), 0.02 * np.sin(i / 7.0)])
    # points on rays of random (kf, cam, pixel inside the mirror mask)
    ys, xs = np.nonzero(mask[40:-40, 40:-40])
    pick = rng.integers(len(xs), size=n_points)
    u = xs[pick] + 40 + rng.uniform(0, 1, n_points)
    v = ys[pick] + 40 + rng.uniform(0, 1, n_points)
    rx, ry, rz = synth.img_to_world(cam, u, v)
    depth = rng.uniform(1.5, max_range, n_points)
    kk = rng.integers(n_kf, size=n_points)
    cc = rng.integers(ncams, size=n_points)
    Xc = np.stack([rx, ry, rz], 1) * depth[:, None]
    Rt = cay2rot(gt_poses[kk, :3])
    Rc = cay2rot(mcs[cc, :3])
    Rw = Rt @ Rc
    tw = np.einsum("nij,nj->ni", Rt, mcs[cc, 3:]) + gt_poses[kk, 3:]
    pts = np.einsum("nij,nj->ni", Rw, Xc) + tw
    # visibility of every point in every (kf, cam): in range, inside the mask, ray-consistent
    rows, cols, uvs = [], [], []
    for i in range(n_kf):
        near = np.nonzero(np.linalg.norm(pts - gt_poses[i, 3:], axis=1) < max_range)[0]
        if len(near) == 0:
            continue
        for c in range(ncams):
            uv, Xc_ = project(gt_poses[i], mcs[c], camv[c], pts[near])
            ok = np.isfinite(uv).all(-1)
            ui = np.round(np.nan_to_num(uv[:, 0], nan=-1e6)).astype(np.int64)
            vi = np.round(np.nan_to_num(uv[:, 1], nan=-1e6)).astype(np.int64)
            ok &= (ui > 30) & (vi > 30) & (ui < size - 30) & (vi < size - 30)
            idx = np.nonzero(ok)[0]
            if len(idx) == 0:
                continue
            ok2 = mask[vi[idx], ui[idx]] > 0
            rx, ry, rz = synth.img_to_world(cam, uv[idx, 0], uv[idx, 1])
            d = Xc_[idx] / np.linalg.norm(Xc_[idx], axis=1, keepdims=True)
            ok2 &= (rx * d[:, 0] + ry * d[:, 1] + rz * d[:, 2]) > 0.9999
            idx = idx[ok2]
            rows.append(near[idx])
            cols.append(np.full(len(idx), i * ncams + c))
            uvs.append(uv[idx])
    rows = np.concatenate(rows)
    cols = np.concatenate(cols)
    uvs = np.concatenate(uvs)
    # subsample observations towards the target (keep >= 2 per point when possible)
    order = np.argsort(rows, kind="stable")
    rows, cols, uvs = rows[order], cols[order], uvs[order]
    cnt_all = np.bincount(rows, minlength=n_points)
    forced = 2 * int((cnt_all >= 2).sum())
    keep = rng.random(len(rows)) < min(1.0, max(0, target_edges - forced) / max(1, len(rows) - forced))
    start = np.concatenate([[0], np.cumsum(cnt_all)[:-1]])
    for j in (0, 1):   # force the first two observations of points that have >= 2
        sel = cnt_all >= 2
        keep[start[sel] + j] = True
    rows, cols, uvs = rows[keep], cols[keep], uvs[keep]
    cnt = np.bincount(rows, minlength=n_points)
    good = cnt >= 2
    m = good[rows]
    rows, cols, uvs = rows[m], cols[m], uvs[m]
    new_id = -np.ones(n_points, np.int64)
    new_id[good] = np.arange(good.sum())
    ne = len(rows)
    lev = np.array([869, 724, 603, 503, 419, 349, 291, 242], np.float64)
    octv = rng.choice(8, size=ne, p=lev / lev.sum())
    meas = uvs + rng.normal(0, 1, (ne, 2)) * (noise_scale * 1.2 ** octv)[:, None]
    out = rng.random(ne) < outlier_frac
    meas[out] = rng.uniform(60, size - 60, (int(out.sum()), 2))
    poses0 = gt_poses.copy()
    pose_fixed = np.zeros(n_kf, np.uint8)
    pose_fixed[0] = 1
    poses0[1:, :3] += rng.normal(0, pose_noise[0], (n_kf - 1, 3))
    poses0[1:, 3:] += rng.normal(0, pose_noise[1], (n_kf - 1, 3))
    gt_pts = pts[good]
    pts0 = gt_pts + rng.normal(0, point_noise, gt_pts.shape)
    return dict(poses=poses0, pose_fixed=pose_fixed, points=pts0, mc=mcs, cam=camv,
                edge_pose=(cols // ncams).astype(np.int32), edge_point=new_id[rows].astype(np.int32),
                edge_cam=(cols % ncams).astype(np.int32), edge_meas=meas,
                edge_info=np.ones(ne), huber_delta=HUBER_GLOBAL, gt_poses=gt_poses,
                gt_points=gt_pts)


def global_map_from_problem(pr):
    """Config E as the map GlobalBundleAdjustment reads: keyframe i = pose i (mnId = i, so
    keyframe 0 is the fixed one), point j = point j (mnId = j), observations = the problem's
    edges in point order (each point's edges are in keyframe order, the std::map order)."""
    ep = np.asarray(pr["edge_point"])
    order = np.argsort(ep, kind="stable")
    npt, nk = len(pr["points"]), len(pr["poses"])
    off = np.zeros(npt + 1, np.int64)
    np.add.at(off, ep + 1, 1)
    return dict(kf_id=np.arange(nk, dtype=np.int64), kf_bad=np.zeros(nk, np.uint8),
                pt_id=np.arange(npt, dtype=np.int64), pt_bad=np.zeros(npt, np.uint8),
                pt_obs_off=np.cumsum(off).astype(np.int32),
                obs_kf=np.asarray(pr["edge_pose"])[order].astype(np.int32),
                obs_cam=np.asarray(pr["edge_cam"])[order], obs_meas=np.asarray(pr["edge_meas"])[order],
                kf_pose=pr["poses"], pt_pos=pr["points"], mc=pr["mc"], cam=pr["cam"])


def config_e_problem(n_kf=200, n_points=50000, target_edges=400000, seed=7, **kw):
    """Config E through the reference-side boundary: the generated map (make_global_problem as
    GlobalBundleAdjustment's keyframe / map-point lists) assembled by mcs_global_ba_select into
    the problem mcs_global_ba takes (src/cOptimizer.cpp:101-234).  Ground truth kept."""
    from . import ba   # the select is a library call; ba imports this module
    pr = make_global_problem(n_kf=n_kf, n_points=n_points, target_edges=target_edges, seed=seed, **kw)
    m = global_map_from_problem(pr)
    g = ba.global_ba_select(m)
    out = ba.problem_from_gba_graph(m, g)
    out["gt_poses"], out["gt_points"] = pr["gt_poses"], pr["gt_points"]
    return out


def shard_points(pr, world):
    """Contiguous point ranges with balanced edge counts -> list of (point_lo, point_hi)."""
    npts = len(pr["points"])
    cnt = np.bincount(pr["edge_point"], minlength=npts)
    cum = np.cumsum(cnt)
    tot = cum[-1] if npts else 0
    bounds = [0]
    for r in range(1, world):
        bounds.append(int(np.searchsorted(cum, tot * r / world, side="left")) + 1 if npts else 0)
    bounds.append(npts)
    bounds = np.maximum.accumulate(np.minimum(np.array(bounds), npts))
    return [(int(bounds[r]), int(bounds[r + 1])) for r in range(world)]


def shard_problem(pr, rank, world):
    """This rank's BA shard: the points [lo, hi) with ALL their edges (edge order kept),
    every pose (replicated).  Returns (sub_problem, (lo, hi), edge_ids)."""
    lo, hi = shard_points(pr, world)[rank]
    ep = np.asarray(pr["edge_point"])
    eids = np.nonzero((ep >= lo) & (ep < hi))[0]
    sub = dict(pr)
    sub["points"] = np.ascontiguousarray(pr["points"][lo:hi])
    for k in ("edge_pose", "edge_cam", "edge_meas", "edge_info"):
        sub[k] = np.ascontiguousarray(np.asarray(pr[k])[eids])
    sub["edge_point"] = np.ascontiguousarray(ep[eids] - lo, dtype=np.int32)
    return sub, (lo, hi), eids
