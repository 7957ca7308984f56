#!/usr/bin/env python3
"""Time the tracking matchers of one frame on the device form against the host-split form.

3 cameras x 2000 keypoints on the Lafida rig, 32-byte descriptors; per frame, as cTracking does:
SearchByProjection(Current, Last, th = 50) over 1500 tracked slots of the last frame (rule 1),
then SearchByProjection(F, MPs, th = 3) over 2000 local map points (rule 0) on the same
mvpMapPoints.  Everything a frame starts from is resident on the device: the keypoints, the
descriptors, the last frame's points and the isInFrustum outputs.

  (a) device form: mcs_frame_grid_build_device, mcs_track_queries_lastframe_device /
      _mappoints_device, mcs_track_search_device twice; one synchronisation at the end.
  (b) host-split form, the same work as the parent of this change does it: keypoint download,
      mcs_frame_grid_build and grid upload, host-made queries (rule 0 in numpy from the downloaded
      isInFrustum outputs; rule 1's projections are taken as given, which favours (b)), and per
      rule mcs_window_search_device, the candidate download and mcs_window_select.

Both variants run through the Python bindings, in alternating windows after a warm-up; their
matches must agree (the tool fails otherwise).  Reported: wall time per frame of both, device
time per frame of (a) from events around each window, the device time of the selection step
alone (mcs_track_select_device, events around single calls) and the settle rounds.  Prints one
JSON line; --out also writes it.

    python tools/bench_track_match.py [--windows 6] [--frames 10] [--warmup 3] [--out profiles/track_match_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multicol-slam-annotation_amd"))

W, H, C, KP, NMP, NLAST = 754, 480, 3, 2000, 2000, 1500
TH_HIGH, RATIO0, RATIO1 = 96, 0.8, 0.9


def make_scene(seed=2026):
    from mcs_amd import window as mw
    from tests import test_frame as tf
    from tests.test_window import LEVEL_P, _flip
    rng = np.random.default_rng(seed)
    pose, mc, cam, masks, pts, _, _, scale = tf._frustum_inputs(3, n=C * KP)
    n = C * KP
    s = dict(pose=pose, mc=np.ascontiguousarray(mc), cam=np.ascontiguousarray(cam), masks=masks, scale=scale,
             gp=mw.grid_params([(0, 0)] * C, [(W, H)] * C))
    s["xy"] = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)
    s["kp_cam"] = np.repeat(np.arange(C, dtype=np.int32), KP)
    s["oct"] = rng.choice(8, n, p=LEVEL_P / LEVEL_P.sum()).astype(np.int32)
    s["desc"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    # the last frame: 1500 of its slots hold a point (plant_last_frame gives most of them a
    # look-alike in the current frame, once their projections are known)
    s["last_pos"] = np.ascontiguousarray(pts)
    s["last_cam"] = np.zeros(n, np.int32)          # main() picks a camera that sees the point
    s["last_oct"] = rng.choice(8, n, p=LEVEL_P / LEVEL_P.sum()).astype(np.int32)
    s["last_desc"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s["last_valid"] = np.zeros(n, np.uint8)        # and the 1500 tracked slots among the seen ones
    # the local map: isInFrustum outputs of 2000 points, about 40 % of (point, camera) in view
    s["iv"] = (rng.random((NMP, C)) < 0.4).astype(np.uint8)
    s["pj"] = np.stack([rng.uniform(20, W - 20, (NMP, C)), rng.uniform(20, H - 20, (NMP, C))], -1)
    s["lv"] = rng.choice(8, (NMP, C), p=LEVEL_P / LEVEL_P.sum()).astype(np.int32)
    s["vc"] = rng.uniform(0.9, 1.0, (NMP, C))
    s["mp_desc"] = rng.integers(0, 256, (NMP, 32), dtype=np.uint8)
    s["planted"] = np.zeros(n, bool)
    for p in range(NMP):                       # a keypoint that looks like the point, in the first camera seeing it
        cams = np.nonzero(s["iv"][p])[0]
        if len(cams) and rng.random() < 0.7:
            c = int(cams[0])
            k = c * KP + int(rng.integers(KP))
            s["xy"][k] = (s["pj"][p, c] + rng.normal(0, 2.0, 2)).astype(np.float32)
            s["oct"][k] = max(0, s["lv"][p, c] - int(rng.integers(0, 2)))
            s["desc"][k] = _flip(s["mp_desc"][p], int(rng.integers(0, 40)), rng)
            s["planted"][k] = True
    return s


def plant_last_frame(s, q_xyr, q_cl, seed=2027):
    """TrackWithMotionModel's scene: 80 % of the last frame's slots that project into their camera
    get a keypoint of the current frame near the projection, at the slot's octave, with the slot's
    descriptor up to 40 flipped bits.  Returns how many were planted."""
    from tests.test_window import _flip
    rng = np.random.default_rng(seed)
    count = 0
    for i in np.nonzero(q_cl[:, 0] >= 0)[0]:
        if rng.random() >= 0.8:
            continue
        k = int(q_cl[i, 0]) * KP + int(rng.integers(KP))
        if s["planted"][k]:
            continue
        s["xy"][k] = (q_xyr[i, :2] + rng.normal(0, 3.0, 2)).astype(np.float32)
        s["oct"][k] = s["last_oct"][i]
        s["desc"][k] = _flip(s["last_desc"][i], int(rng.integers(0, 40)), rng)
        s["planted"][k] = True
        count += 1
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from mcs_amd import track_match as tm
    from mcs_amd import window as mw
    s = make_scene()
    n = C * KP
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    # where the last frame's points project now (they do not depend on the current keypoints):
    # every tracked slot gets a camera whose mirror mask its point falls into
    def project(valid, cam):
        q = tm.queries_lastframe(T(s["pose"]), T(s["mc"]), T(s["cam"]), T(s["masks"]), T(s["last_pos"]), T(valid),
                                 T(cam), T(s["last_oct"]), T(s["scale"]), 50.0)
        torch.cuda.synchronize()
        return q[0].cpu().numpy(), q[1].cpu().numpy()
    seen = np.stack([project(np.ones(n, np.uint8), np.full(n, c, np.int32))[1][:, 0] >= 0 for c in range(C)], 1)
    s["last_cam"] = np.argmax(seen, axis=1).astype(np.int32)
    s["last_valid"] = np.zeros(n, np.uint8)
    s["last_valid"][np.random.default_rng(2028).choice(np.nonzero(seen.any(axis=1))[0], NLAST, replace=False)] = 1
    q = project(s["last_valid"], s["last_cam"])
    planted = plant_last_frame(s, q[0], q[1])
    d = {k: T(v) for k, v in s.items() if k != "planted"}
    ws = tm.Workspace(n, max(n, NMP * C), 1 << 22)
    a0 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_as = torch.zeros_like(a0)

    def frame_a(keep=None):
        d_as.copy_(a0)
        ptr, cells, _ = ws.grid_build(d["xy"], d["kp_cam"], d["gp"])
        fr = tm.DeviceFrame(d["gp"], d["xy"], d["oct"], d["desc"], ptr, cells)
        q1 = tm.queries_lastframe(d["pose"], d["mc"], d["cam"], d["masks"], d["last_pos"], d["last_valid"],
                                  d["last_cam"], d["last_oct"], d["scale"], 50.0)
        r1 = ws.search(1, fr, q1[0], q1[1], d["last_desc"], TH_HIGH, RATIO1, d_as, q_desc_idx=q1[2])
        q0 = tm.queries_mappoints(d["iv"], d["pj"], d["lv"], d["vc"], d["scale"], 3.0)
        r0 = ws.search(0, fr, q0[0], q0[1], d["mp_desc"], TH_HIGH, RATIO0, d_as, q_desc_idx=q0[2])
        if keep is not None:
            keep.update(fr=fr, q1=q1, q0=q0, r1=r1, r0=r0)
        return r1, r0

    # rule 1's host queries of (b): given (the parent's caller projects on the host; not timed here)
    keep = {}
    frame_a(keep)
    torch.cuda.synchronize()
    h_q1 = [t.cpu().numpy() for t in keep["q1"]]
    h_q1d = s["last_desc"]

    def frame_b():
        xy, cam = d["xy"].cpu().numpy(), d["kp_cam"].cpu().numpy()            # keypoint download
        frame = mw.FrameGrid(xy, cam, s["oct"], s["desc"], s["gp"])           # host grid, upload
        assigned = np.zeros(n, np.uint8)
        m1, n1, assigned = mw.window_match(1, frame, h_q1[0], h_q1[1], h_q1d, TH_HIGH, RATIO1, kp_assigned=assigned)
        iv, pj, lv, vc = (d[k].cpu().numpy() for k in ("iv", "pj", "lv", "vc"))
        r = np.where(vc > 0.998, 2.5, 4.0) * 3.0 * s["scale"][lv]
        xyr = np.concatenate([pj, r[..., None]], -1).reshape(-1, 3)
        cl = np.stack([np.where(iv == 1, np.arange(C), -1), lv - 1, lv], -1).astype(np.int32).reshape(-1, 3)
        qd = np.repeat(s["mp_desc"], C, axis=0)
        m0, n0, assigned = mw.window_match(0, frame, xyr, cl, qd, TH_HIGH, RATIO0, kp_assigned=assigned)
        return (m1, n1), (m0, n0)

    (m1, n1), (m0, n0) = frame_b()
    for got, want, cnt in ((keep["r1"], m1, n1), (keep["r0"], m0, n0)):
        if int(got[2].cpu()[0]) != cnt or not np.array_equal(got[0].cpu().numpy(), want):
            raise SystemExit("the device form and the host-split form disagree")
    st1, st0 = keep["r1"][3].cpu().numpy(), keep["r0"][3].cpu().numpy()

    for _ in range(a.warmup):
        frame_a()
        frame_b()
    torch.cuda.synchronize()
    wall_a, wall_b, dev_a = [], [], []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        for _ in range(a.frames):
            frame_a()
        e1.record()
        torch.cuda.synchronize()
        wall_a.append((time.perf_counter() - t) * 1e3 / a.frames)
        dev_a.append(e0.elapsed_time(e1) / a.frames)
        t = time.perf_counter()
        for _ in range(a.frames):
            frame_b()
        wall_b.append((time.perf_counter() - t) * 1e3 / a.frames)

    def select_ms(rule, q, out, ratio, start):
        ms = []
        for _ in range(20):
            d_as.copy_(start)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ws.select(rule, keep["fr"], q[1], TH_HIGH, ratio, d_as, out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    # the workspace holds rule 0's lists (the last search); rule 1's after one more search
    after1 = torch.zeros_like(a0)
    after1[keep["r1"][0][keep["r1"][0] >= 0].long()] = 1
    sel0 = select_ms(0, keep["q0"], keep["r0"], RATIO0, after1)
    d_as.copy_(a0)
    r1 = ws.search(1, keep["fr"], keep["q1"][0], keep["q1"][1], d["last_desc"], TH_HIGH, RATIO1, d_as,
                   q_desc_idx=keep["q1"][2])
    sel1 = select_ms(1, keep["q1"], r1, RATIO1, a0)
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {"metric": "track_match_ms_per_frame", "cameras": C, "keypoints": n, "bytes": 32,
           "rule1_slots_tracked": NLAST, "rule1_th": 50.0, "rule0_points": NMP, "rule0_th": 3.0,
           "windows": a.windows, "frames_per_window": a.frames, "warmup": a.warmup,
           "rule1": {"queries": n, "live_queries": int((h_q1[1][:, 0] >= 0).sum()), "look_alikes_planted": planted,
                     "candidates": int(st1[0]), "matches": int(n1), "settle_rounds": tm.rounds(st1[1]),
                     "select_device_ms_median": sel1[0], "select_device_ms_min": sel1[1]},
           "rule0": {"queries": NMP * C, "candidates": int(st0[0]), "matches": int(n0), "settle_rounds": tm.rounds(st0[1]),
                     "select_device_ms_median": sel0[0], "select_device_ms_min": sel0[1]},
           "device_form": {"wall_ms_per_frame_median": med(wall_a), "wall_ms_per_frame_min": float(np.min(wall_a)),
                           "device_ms_per_frame_median": med(dev_a), "device_ms_per_frame_min": float(np.min(dev_a))},
           "host_split_form": {"wall_ms_per_frame_median": med(wall_b), "wall_ms_per_frame_min": float(np.min(wall_b)),
                               "rule1_host_projection_included": False}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
