#!/usr/bin/env python3
"""Time CreateNewMapPoints' neighbour loop at the config-B shape, on the device and as a caller had
to run it before the device entry existed.

3 cameras x 2000 keypoints per keyframe on the Lafida rig, 5 neighbours, 32-byte descriptors, about
30 % of the keypoints tracked already (tests/test_newpoints_ref.make_scene).  In one run, after a
warm-up, the median and minimum of --iters >= 20 of
  (a) mcs_create_new_map_points_device for the whole keyframe: events on the stream around the call
      (inputs resident, the flags restored by a device copy outside the events);
  (b) per neighbour: mcs_search_for_triangulation_raw_device, download of the match list, the
      per-match loop as plain single-thread -O3 C++ (tests/cpp/newpoints_cpu.cpp), upload of both
      flag arrays: wall time around the five rounds;
  and the five matcher calls of (a) alone (events), so that (a) minus the matcher is the cost of
  the new kernels.
The tool fails unless both paths produce the same points.  Prints one JSON line; --out also writes
it.

    python tools/bench_new_points.py [--iters 30] [--warmup 5] [--out profiles/new_points_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multicol-slam-annotation_amd"))

EPI = 1e-2


def build_cpu(tmp):
    so = os.path.join(tmp, "libnewpoints_cpu.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "newpoints_cpu.cpp"), "-o", so])
    return ctypes.CDLL(so)


def cpu_pair(L, rig, kf1, kf2, matches12, kf2_first, neighbour, has1, has2, out=None):
    """newpoints_cpu_pair on one neighbour; has1 / has2 (uint8, contiguous) are updated in place.
    out: the dict of an earlier call to append to -> dict with verdict and the points so far."""
    c = lambda a, dt: np.ascontiguousarray(a, dt)  # noqa: E731
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    n1, n2, nb = len(kf1["kp_xy"]), len(kf2["kp_xy"]), kf1["desc"].shape[1]
    masked = kf1.get("mask") is not None
    if out is None:
        cap = max(n1 * 8, 1)
        out = dict(count=np.zeros(1, np.int32), kp1=np.zeros(cap, np.int32), kp2=np.zeros(cap, np.int32),
                   neighbour=np.zeros(cap, np.int32), pos=np.zeros((cap, 3)), normal=np.zeros((cap, 3)),
                   min_dist=np.zeros(cap), max_dist=np.zeros(cap), desc=np.zeros((cap, nb), np.uint8),
                   mask=np.zeros((cap, nb), np.uint8) if masked else None, cap=cap)
    a = [c(rig["m_c"], np.float64), c(rig["cam"], np.float64), c(rig["scale"], np.float64),
         c(kf1["kp_xy"], np.float32), c(kf1["kp_octave"], np.int32), c(kf1["kp_cam"], np.int32), c(kf1["desc"], np.uint8),
         c(kf1["mask"], np.uint8) if masked else None, c(kf1["rays"], np.float64), c(kf1["m_t"], np.float64),
         c(kf2["kp_xy"], np.float32), c(kf2["kp_cam"], np.int32), c(kf2["desc"], np.uint8),
         c(kf2["mask"], np.uint8) if masked else None, c(kf2["rays"], np.float64), c(kf2["m_t"], np.float64),
         c(matches12, np.int32)]
    verdict = np.zeros(n1, np.uint8)
    V = ctypes.c_void_p
    L.newpoints_cpu_pair.argtypes = [ctypes.c_int] * 3 + [V] * 3 + [ctypes.c_int] + [V] * 7 + [ctypes.c_int] + [V] * 6 + \
        [V, ctypes.c_int, ctypes.c_int, V, V, V, ctypes.c_int] + [V] * 10
    rc = L.newpoints_cpu_pair(len(rig["m_c"]), nb, len(rig["scale"]), p(a[0]), p(a[1]), p(a[2]), n1, p(a[3]), p(a[4]), p(a[5]),
                              p(a[6]), p(a[7]), p(a[8]), p(a[9]), n2, p(a[10]), p(a[11]), p(a[12]), p(a[13]), p(a[14]),
                              p(a[15]), p(a[16]), int(kf2_first), int(neighbour), p(has1), p(has2), p(verdict), out["cap"],
                              p(out["count"]), p(out["kp1"]), p(out["kp2"]), p(out["neighbour"]), p(out["pos"]),
                              p(out["normal"]), p(out["min_dist"]), p(out["max_dist"]), p(out["desc"]), p(out["mask"]))
    if rc:
        raise SystemExit("newpoints_cpu_pair failed")
    n = int(out["count"][0])
    res = {k: (v[:n] if isinstance(v, np.ndarray) and k != "count" else v) for k, v in out.items()}
    res["verdict"], res["_bufs"] = verdict, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-cam", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20 (median of at least 20)")
    import torch
    import mcs_amd
    from mcs_amd import fuse, new_points as npz
    from tests.test_newpoints_ref import TOL_X, make_scene
    T, nb = 5, 32
    rig, kf1, kf2s, _ = make_scene(2026, n_per_cam=a.per_cam, nbytes=nb, neighbours=("normal",) * T, tracked=0.3)
    kfs = [kf1] + kf2s
    n_kp = [len(k["kp_xy"]) for k in kfs]
    n1 = n_kp[0]
    off = np.concatenate([[0], np.cumsum(n_kp)])
    pk = fuse.pack_targets(rig, kfs, nb, False)
    ks, keep = npz.device_set(pk)
    mc = np.ascontiguousarray(rig["m_c"], np.float64)
    E = np.zeros((T, 3, 3, 9))
    L = mcs_amd.lib()
    for t in range(T):
        m1, m2 = (np.ascontiguousarray(k["m_t"], np.float64) for k in (kf1, kf2s[t]))
        assert L.mcs_compute_e_rig_hom(m1.ctypes.data, m2.ctypes.data, mc.ctypes.data, 3, E[t].ctypes.data) == 0
    dE = torch.from_numpy(E).cuda()
    has0 = torch.from_numpy(np.concatenate([k["has_mp"] for k in kfs])).cuda()
    has = has0.clone()
    skip, first = np.zeros(T, np.uint8), np.array([t % 2 for t in range(T)], np.uint8)
    ws, tri = npz.Workspace(n1), npz.TriWorkspace(n1, max(n_kp[1:]))
    cap = n1 * T
    out, ot = npz.new_out(cap, nb, False)
    m12 = torch.empty((T, n1), dtype=torch.int32, device="cuda")
    vd = torch.empty((T, n1), dtype=torch.uint8, device="cuda")

    def run_a():
        npz.create_device(ws, tri, ks, n_kp, skip, first, dE, has, 2 * nb, EPI, out, m12, vd)
    st = torch.cuda.current_stream().cuda_stream
    nmatch = torch.zeros(1, dtype=torch.int32, device="cuda")
    dptr = lambda k, o, w: keep[k].data_ptr() + int(o) * w  # noqa: E731

    def matcher(t, m_out):
        o2 = off[t + 1]
        rc = L.mcs_search_for_triangulation_raw_device(
            tri._h, dptr("desc", 0, nb), None, dptr("kp_cam", 0, 4), has.data_ptr(), dptr("rays", 0, 24), n1,
            dptr("desc", o2, nb), None, dptr("kp_cam", o2, 4), has.data_ptr() + int(o2), dptr("rays", o2, 24), n_kp[t + 1], 3,
            dE.data_ptr() + t * 81 * 8, nb, 2 * nb, EPI, m_out.data_ptr(), nmatch.data_ptr(), st)
        assert rc == 0

    def timed(fn, events=True):
        ms = []
        for k in range(a.warmup + a.iters):
            has.copy_(has0)
            torch.cuda.synchronize()
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                dt = e0.elapsed_time(e1)
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                ms.append(dt)
        return float(np.median(ms)), float(np.min(ms))
    a_med, a_min = timed(run_a)
    torch.cuda.synchronize()
    count = int(ot["count"].item())
    dev = {k: ot[k][:count].cpu().numpy() for k in ("kp1", "kp2", "neighbour", "pos", "normal", "min_dist", "max_dist", "desc")}
    dev_has = has.cpu().numpy()
    m_med, m_min = timed(lambda: [matcher(t, m12[t]) for t in range(T)])
    with tempfile.TemporaryDirectory() as tmp:
        C = build_cpu(tmp)
        box = {}

        def run_b():
            res = None
            h = [has0[off[t]:off[t + 1]].cpu().numpy().copy() for t in range(T + 1)]     # the caller's host copy of the flags
            for t in range(T):
                matcher(t, m12[t])
                m = m12[t].cpu().numpy()                                                # download (synchronises)
                res = cpu_pair(C, rig, kf1, kf2s[t], m, first[t], t, h[0], h[t + 1], None if res is None else res["_bufs"])
                has[off[0]:off[1]].copy_(torch.from_numpy(h[0]))                         # upload both flag arrays
                has[off[t + 1]:off[t + 2]].copy_(torch.from_numpy(h[t + 1]))
            box["res"], box["has"] = res, np.concatenate(h)
        b_med, b_min = timed(run_b, events=False)
    cpu = box["res"]
    same = count == int(cpu["count"][0]) and all(np.array_equal(dev[k], cpu[k]) for k in ("kp1", "kp2", "neighbour", "desc")) \
        and np.array_equal(dev_has, box["has"])
    if same:
        for k in ("pos", "normal", "min_dist", "max_dist"):
            d = np.abs(dev[k] - cpu[k]).reshape(count, -1).max(1) / np.abs(cpu[k]).reshape(count, -1).max(1)
            same = same and bool((d <= TOL_X).all())
    if not same:
        raise SystemExit("the device's points differ from the CPU loop's (%d against %d)" % (count, int(cpu["count"][0])))
    res = {"metric": "create_new_map_points_ms_per_keyframe", "cameras": 3, "keypoints_current_keyframe": n1,
           "neighbours": T, "bytes": nb, "tracked_fraction": float(np.mean(kf1["has_mp"])), "iters": a.iters, "warmup": a.warmup,
           "points_created": count, "device_entry_ms_median": a_med, "device_entry_ms_min": a_min,
           "matcher_only_ms_median": m_med, "matcher_only_ms_min": m_min,
           "new_kernels_ms_median": a_med - m_med, "host_round_trip_ms_median": b_med, "host_round_trip_ms_min": b_min,
           "points_equal": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
