#!/usr/bin/env python3
"""Time mcs_optimize_sim3_device at the loop-closing shape: T = 3 candidates, a current keyframe
of 6000 keypoint slots, about 150 kept correspondences per candidate of which a tenth are gross
outliers (tests/sim3opt_cases.py on the Lafida rig), inputs resident, one workspace.

matches12 is in-out, so every call is preceded by a device copy that restores it.  Device events
go around batches of --batch calls; windows of (restore + call) alternate with windows of the
restore alone, and the call's time is the difference of the two medians.  Prints one JSON line
with the per-window figures and their spread; --out also writes it.

    python tools/sim3_opt_bench.py [--windows 7] [--batch 50] [--warmup 20] [--out profiles/sim3_opt_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multicol-slam-annotation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--slots", type=int, default=6000)
    ap.add_argument("--kept", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from mcs_amd import sim3_opt as so
    from tests import sim3opt_cases as sc
    T = 3
    sc.CASES["bench"] = dict(seed=2026, n1=a.slots, cands=[(a.slots, a.kept, a.kept // 10, 5)] * T, s=1.1,
                             start=(0.02, 0.05, 0.04))
    c = sc.make_case("bench")
    pk1, pp1, pk2, pp2, m12, o1, o2, f2 = so.pack_call(*sc.call_args(c))
    k1, p1, keep1 = so.device_sets(pk1, pp1)
    k2, p2, keep2 = so.device_sets(pk2, pp2)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()  # noqa: E731
    m_in, ok1, ok2, df2 = up(m12, np.int32), up(o1, np.uint8), up(o2, np.uint8), up(f2, np.int32)
    is1, s2 = up(c["inv_sigma2_1"], np.float64), up(c["sigma2_2"], np.float64)
    s, R, t = up(c["s12"], np.float64), up(c["R12"], np.float64), up(c["t12"], np.float64)
    n1 = pk1["n_kp_total"]
    ws, out, opts = so.Workspace(T, n1), so.new_out(T, n1), so.default_options()
    m = m_in.clone()

    def call():
        m.copy_(m_in)
        so.optimize_sim3_device(ws, k1, p1, k2, p2, m, ok1, ok2, df2, is1, s2, s, R, t, opts, out=out)

    def restore():
        m.copy_(m_in)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch          # us per call
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    first = {k: v.cpu().numpy().copy() for k, v in out[1].items()}
    both, rest = [], []
    for _ in range(a.windows):
        both.append(window(call))
        rest.append(window(restore))
    torch.cuda.synchronize()
    for k, v in out[1].items():                               # deterministic: the last call equals the first
        assert v.cpu().numpy().tobytes() == first[k].tobytes(), k
    res = {"metric": "optimize_sim3_us_per_call", "candidates": T, "slots": n1,
           "kept": first["n_corr"].tolist(), "n_bad": first["n_bad"].tolist(), "n_in": first["n_in"].tolist(),
           "iters": first["iters"].tolist(), "trials": first["trials"].sum(2).tolist(),
           "windows": a.windows, "batch": a.batch, "warmup": a.warmup,
           "restore_plus_call_us": [round(x, 2) for x in both], "restore_us": [round(x, 2) for x in rest],
           "call_us_median": round(float(np.median(both) - np.median(rest)), 2),
           "call_us_min": round(float(np.min(both) - np.median(rest)), 2),
           "call_us_max": round(float(np.max(both) - np.median(rest)), 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ws.close()


if __name__ == "__main__":
    main()
