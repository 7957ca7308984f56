#!/usr/bin/env python3
"""Time mcs_optimize_essential_graph_device at map sizes a loop closure meets: N keyframes in a
drifted chain that a loop closes (tests/essgraph_cases.py), each covisible with its --nbr
predecessors (with the parent about 8 edges per keyframe), --points map points, inputs resident,
one workspace.  --solver dense (the tiled LDL^T of the workspace entry), sparse (the block-sparse
LDL^T over a plan, any number of keyframes) or both: with both, the windows of the two solvers
alternate inside one process, so that both see the same clocks.  --cov adds C_cov40's loop
connections and second neighbours (essgraph_cases.make_case `cov`): loop connections that join free
keyframes across the chain, the case a real loop produces; the dense system's tile band is then
the whole matrix.

The points are corrected in place, so every call is preceded by a device copy that restores them.
Device events go around batches of --batch calls; windows of (restore + call) alternate with
windows of the restore alone, and the call's time is the difference of the two medians.  Prints
one JSON line per size; --out appends them to a file.

--cpu-reference DRIVER times the reference's own g2o on the same inputs instead (wall clock of the
driver process tests/cpp/essgraph_g2o_driver.cpp, mode 0, on the CPU; no GPU is used): a scale, not
a comparison of like with like.

    python tools/essential_graph_bench.py [--n 200 800] [--points 50000] [--out profiles/essential_graph_bench.json]
"""
import argparse
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


def make(n, points, nbr, cov=False):
    from tests import essgraph_cases as ec
    ec.CASES["bench"] = dict(seed=2026, N=n, drift=(0.10, 0.5, 1.10), P=points, n_corr=4, nbr=nbr, cov=cov)
    return ec, ec.make_case("bench")


def cpu_reference(a, n):
    ec, c = make(n, a.points, a.nbr, a.cov)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.txt")
        ec.write_case_file(c, path)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = subprocess.check_output([a.cpu_reference, path, "0"], text=True)
            times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        subprocess.check_output([a.cpu_reference, path, "4"], text=True)      # reading the case + the edge list
        base = time.perf_counter() - t0
    r = ec.parse_results(out)
    return {"metric": "reference_g2o_driver_CPU_wall_ms", "keyframes": n, "edges": int(len(r["edges"])),
            "points": a.points, "iterations": r["iterations"], "trials": r["trials"].tolist(),
            "wall_ms": [round(1e3 * t, 1) for t in times], "read_and_select_only_ms": round(1e3 * base, 1)}


def gpu(a, n):
    import torch
    from mcs_amd import essential_graph as es
    ec, c = make(n, a.points, a.nbr, a.cov)
    edges, counts = es.select_edges(c["ids"], c["parent"], c["has_corr"], (c["loop_ptr"], c["loop_idx"]),
                                    (c["cov_ptr"], c["cov_idx"], c["cov_w"]), (c["lc_ptr"], c["lc_idx"], c["lc_w"]),
                                    c["cur"], c["loop"], c["min_weight"])
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()  # noqa: E731
    Scw, Snc, dE = up(c["Scw"], np.float64), up(c["Snc"], np.float64), up(edges, np.int32)
    pos_in, ref, bad = up(c["pos"], np.float64), up(ec.point_refs(c), np.int32), up(c["bad"], np.uint8)
    band = es.tile_band(n, c["loop"], edges)
    opts = es.default_options(tile_band=band)
    solvers = ["dense", "sparse"] if a.solver == "both" else [a.solver]
    out = es.new_out(n, len(edges))
    pos = pos_in.clone()
    ws = es.Workspace(n, len(edges), a.points) if "dense" in solvers else None
    plan, plan_ms = None, None
    if "sparse" in solvers:
        t0 = time.perf_counter()
        plan = es.Plan(n, c["loop"], edges, max_points=a.points, leaf_size=a.leaf)
        plan_ms = 1e3 * (time.perf_counter() - t0)           # host planning + the device allocation and upload

    def call_dense():
        pos.copy_(pos_in)
        es.optimize_device(ws, Scw, Snc, c["loop"], dE, pos, ref, bad, opts, out=out)

    def call_sparse():
        pos.copy_(pos_in)
        es.optimize_planned_device(plan, Scw, Snc, dE, pos, ref, bad, opts, out=out)
    calls = {"dense": call_dense, "sparse": call_sparse}

    def restore():
        pos.copy_(pos_in)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch                 # ms per call
    first = {}
    for sv in solvers:
        for _ in range(a.warmup):
            calls[sv]()
        torch.cuda.synchronize()
        first[sv] = {k: v.cpu().numpy().copy() for k, v in out[1].items()}
        assert first[sv]["status"][0] == 0
    both, rest = {sv: [] for sv in solvers}, []
    for _ in range(a.windows):
        for sv in solvers:
            both[sv].append(window(calls[sv]))
        rest.append(window(restore))
    torch.cuda.synchronize()
    for k, v in out[1].items():                               # deterministic: the last call equals the solver's first
        assert v.cpu().numpy().tobytes() == first[solvers[-1]][k].tobytes(), k
    res = {"metric": "optimize_essential_graph_ms_per_call", "keyframes": n, "edges": int(len(edges)),
           "edges_per_source": counts.tolist(), "points": a.points, "system": 7 * (n - 1), "cov": bool(a.cov),
           "tile_band": band, "tiles": (7 * (n - 1) + 63) // 64, "windows": a.windows, "batch": a.batch,
           "warmup": a.warmup, "restore_ms": [round(x, 4) for x in rest]}
    for sv in solvers:
        f = first[sv]
        it = int(f["iterations"][0])
        res[sv] = {"iterations": it, "trials": f["trials"][:it].tolist(),
                   "chi2": [float(f["chi2"][0]), float(f["chi2"][max(it - 1, 0)])],
                   "restore_plus_call_ms": [round(x, 3) for x in both[sv]],
                   "call_ms_median": round(float(np.median(both[sv]) - np.median(rest)), 3),
                   "call_ms_min": round(float(np.min(both[sv]) - np.median(rest)), 3),
                   "call_ms_max": round(float(np.max(both[sv]) - np.median(rest)), 3)}
    if plan is not None:
        res["sparse"]["plan"] = dict(plan.info, plan_create_ms=round(plan_ms, 2))
        plan.close()
    if ws is not None:
        ws.close()
    if len(solvers) == 2:
        res["sparse_faster_in_every_window"] = bool(all(s < d for s, d in zip(both["sparse"], both["dense"])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 800])
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--nbr", type=int, default=7)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solver", choices=["dense", "sparse", "both"], default="dense")
    ap.add_argument("--cov", action="store_true")
    ap.add_argument("--leaf", type=int, default=None, help="leaf_size of the sparse plan")
    ap.add_argument("--cpu-reference", default=None, metavar="DRIVER")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for n in a.n:
        line = json.dumps(cpu_reference(a, n) if a.cpu_reference else gpu(a, n))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
