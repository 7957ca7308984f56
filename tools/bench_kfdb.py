#!/usr/bin/env python3
"""Time the keyframe database queries on the device and on one CPU thread.

--n keyframes (default 2000) of 3 x 2000 descriptors on the Lafida vocabulary fixture
(tests/golden/small_orb_omni_voc_9_6.npz).  The descriptors of keyframe i are vocabulary words with
a few flipped bits, drawn from a window of the word list that slides with i, so neighbouring
keyframes share most of their words and distant ones few.  The query revisits the place of a
keyframe in the first quarter; its connected keyframes are the last 30, the neighbours of a
keyframe the ten nearest in time.  After a warm-up, median and minimum of --iters >= 20 of
  * one loop query (mcs_kfdb_detect_loop_device; events on the stream, everything resident, the
    minScore of mcs_kfdb_min_score_device read on the device),
  * one relocalisation query (mcs_kfdb_detect_reloc_device),
  * the minScore call, and one mcs_bow_vector_device of 6000 descriptors,
  * the same queries as plain single-thread -O3 C++ with a real inverted file
    (tests/cpp/kfdb_cpu.cpp), wall time.
Every iteration uses a fresh query id (a repeated id lists nothing), the same sequence on both
paths.  The tool fails unless both paths return the same candidates.  --sweep repeats the queries
for smaller databases and reports the N from which the device is faster.  Prints one JSON line;
--out also writes it.

    python tools/bench_kfdb.py [--n 2000] [--iters 30] [--warmup 5] [--sweep] [--out profiles/kfdb_bench.json]
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "small_orb_omni_voc_9_6.npz")
ND, WINDOW, STEP, NEIGH = 6000, 1500, 3, 10


def build_cpu(tmp):
    so = os.path.join(tmp, "libkfdb_cpu.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "kfdb_cpu.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    V, I = ctypes.c_void_p, ctypes.c_int
    L.kfdb_cpu_create.restype = V
    L.kfdb_cpu_create.argtypes = [I]
    L.kfdb_cpu_destroy.argtypes = [V]
    L.kfdb_cpu_add.argtypes = [V, V, V, I]
    L.kfdb_cpu_min_score.restype = ctypes.c_double
    L.kfdb_cpu_min_score.argtypes = [V, V, V, I, V, I]
    L.kfdb_cpu_detect.argtypes = [V, I, V, V, I, ctypes.c_int64, V, ctypes.c_double, V, V]
    return L


def descriptors(leaves, perm, place, rng):
    """ND descriptors around the words of the window at `place`."""
    idx = perm[(place * STEP + rng.integers(0, WINDOW, size=ND)) % len(perm)]
    d = leaves[idx].copy()
    for _ in range(3):
        pos = rng.integers(0, 256, size=ND)
        d[np.arange(ND), pos >> 3] ^= (1 << (pos & 7)).astype(np.uint8)
    return d


def stats(ms):
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20 (median of at least 20)")
    import torch
    from mcs_amd import bow_match, kfdb, vocab
    vd = vocab.load_npz(FIXTURE)
    voc = vocab.Vocabulary(vd)
    n_words = voc.info()["n_words"]
    order = np.argsort(vd["node_id"])
    leaves = vd["desc"][order][np.searchsorted(vd["node_id"][order], vd["word_node"])]
    rng = np.random.default_rng(2026)
    perm = rng.permutation(len(leaves))
    ws = bow_match.Workspace(ND, 1)
    N = a.n

    def bow_of(place):
        t = torch.from_numpy(descriptors(leaves, perm, place, rng)).cuda()
        word, weight, _ = voc.transform_words(t, 4)
        return voc.bow_vector(ws, word, weight), (word, weight)
    bows = [bow_of(i)[0] for i in range(N)]
    (qb, (q_word, q_weight)) = bow_of(N // 5)
    torch.cuda.synchronize()
    host = [(w.cpu().numpy()[:int(n.item())].view(np.uint32).copy(), v.cpu().numpy()[:int(n.item())].copy())
            for w, v, n in bows]
    qn = int(qb[2].item())
    qw, qv = qb[0].cpu().numpy()[:qn].view(np.uint32).copy(), qb[1].cpu().numpy()[:qn].copy()
    entries = int(sum(len(w) for w, _ in host))

    def bench(n, C):
        """Both paths on the first n keyframes -> dict of timings; fails on different candidates."""
        ng = np.full((n, NEIGH), -1, np.int32)
        for s in range(n):
            near = [s + d for d in (-1, 1, -2, 2, -3, 3, -4, 4, -5, 5) if 0 <= s + d < n]
            ng[s, :len(near)] = near
        conn = np.zeros(n, np.uint8)
        conn[max(0, n - 30):] = 1
        slots = np.flatnonzero(conn).astype(np.int32)
        db = kfdb.KeyFrameDatabase(voc, n, max(1, sum(len(w) for w, _ in host[:n])))
        for w, v, cnt in bows[:n]:
            db.add_device(w, v, cnt, n_upper=int(cnt.item()))
        d_ng, d_conn, d_slots = torch.from_numpy(ng).cuda(), torch.from_numpy(conn).cuda(), torch.from_numpy(slots).cuda()
        q = kfdb.query_of(*qb)
        dmin = torch.zeros(1, dtype=torch.float64, device="cuda")
        res, ts = kfdb.new_result(n, n, diagnostics=False)
        ids = {"loop": 10 ** 6, "reloc": 10 ** 6}

        def timed(fn, events):
            ms = []
            for k in range(a.warmup + a.iters):
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
                    dt = (time.perf_counter() - t0) * 1e3
                if k >= a.warmup:
                    ms.append(dt)
            return stats(ms)

        def dev_loop():
            ids["loop"] += 1
            db.detect_loop_device(q, ids["loop"], d_conn, dmin, d_ng, res)

        def dev_reloc():
            ids["reloc"] += 1
            db.detect_reloc_device(q, ids["reloc"], d_ng, res)
        out = {"keyframes": n}
        out["min_score_ms_median"], out["min_score_ms_min"] = timed(lambda: db.min_score_device(q, d_slots, dmin), True)
        out["loop_ms_median"], out["loop_ms_min"] = timed(dev_loop, True)
        dev_loop_c = ts["candidates"].cpu().numpy()[:int(ts["n_candidates"].item())].tolist()
        out["reloc_ms_median"], out["reloc_ms_min"] = timed(dev_reloc, True)
        dev_reloc_c = ts["candidates"].cpu().numpy()[:int(ts["n_candidates"].item())].tolist()
        dev_min = float(dmin.item())
        # ---- one CPU thread, inverted file
        h = C.kfdb_cpu_create(n_words)
        for w, v in host[:n]:
            C.kfdb_cpu_add(h, w.ctypes.data, v.ctypes.data, len(w))
        cand, box = np.zeros(n + 1, np.int32), {}
        cpu_min = C.kfdb_cpu_min_score(h, qw.ctypes.data, qv.ctypes.data, qn, slots.ctypes.data, len(slots))
        ids = {"loop": 10 ** 6, "reloc": 10 ** 6}

        def cpu(kind):
            ids[kind] += 1
            box[kind] = C.kfdb_cpu_detect(h, 1 if kind == "loop" else 0, qw.ctypes.data, qv.ctypes.data, qn, ids[kind],
                                          conn.ctypes.data, cpu_min, ng.ctypes.data, cand.ctypes.data)
        out["cpu_loop_ms_median"], out["cpu_loop_ms_min"] = timed(lambda: cpu("loop"), False)
        cpu_loop_c = cand[:box["loop"]].tolist()
        out["cpu_reloc_ms_median"], out["cpu_reloc_ms_min"] = timed(lambda: cpu("reloc"), False)
        cpu_reloc_c = cand[:box["reloc"]].tolist()
        C.kfdb_cpu_destroy(h)
        if np.float64(dev_min).tobytes() != np.float64(cpu_min).tobytes() or dev_loop_c != cpu_loop_c or \
                dev_reloc_c != cpu_reloc_c:
            raise SystemExit("n=%d: the device's candidates differ from the CPU's: loop %r / %r, reloc %r / %r, min %r / %r"
                             % (n, dev_loop_c, cpu_loop_c, dev_reloc_c, cpu_reloc_c, dev_min, cpu_min))
        out["loop_candidates"], out["reloc_candidates"] = len(dev_loop_c), len(dev_reloc_c)
        out["entries"] = int(sum(len(w) for w, _ in host[:n]))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        C = build_cpu(tmp)
        main_res = bench(N, C)
        sweep = []
        if a.sweep:
            n = N // 2
            while n >= 16:
                sweep.append(bench(n, C))
                n //= 2
    # one BowVector of 6000 descriptors
    ms = []
    bw, bv, bn = (torch.zeros(ND, dtype=torch.int32, device="cuda"), torch.zeros(ND, dtype=torch.float64, device="cuda"),
                  torch.zeros(1, dtype=torch.int32, device="cuda"))
    st = torch.cuda.current_stream().cuda_stream
    for k in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        voc.bow_vector_device(ws, q_word.data_ptr(), q_weight.data_ptr(), ND, bw.data_ptr(), bv.data_ptr(), bn.data_ptr(), st)
        e1.record()
        e1.synchronize()
        if k >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    res = {"metric": "kfdb_query_ms", "vocabulary_words": n_words, "descriptors_per_keyframe": ND, "iters": a.iters,
           "warmup": a.warmup, "query_bow_entries": qn, "mean_bow_entries": entries / max(N, 1)}
    res.update(main_res)
    res["bow_vector_ms_median"], res["bow_vector_ms_min"] = stats(ms)
    res["candidates_equal"] = True
    if sweep:
        res["sweep"] = sweep
        rows = sorted(sweep + [main_res], key=lambda r: r["keyframes"])
        for kind in ("loop", "reloc"):
            wins = [r["keyframes"] for r in rows if r[kind + "_ms_median"] < r["cpu_" + kind + "_ms_median"]]
            loses = [r["keyframes"] for r in rows if not r[kind + "_ms_median"] < r["cpu_" + kind + "_ms_median"]]
            res[kind + "_device_faster_from_n"] = min(wins) if wins and (not loses or min(wins) > max(loses)) else None
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
