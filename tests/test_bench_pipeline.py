"""GPU: the bench's production schedule (two parts on two streams, pipelined steps with
double-buffered outputs) end to end.  bench.py raises when its post-run spot check of the last
pipelined step's output set (keypoints, descriptors, top-2 matches) differs from the oracle;
with --stage-timing 0 that check reads the pipelined set, not the one-stream stage-timed run.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps", [3, 4])   # last step in output set 0 / set 1
def test_bench_pipelined_parity(gpu, steps):
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", str(steps), "--warmup", "1",
            "--multiframes", "12", "--unique", "4", "--split", "2", "--pipeline", "1",
            "--stage-timing", "0", "--cpu-sample", "4", "--ba-calls", "0", "--gba-calls", "0",
            "--d-multiframes", "0", "--bow-reps", "0", "--tri-reps", "0", "--latency-reps", "0"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    pc = d["parity_check"]
    assert pc["of_step"] == "last timed step"
    assert pc["camera_frames_bitexact"] == 12 and pc["match_pairs_bitexact"] == 9
    assert "pipelined" in d["config"]["schedule"]


SIDE_FIELDS = ("roofline", "roofline_orient_desc", "roofline_octree", "cpu_baseline", "parity_check",
               "localba", "cpu_baseline_localba", "globalba", "cpu_baseline_globalba", "config_d",
               "bow", "cpu_baseline_bow", "triangulation", "cpu_baseline_triangulation", "latency",
               "match_ms_per_step")


def test_bench_plain_run_dumps_last_step(gpu, tmp_path):
    """A plain run (no --full) measures the headline figure alone, and --dump-outputs writes the
    last timed step's keypoints, descriptors and top-2 matches: float32, within 64 MB, and equal
    to the oracle's for every dumped camera-frame and pair."""
    import numpy as np
    import mcs_amd
    from mcs_amd import synth
    from tests import oracle_bind as ob
    out = tmp_path / "dump"
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--multiframes", "4", "--unique", "4", "--dump-outputs", str(out)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["full"] is False and d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert all(d[k] is None for k in SIDE_FIELDS) and d["stage_ms_per_step"] == {}
    a = {name: np.load(str(out / (name + ".npy"))) for name in d["dumped_outputs"]}
    assert sorted(a) == ["counts", "descriptors", "frame_index", "keypoints", "matches", "pair_index"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert int(a["counts"].sum()) == d["config"]["keypoints_per_step_per_gpu"]
    _, imgs, masks, midx, pairs = synth.config_b_batch(4, 4, 0, 754, 480, 3)
    frames = a["frame_index"].astype(int)
    assert list(frames) == list(range(12)) and len(a["pair_index"]) == 9   # small batch: all of it
    descs = {}
    for i, f in enumerate(frames):
        k, de = ob.extract(imgs[f], masks[midx[f]], nfeatures=2000)
        n = len(k)
        assert a["counts"][f] == n
        for j, name in enumerate(mcs_amd.KEYPOINT_DTYPE.names):
            assert np.array_equal(a["keypoints"][i, :n, j], k[name].astype(np.float32)), (f, name)
        assert np.array_equal(a["descriptors"][i, :n], de.astype(np.float32)), f
        assert not a["keypoints"][i, n:].any() and not a["descriptors"][i, n:].any()
        descs[f] = de
    for i, p in enumerate(a["pair_index"].astype(int)):
        q, t = pairs[p]
        bi, bd, sd = ob.hamming_top2(descs[q], descs[t])
        n = len(bi)
        m = a["matches"][:, i]
        assert np.array_equal(m[0, :n], bi) and np.array_equal(m[1, :n], bd), p
        assert np.array_equal(m[3, :n], sd), p
        assert not m[:, n:].any()
