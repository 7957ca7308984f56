"""SearchByBoW on the GPU: the fixture evaluated from the reference's text (tests/golden/bow_ref.npz)
and, at other shapes, the NumPy restatement of tests/test_bow_ref.py (itself pinned by the
fixture).  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_bow_ref import (A_SCENARIOS, B_SCENARIOS, a_frames, b_frames, build_demo,
                                np_search_by_bow, np_search_by_bow_kf)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOC = os.path.join(ROOT, "tests", "golden", "small_orb_omni_voc_9_6.npz")
pytestmark = pytest.mark.gpu


def _bm():
    from mcs_amd import bow_match
    return bow_match


# ------------------------------------------------------------------ helpers
def dev_a(f, kfs, nbytes, th, nnratio=0.75, orient=False, ws=None):
    import torch
    bm = _bm()
    ws = ws or bm.Workspace(max([1, len(f["desc"])] + [len(k["desc"]) for k in kfs]), max(1, len(kfs)))
    fs, k1 = bm.device_set(bm.pack([f], nbytes))
    ks, k2 = bm.device_set(bm.pack(list(kfs), nbytes))
    m, n = bm.search_by_bow_device(ws, fs, ks, nbytes, th, nnratio, orient)
    torch.cuda.synchronize()
    return m.cpu().numpy(), n.cpu().numpy()


def dev_b(k1, k2s, nbytes, th, nnratio=0.75, ws=None):
    import torch
    bm = _bm()
    ws = ws or bm.Workspace(max([1, len(k1["desc"])] + [len(k["desc"]) for k in k2s]), max(1, len(k2s)))
    s1, a1 = bm.device_set(bm.pack([k1], nbytes, with_fv=False))
    s2, a2 = bm.device_set(bm.pack(list(k2s), nbytes, with_fv=False))
    m, n = bm.search_by_bow_kf_device(ws, s1, s2, nbytes, th, nnratio)
    torch.cuda.synchronize()
    return m.cpu().numpy(), n.cpu().numpy()


def flip(d, nbits, rng):
    bits = np.unpackbits(d)
    if nbits:
        bits[rng.choice(bits.size, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def rand_masks(rng, n, nbytes):
    return np.packbits((rng.random((n, nbytes * 8)) < 0.85).astype(np.uint8), axis=1)


def rand_pair_a(rng, kf_sizes, f_sizes, nbytes=32, masked=False, max_flip=40):
    """A keyframe and a frame whose vocabulary nodes have the given sizes (node j has
    kf_sizes[j] keyframe and f_sizes[j] frame keypoints; 0 = absent on that side).  Frame
    descriptors are noisy copies of keyframe descriptors of the same node, with exact copies."""
    nodes = [3 + 5 * j for j in range(len(kf_sizes))]
    nk, nf = int(sum(kf_sizes)), int(sum(f_sizes))
    knode = np.repeat(nodes, kf_sizes)[rng.permutation(nk)] if nk else np.zeros(0, int)
    fnode = np.repeat(nodes, f_sizes)[rng.permutation(nf)] if nf else np.zeros(0, int)
    kd = rng.integers(0, 256, (nk, nbytes), dtype=np.uint8)
    fd = rng.integers(0, 256, (nf, nbytes), dtype=np.uint8)
    for i in range(nf):
        src = np.flatnonzero(knode == fnode[i])
        if len(src) and rng.random() < 0.85:
            fd[i] = flip(kd[rng.choice(src)], int(rng.integers(0, max_flip + 1)) * int(rng.random() < 0.9), rng)
    fv = lambda nd: {int(x): np.flatnonzero(nd == x).tolist() for x in sorted(set(nd.tolist()))}  # noqa: E731
    kf = dict(desc=kd, mask=rand_masks(rng, nk, nbytes) if masked else None,
              angle=rng.integers(0, 360, nk).astype(np.float32), has_mp=(rng.random(nk) < 0.8).astype(np.uint8),
              fv=fv(knode))
    f = dict(desc=fd, mask=rand_masks(rng, nf, nbytes) if masked else None,
             angle=rng.integers(0, 360, nf).astype(np.float32), fv=fv(fnode))
    return f, kf


def rand_pair_b(rng, n1, n2, nbytes=32, masked=False, max_flip=40):
    d1 = rng.integers(0, 256, (n1, nbytes), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
    for j in range(n2):
        if n1 and rng.random() < 0.8:
            d2[j] = flip(d1[rng.integers(n1)], int(rng.integers(0, max_flip + 1)) * int(rng.random() < 0.9), rng)
    k1 = dict(desc=d1, mask=rand_masks(rng, n1, nbytes) if masked else None,
              has_mp=(rng.random(n1) < 0.7).astype(np.uint8))
    k2 = dict(desc=d2, mask=rand_masks(rng, n2, nbytes) if masked else None,
              has_mp=(rng.random(n2) < 0.7).astype(np.uint8))
    return k1, k2


# ------------------------------------------------------------------ the reference text's outputs
@pytest.mark.parametrize("name", A_SCENARIOS)
def test_overload_a_matches_reference_text(gpu, name):
    f, kf, e = a_frames(name)
    m, n = _bm().search_by_bow(f, [kf], th=e["th"], nnratio=e["nnratio"], check_orientation=e["orient"])
    assert n.tolist() == [e["n"]] and np.array_equal(m[0], e["match"])
    m, n = dev_a(f, [kf], e["nbytes"], e["th"], e["nnratio"], e["orient"])
    assert n.tolist() == [e["n"]] and np.array_equal(m[0], e["match"])


@pytest.mark.parametrize("name", B_SCENARIOS)
def test_overload_b_matches_reference_text(gpu, name):
    k1, k2, e = b_frames(name)
    m, n = _bm().search_by_bow_kf(k1, [k2], th=e["th"], nnratio=e["nnratio"])
    assert n.tolist() == [e["n"]] and np.array_equal(m[0], e["match"])
    m, n = dev_b(k1, [k2], e["nbytes"], e["th"], e["nnratio"])
    assert n.tolist() == [e["n"]] and np.array_equal(m[0], e["match"])


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("orient", [False, True])
def test_overload_a_batch_of_seven_equals_single_calls(gpu, orient):
    """F against 7 candidates of different sizes (one empty, one with a single keypoint) in one
    call: every row equals the single call and the NumPy restatement."""
    rng = np.random.default_rng(41)
    f, kf0 = rand_pair_a(rng, [70, 30, 10, 0, 25], [80, 40, 0, 12, 30])
    sizes = [[70, 30, 10, 0, 25], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [5, 90, 3, 7, 0], [33, 0, 0, 0, 64],
             [0, 65, 0, 0, 0], [20, 20, 20, 20, 20]]
    kfs = [kf0]
    for s in sizes[1:]:
        _, kf = rand_pair_a(rng, s, [0] * 5)
        for i in range(len(kf["desc"])):        # make them look like F
            if rng.random() < 0.7:
                kf["desc"][i] = flip(f["desc"][rng.integers(len(f["desc"]))], int(rng.integers(0, 30)), rng)
        kfs.append(kf)
    m, n = dev_a(f, kfs, 32, 64, 0.75, orient)
    total = 0
    for k, kf in enumerate(kfs):
        em, en = np_search_by_bow(f, kf, 64, 0.75, orient)
        assert n[k] == en and np.array_equal(m[k], em), k
        m1, n1 = dev_a(f, [kf], 32, 64, 0.75, orient)
        assert n1[0] == en and np.array_equal(m1[0], em), k
        total += en
    assert total >= 30 and n[1] == 0


@pytest.mark.parametrize("ncand", [1, 5])
def test_overload_b_batch_equals_single_calls(gpu, ncand):
    rng = np.random.default_rng(43 + ncand)
    k1, _ = rand_pair_b(rng, 220, 1)
    k2s = []
    for n2 in [260, 0, 1, 130, 301][:ncand]:
        k2 = rand_pair_b(rng, 0, n2)[1]
        for j in range(n2):
            if rng.random() < 0.8:
                k2["desc"][j] = flip(k1["desc"][rng.integers(220)], int(rng.integers(0, 40)), rng)
        k2s.append(k2)
    m, n = dev_b(k1, k2s, 32, 64)
    for k, k2 in enumerate(k2s):
        em, en = np_search_by_bow_kf(k1, k2, 64, 0.75)
        assert n[k] == en and np.array_equal(m[k], em), k
        m1, n1 = dev_b(k1, [k2], 32, 64)
        assert n1[0] == en and np.array_equal(m1[0], em), k
    assert n[0] >= 30


# ------------------------------------------------------------------ lane and segment boundaries
NODE_SIZES = [1, 63, 64, 65, 129, 300]


@pytest.mark.parametrize("nbytes,masked,reverse", [(32, False, False), (32, False, True), (16, True, False),
                                                   (64, False, True), (32, True, True)])
def test_overload_a_node_sizes_at_lane_boundaries(gpu, nbytes, masked, reverse):
    """Node sizes 1, 63, 64, 65, 129 and 300 on each side (same order, and crossed so that a
    300-entry keyframe node meets a 1-entry frame node)."""
    rng = np.random.default_rng(50 + nbytes + int(masked))
    f, kf = rand_pair_a(rng, NODE_SIZES, NODE_SIZES[::-1] if reverse else NODE_SIZES, nbytes, masked,
                        max_flip=nbytes)
    th = nbytes if masked else 2 * nbytes
    em, en = np_search_by_bow(f, kf, th, 0.75, True)
    assert en >= 30
    m, n = dev_a(f, [kf], nbytes, th, 0.75, True)
    assert n[0] == en and np.array_equal(m[0], em)
    m, n = _bm().search_by_bow(f, [kf], th=th, check_orientation=True)
    assert n[0] == en and np.array_equal(m[0], em)


@pytest.mark.parametrize("n2", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("nbytes,masked", [(32, False), (16, True)])
def test_overload_b_n2_at_tile_boundaries(gpu, n2, nbytes, masked):
    rng = np.random.default_rng(60 + n2)
    k1, k2 = rand_pair_b(rng, 200, n2, nbytes, masked, max_flip=nbytes)
    th = nbytes if masked else 2 * nbytes
    em, en = np_search_by_bow_kf(k1, k2, th, 0.75)
    m, n = dev_b(k1, [k2], nbytes, th)
    assert n[0] == en and np.array_equal(m[0], em)
    assert en > 0 or n2 == 1          # the case is not empty


def test_overload_b_slot_overflow_is_exact(gpu):
    """One group of KF1 queries has 40 consecutive near-duplicate KF2 keypoints within the
    candidate bound: more than a (query, segment) slot list holds, so those queries take the
    exact rescan of the ordered pass."""
    rng = np.random.default_rng(71)
    k1, k2 = rand_pair_b(rng, 150, 512)
    proto = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in range(60, 72):
        k1["desc"][i] = flip(proto, int(rng.integers(0, 5)), rng)
        k1["has_mp"][i] = 1
    for j in range(100, 140):
        k2["desc"][j] = flip(proto, int(rng.integers(0, 7)), rng)
    k2["has_mp"][100:140] = 1
    k2["desc"][101] = k2["desc"][100]
    em, en = np_search_by_bow_kf(k1, k2, 64, 0.75)
    m, n = dev_b(k1, [k2], 32, 64)
    assert n[0] == en and np.array_equal(m[0], em)
    # nnratio above 1 and a loose ratio: the bound follows th_low - 1
    for ratio in (1.5, 0.3):
        em, en = np_search_by_bow_kf(k1, k2, 64, ratio)
        m, n = dev_b(k1, [k2], 32, 64, nnratio=ratio)
        assert n[0] == en and np.array_equal(m[0], em), ratio


# ------------------------------------------------------------------ device FeatureVector
def _fv_device(V, ws, desc, levelsup):
    import torch
    bm = _bm()
    d = torch.from_numpy(desc).cuda()
    word, weight, node = V.transform_words(d, levelsup)
    fv_node, fv_ptr, fv_feat, fv_n = bm.feature_vector_device(ws, node, weight)
    torch.cuda.synchronize()
    m = int(fv_n.item())
    node, ptr, feat = fv_node.cpu().numpy()[:m], fv_ptr.cpu().numpy()[:m + 1], fv_feat.cpu().numpy()
    return {int(node[j]): feat[ptr[j]:ptr[j + 1]].tolist() for j in range(m)}, (fv_node, fv_ptr, fv_feat, fv_n)


@pytest.mark.parametrize("which", ["real", "ragged"])
def test_feature_vector_device_equals_host_transform(gpu, which):
    from mcs_amd import vocab
    if which == "real":
        v, levelsup, n = vocab.load_npz(VOC), 4, 600
    else:
        v, levelsup, n = vocab.synthetic(k=6, L=4, seed=9, stop_frac=0.3, ragged=True), 2, 333
    V = vocab.Vocabulary(v)
    ws = _bm().Workspace(700, 1)
    desc = np.random.default_rng(81).integers(0, 256, (n, 32), dtype=np.uint8)
    _, host_fv = V.transform(desc, levelsup)
    dev_fv, _ = _fv_device(V, ws, desc, levelsup)
    assert dev_fv == host_fv and len(host_fv) > 1
    if which == "ragged":
        assert sum(len(x) for x in host_fv.values()) < n     # stopped words were dropped
    dev_fv2, _ = _fv_device(V, ws, desc[:1], levelsup)        # the same workspace, another size
    assert dev_fv2 == V.transform(desc[:1], levelsup)[1]


def test_transform_to_match_stays_on_device(gpu):
    """extract -> BoW -> match: transform on device, FeatureVector on device, SearchByBoW on
    device equals the NumPy restatement fed the host FeatureVector."""
    import torch
    from mcs_amd import vocab
    bm = _bm()
    V = vocab.Vocabulary(vocab.load_npz(VOC))
    rng = np.random.default_rng(91)
    nk, nf = 500, 450
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    fd = np.stack([flip(kd[rng.integers(nk)], int(rng.integers(0, 12)), rng) for _ in range(nf)])
    has = (rng.random(nk) < 0.8).astype(np.uint8)
    ka, fa = rng.integers(0, 360, nk).astype(np.float32), rng.integers(0, 360, nf).astype(np.float32)
    ws = bm.Workspace(max(nk, nf), 1)
    sets = []
    for d, ang, hm in ((fd, fa, None), (kd, ka, has)):
        _, (fv_node, fv_ptr, fv_feat, fv_n) = _fv_device(V, ws, d, 4)
        n = len(d)
        keep = dict(desc=torch.from_numpy(d).cuda(), angle=torch.from_numpy(ang).cuda(),
                    off=torch.tensor([0, n], dtype=torch.int32, device="cuda"),
                    has=torch.from_numpy(hm if hm is not None else np.zeros(n, np.uint8)).cuda(),
                    fv=(fv_node, fv_ptr, fv_feat, fv_n))
        s = bm.BowSet(1, n)
        s.off, s.desc, s.angle, s.has_mp = (keep[k].data_ptr() for k in ("off", "desc", "angle", "has"))
        s.fv_node, s.fv_ptr, s.fv_feat, s.fv_n = (t.data_ptr() for t in keep["fv"])
        sets.append((s, keep))
    m, n = bm.search_by_bow_device(ws, sets[0][0], sets[1][0], 32, 64, 0.75, True)
    torch.cuda.synchronize()
    f = dict(desc=fd, angle=fa, fv=V.transform(fd, 4)[1])
    kf = dict(desc=kd, angle=ka, has_mp=has, fv=V.transform(kd, 4)[1])
    em, en = np_search_by_bow(f, kf, 64, 0.75, True)
    assert en >= 30
    assert int(n[0]) == en and np.array_equal(m[0].cpu().numpy(), em)


# ------------------------------------------------------------------ workspace
def test_workspace_reuse_leaks_no_state(gpu):
    """Two calls of each overload on one workspace, with different sizes and the orientation
    check on, give what fresh workspaces give."""
    bm = _bm()
    rng = np.random.default_rng(95)
    fa, ka = rand_pair_a(rng, [90, 40, 130], [100, 30, 120])
    fb, kb = rand_pair_a(rng, [20, 0, 70], [10, 35, 66])
    k1a, k2a = rand_pair_b(rng, 300, 500)
    k1b, k2b = rand_pair_b(rng, 120, 90)
    ws = bm.Workspace(600, 2)
    got = [dev_a(fa, [ka, kb], 32, 64, 0.75, True, ws=ws), dev_b(k1a, [k2a, k2b], 32, 64, ws=ws),
           dev_a(fb, [kb], 32, 64, 0.75, True, ws=ws), dev_b(k1b, [k2b], 32, 64, ws=ws)]
    fresh = [dev_a(fa, [ka, kb], 32, 64, 0.75, True), dev_b(k1a, [k2a, k2b], 32, 64),
             dev_a(fb, [kb], 32, 64, 0.75, True), dev_b(k1b, [k2b], 32, 64)]
    for (m, n), (em, en) in zip(got, fresh):
        assert np.array_equal(m, em) and np.array_equal(n, en)
    assert np.array_equal(got[2][0][0], np_search_by_bow(fb, kb, 64, 0.75, True)[0])
    assert np.array_equal(got[3][0][0], np_search_by_bow_kf(k1b, k2b, 64, 0.75)[0])


def test_workspace_too_small_is_an_argument_error(gpu):
    import ctypes
    import mcs_amd
    bm = _bm()
    rng = np.random.default_rng(97)
    f, kf = rand_pair_a(rng, [40, 30], [45, 30])
    ws = bm.Workspace(70, 1)                       # kf has 70 keypoints, f has 75
    with pytest.raises(mcs_amd.McsError) as ei:
        dev_a(f, [kf], 32, 64, ws=ws)
    assert ei.value.code == mcs_amd.MCS_ERR_ARG
    k1, k2 = rand_pair_b(rng, 60, 80)
    with pytest.raises(mcs_amd.McsError) as ei:
        dev_b(k1, [k2, k2], 32, 64, ws=ws)         # two candidates, room for one
    assert ei.value.code == mcs_amd.MCS_ERR_ARG
    node = ctypes.c_void_p(16)
    assert mcs_amd.lib().mcs_feature_vector_device(ws._h, node, node, 71, node, node, node, node, None) == \
        mcs_amd.MCS_ERR_ARG


# ------------------------------------------------------------------ the C++ adapter
def _write_frames(path, mode, nbytes, th, orient, nnratio, frames):
    with open(path, "wb") as fh:
        fh.write(np.array([mode, nbytes, th, int(orient), len(frames)], np.int32).tobytes())
        fh.write(np.array([nnratio], np.float64).tobytes())
        for fr in frames:
            n = len(fr["desc"])
            node, ptr, feat = fr.get("fv", (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)))
            masked = fr.get("mask") is not None
            fh.write(np.array([n, int(masked), len(node), len(feat)], np.int32).tobytes())
            fh.write(np.ascontiguousarray(fr["desc"], np.uint8).tobytes())
            if masked:
                fh.write(np.ascontiguousarray(fr["mask"], np.uint8).tobytes())
            fh.write(np.asarray(fr.get("angle", np.zeros(n)), np.float32).tobytes())
            fh.write(np.asarray(fr.get("has_mp", np.zeros(n)), np.uint8).tobytes())
            fh.write(np.asarray(node, np.uint32).tobytes())
            if len(node):
                fh.write(np.asarray(ptr, np.int32).tobytes())
            fh.write(np.asarray(feat, np.uint32).tobytes())


def test_cpp_adapter_runs_both_overloads(gpu, tmp_path):
    exe = build_demo(tmp_path)
    f, kf, e = a_frames("a2")
    fin, fout = tmp_path / "a.bin", tmp_path / "a.out"
    _write_frames(fin, 0, 32, e["th"], True, e["nnratio"], [f, kf, kf])
    subprocess.check_call([exe, str(fin), str(fout)], timeout=120)
    out = np.fromfile(fout, np.int32).reshape(2, 1 + len(e["match"]))
    for k in range(2):
        assert out[k, 0] == e["n"] and np.array_equal(out[k, 1:], e["match"])
    k1, k2, eb = b_frames("b1")
    fin, fout = tmp_path / "b.bin", tmp_path / "b.out"
    _write_frames(fin, 1, 16, eb["th"], False, eb["nnratio"], [k1, k2])
    subprocess.check_call([exe, str(fin), str(fout)], timeout=120)
    out = np.fromfile(fout, np.int32)
    assert out[0] == eb["n"] and np.array_equal(out[1:], eb["match"])
