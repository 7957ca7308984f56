"""SearchByBoW against the reference's OWN text (CPU part).

tests/golden/bow_ref.npz holds, evaluated from the reference's text by tests/golden/gen_bow_ref.py,
the outputs of both SearchByBoW overloads (src/cORBmatcher.cpp:179-323, :885-966) on scripted
frames.  This module holds a plain NumPy restatement of the two overloads, pinned here against
that fixture; tests/test_bow_gpu.py uses it as the comparator at shapes the fixture does not have.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "bow_ref.npz")
INT_MAX = 2 ** 31 - 1
A_SCENARIOS = ["a0", "a1", "a2", "a3", "a3k", "a3f"]
B_SCENARIOS = ["b0", "b1", "b2"]
_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(FIX, allow_pickle=False)
        _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


# ------------------------------------------------------------------ NumPy restatement
def dist_matrix(d1, d2, m1=None, m2=None):
    """DescriptorDistance64 (:2443-2455) or, with masks, DescriptorDistance64Masked
    (:2457-2477: (popc(x & m1) + popc(x & m2)) / 2, integer division of the total)."""
    b1, b2 = np.unpackbits(d1, axis=1).astype(np.int32), np.unpackbits(d2, axis=1).astype(np.int32)
    if m1 is None:
        return b1.sum(1)[:, None] + b2.sum(1)[None, :] - 2 * (b1 @ b2.T)
    k1, k2 = np.unpackbits(m1, axis=1).astype(np.int32), np.unpackbits(m2, axis=1).astype(np.int32)
    # x & m1 summed: bits set in exactly one of d1, d2, under m1
    s1 = (b1 * k1).sum(1)[:, None] + k1 @ b2.T - 2 * ((b1 * k1) @ b2.T)
    s2 = b1 @ k2.T + (b2 * k2).sum(1)[None, :] - 2 * (b1 @ (b2 * k2).T)
    return (s1 + s2) // 2


def _top2(dists, idxs):
    """The update rule of :252-261 / :942-949 over candidates in order."""
    b1 = b2 = INT_MAX
    bi = -1
    for d, i in zip(dists, idxs):
        if d < b1:
            b2, b1, bi = b1, int(d), int(i)
        elif d < b2:
            b2 = int(d)
    return b1, bi, b2


def ori_bin(a_kf, a_f):
    """:274-279 in float32: rot, +360 if negative, cvRound(rot * (1.0f / 30)) half to even."""
    rot = np.float32(a_kf) - np.float32(a_f)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    factor = np.float32(1.0) / np.float32(30)
    b = int(np.rint(np.float32(rot * factor)))       # np.rint: half to even
    return 0 if b == 30 else b


def three_maxima(sizes):
    """ComputeThreeMaxima (:2399-2441)."""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        i2 = i3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        i3 = -1
    return i1, i2, i3


def fv_dict(fv):
    if isinstance(fv, dict):
        return {int(k): [int(x) for x in v] for k, v in fv.items()}
    node, ptr, feat = fv
    return {int(node[j]): [int(x) for x in feat[ptr[j]:ptr[j + 1]]] for j in range(len(node))}


def np_search_by_bow(f, kf, th_low, nnratio, check_orientation=False):
    """Overload A (:179-323) for one keyframe -> (match_f [n_f], nmatches)."""
    nf = len(f["desc"])
    match = np.full(nf, -1, np.int32)                                   # :185
    if nf == 0 or len(kf["desc"]) == 0:
        return match, 0
    D = dist_matrix(kf["desc"], f["desc"], kf.get("mask"), f.get("mask"))
    kfv, ffv = fv_dict(kf["fv"]), fv_dict(f["fv"])
    hist = [[] for _ in range(30)]
    n = 0
    for node in sorted(set(kfv) & set(ffv)):                            # :203-300
        for ik in kfv[node]:
            if not kf["has_mp"][ik]:                                    # :214-220
                continue
            cands = [i for i in ffv[node] if match[i] < 0]              # :237
            b1, bi, b2 = _top2([D[ik, i] for i in cands], cands)
            if b1 <= th_low and float(b1) < nnratio * float(b2):        # :264-266
                match[bi] = ik
                if check_orientation:
                    hist[ori_bin(kf["angle"][ik], f["angle"][bi])].append(bi)
                n += 1
    if check_orientation:                                               # :303-321
        keep = three_maxima([len(h) for h in hist])
        for b in range(30):
            if b in keep:
                continue
            for i in hist[b]:
                match[i] = -1
                n -= 1
    return match, n


def np_search_by_bow_kf(kf1, kf2, th_low, nnratio):
    """Overload B (:885-966) -> (matches12 [n1], nmatches)."""
    n1, n2 = len(kf1["desc"]), len(kf2["desc"])
    m12 = np.full(n1, -1, np.int32)
    if n1 == 0 or n2 == 0:
        return m12, 0
    D = dist_matrix(kf1["desc"], kf2["desc"], kf1.get("mask"), kf2.get("mask"))
    free = np.asarray(kf2["has_mp"]) != 0                               # :924-927, vbMatched2
    idx2 = np.arange(n2)
    n = 0
    for i1 in range(n1):
        if not kf1["has_mp"][i1]:                                       # :903-907
            continue
        c = idx2[free]
        if len(c) == 0:
            continue
        d = D[i1, c]
        o = np.argsort(d, kind="stable")[:2]                            # first minimum wins, second
        b1, bi = int(d[o[0]]), int(c[o[0]])                             # counts multiplicity
        b2 = int(d[o[1]]) if len(o) > 1 else INT_MAX
        if b1 < th_low and float(b1) < nnratio * float(b2):             # :952-955 (strict)
            m12[i1] = bi
            free[bi] = False
            n += 1
    return m12, n


# ------------------------------------------------------------------ fixture access
def a_frames(name):
    z = fixture()
    p = name + "_"
    nbytes, masked, orient, th = (int(x) for x in z[p + "meta"])
    f = dict(desc=z[p + "f_desc"], mask=z[p + "f_mask"] if masked else None, angle=z[p + "f_angle"],
             fv=(z[p + "f_fv_node"], z[p + "f_fv_ptr"], z[p + "f_fv_feat"]))
    kf = dict(desc=z[p + "kf_desc"], mask=z[p + "kf_mask"] if masked else None, angle=z[p + "kf_angle"],
              has_mp=z[p + "kf_has"], fv=(z[p + "kf_fv_node"], z[p + "kf_fv_ptr"], z[p + "kf_fv_feat"]))
    return f, kf, dict(nbytes=nbytes, th=th, orient=bool(orient), nnratio=float(z[p + "nnratio"]),
                       match=z[p + "match_f"], n=int(z[p + "nmatches"]))


def b_frames(name):
    z = fixture()
    p = name + "_"
    nbytes, masked, _, th = (int(x) for x in z[p + "meta"])
    k1 = dict(desc=z[p + "desc1"], mask=z[p + "mask1"] if masked else None, has_mp=z[p + "has1"])
    k2 = dict(desc=z[p + "desc2"], mask=z[p + "mask2"] if masked else None, has_mp=z[p + "has2"])
    return k1, k2, dict(nbytes=nbytes, th=th, nnratio=float(z[p + "nnratio"]), match=z[p + "matches12"],
                        n=int(z[p + "nmatches"]))


# ------------------------------------------------------------------ tests
def test_dist_matrix_is_the_popcount_distance():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (7, 32), dtype=np.uint8), rng.integers(0, 256, (9, 32), dtype=np.uint8)
    ma, mb = rng.integers(0, 256, (7, 32), dtype=np.uint8), rng.integers(0, 256, (9, 32), dtype=np.uint8)
    D, Dm = dist_matrix(a, b), dist_matrix(a, b, ma, mb)
    for i in range(7):
        for j in range(9):
            x = np.unpackbits(a[i] ^ b[j])
            assert D[i, j] == x.sum()
            assert Dm[i, j] == (int((x & np.unpackbits(ma[i])).sum()) + int((x & np.unpackbits(mb[j])).sum())) // 2


@pytest.mark.parametrize("name", A_SCENARIOS)
def test_numpy_overload_a_reproduces_reference_text(name):
    f, kf, e = a_frames(name)
    m, n = np_search_by_bow(f, kf, e["th"], e["nnratio"], e["orient"])
    assert n == e["n"]
    assert np.array_equal(m, e["match"])


@pytest.mark.parametrize("name", B_SCENARIOS)
def test_numpy_overload_b_reproduces_reference_text(name):
    k1, k2, e = b_frames(name)
    m, n = np_search_by_bow_kf(k1, k2, e["th"], e["nnratio"])
    assert n == e["n"]
    assert np.array_equal(m, e["match"])


def test_fixture_thresholds_and_maxima_are_the_reference_ones():
    z = fixture()
    assert int(z["histo_length"]) == 30
    assert [int(z[s + "_meta"][3]) for s in ("a0", "a1", "b0", "b1", "b2")] == [64, 32, 64, 16, 128]
    assert tuple(three_maxima(z["a2_hist"].tolist())) == tuple(int(x) for x in z["a2_maxima"])


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout")
def test_fixture_regenerates_from_reference_text(tmp_path):
    """In the build container the generator re-derives the fixture from the reference text."""
    out = tmp_path / "b.npz"
    gen = os.path.join(ROOT, "tests", "golden", "gen_bow_ref.py")
    subprocess.check_call([sys.executable, gen, "--out", str(out)], timeout=900)
    q, z = np.load(out), fixture()
    assert sorted(q.files) == sorted(z.keys())
    for k in q.files:
        assert np.array_equal(q[k], z[k]), k


NEW_SYMBOLS = ["mcs_bow_workspace_create", "mcs_bow_workspace_destroy", "mcs_feature_vector_device",
               "mcs_search_by_bow_device", "mcs_search_by_bow", "mcs_search_by_bow_kf_device",
               "mcs_search_by_bow_kf"]


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES, s
        assert hasattr(L, s), s


def _call_a(f, kf, nbytes=32, th=64, ori=0):
    import mcs_amd
    from mcs_amd import bow_match as bm
    fs, k1 = bm.host_set(f)
    ks, k2 = bm.host_set(kf)
    m = np.zeros(max(1, ks.n_frames * fs.n_kp_total), np.int32)
    n = np.zeros(max(1, ks.n_frames), np.int32)
    return mcs_amd.lib().mcs_search_by_bow(0, ctypes.byref(fs), ctypes.byref(ks), nbytes, th, 0.75, ori,
                                           m.ctypes.data, n.ctypes.data)


def _call_b(k1, k2, nbytes=32, th=64):
    import mcs_amd
    from mcs_amd import bow_match as bm
    s1, a1 = bm.host_set(k1)
    s2, a2 = bm.host_set(k2)
    m = np.zeros(max(1, s2.n_frames * s1.n_kp_total), np.int32)
    n = np.zeros(max(1, s2.n_frames), np.int32)
    return mcs_amd.lib().mcs_search_by_bow_kf(0, ctypes.byref(s1), ctypes.byref(s2), nbytes, th, 0.75,
                                              m.ctypes.data, n.ctypes.data)


def _small(masked=False):
    from mcs_amd import bow_match as bm
    f, kf, _ = a_frames("a1" if masked else "a3")
    return bm.pack([f], 32), bm.pack([kf], 32)


def test_host_entries_reject_bad_arguments_before_any_device(built):
    """Each MCS_ERR_ARG case of the two host entries; none of them reaches a device (the checks
    come first, so this passes on a machine without a GPU)."""
    import mcs_amd
    ARG = mcs_amd.MCS_ERR_ARG
    f, kf = _small()
    for nbytes in (0, 8, 24, 33, 128):
        assert _call_a(f, kf, nbytes=nbytes) == ARG
        assert _call_b(f, kf, nbytes=nbytes) == ARG
    fm, kfm = _small(masked=True)
    assert _call_a(dict(fm, mask=None), kfm) == ARG          # one mask without the other
    assert _call_a(fm, dict(kfm, mask=None)) == ARG
    assert _call_b(dict(fm, mask=None), kfm) == ARG
    assert _call_b(fm, dict(kfm, mask=None)) == ARG
    for side in (0, 1):
        bad = [dict(f), dict(kf)]
        nodes = bad[side]["fv_node"].copy()
        nodes[1] = nodes[0]                                   # not strictly ascending
        bad[side]["fv_node"] = nodes
        assert _call_a(*bad) == ARG
        bad = [dict(f), dict(kf)]
        nodes = bad[side]["fv_node"].copy()
        nodes[:2] = nodes[:2][::-1].copy()                    # descending
        bad[side]["fv_node"] = nodes
        assert _call_a(*bad) == ARG
        bad = [dict(f), dict(kf)]
        feat = bad[side]["fv_feat"].copy()
        feat[3] = bad[side]["n_kp_total"]                     # feature index == n_kp
        bad[side]["fv_feat"] = feat
        assert _call_a(*bad) == ARG
    assert _call_a(dict(f, angle=None), kf, ori=1) == ARG    # orientation check without angles
    two = dict(kf, n_frames=2, off=np.array([0, 10, kf["n_kp_total"]], np.int32))
    assert _call_b(two, kf) == ARG                            # the single side must be one frame
    assert "SearchByBoW" in mcs_amd.lib().mcs_last_error().decode()


def test_host_entries_zero_sizes_succeed(built):
    """n_kf == 0, n_f == 0 and empty keyframes give zero matches without any device."""
    from mcs_amd import bow_match as bm
    f, kf, e = a_frames("a3")
    empty = dict(desc=np.zeros((0, 32), np.uint8), has_mp=np.zeros(0, np.uint8), fv={})
    m, n = bm.search_by_bow(f, [], th=e["th"])
    assert m.shape == (0, 60) and n.shape == (0,)
    m, n = bm.search_by_bow(empty, [kf], th=e["th"])
    assert m.shape == (1, 0) and n.tolist() == [0]
    m, n = bm.search_by_bow(f, [empty, empty], th=e["th"])
    assert (m == -1).all() and n.tolist() == [0, 0]
    m, n = bm.search_by_bow_kf(kf, [], th=e["th"])
    assert m.shape == (0, 60) and n.shape == (0,)
    m, n = bm.search_by_bow_kf(kf, [empty], th=e["th"])
    assert (m == -1).all() and n.tolist() == [0]


def build_demo(tmp_path):
    lib = os.path.join(ROOT, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / "bow_match_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "bow_match_demo.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib, "-lmcs_amd",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_demo_compiles_against_adapter_header(built, tmp_path):
    assert os.path.exists(build_demo(tmp_path))
