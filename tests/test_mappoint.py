"""Map-point refresh after the LocalBA write-back (src/cOptimizer.cpp:885-902), batched on the
device (include/mcs_mappoint.h), against the oracle's literal restatements:

  ComputeDistinctiveDescriptors  src/cMapPoint.cpp:297-390 -- exact (integer distances, the
      upper-triangle-row median quirk: row i only sees j > i, row N-1 never counts, N <= 2 -> 0)
  UpdateNormalAndDepth           src/cMapPoint.cpp:453-496 -- bitwise (the same correctly
      rounded + - * / sqrt in the reference's order)
and, at the kernels' edge shapes, against NumPy references that do not go through the oracle
(second half of this file); tests/test_mapside_ref.py holds both to the reference text.
"""
import ctypes

import numpy as np
import pytest

from tests import oracle_bind as ob


def _descs(n, nb, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, nb), dtype=np.uint8)


def _observations(counts, nrows, seed):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = rng.integers(0, nrows, int(ptr[-1])).astype(np.int32)
    return ptr, rows


def _oracle_distinctive(desc, masks, nb, ptr, rows):
    best = np.zeros(len(ptr) - 1, np.int32)
    ob.lib().oracle_distinctive_descriptors(ob._p(desc), ob._p(masks), nb, ob._p(ptr), ob._p(rows),
                                            len(ptr) - 1, ob._p(best))
    return best


def test_oracle_median_quirk_by_hand(built):
    """N = 4 descriptors 0, A, B, C: row 0 sees {d01, d02, d03} (median = 2nd smallest), row 1
    {d12, d13} (median = the larger), row 2 {d23}; row 3 is never a candidate."""
    nb = 32
    base = np.zeros((4, nb), np.uint8)
    base[1, :2] = 0xFF     # d01 = 16
    base[2, :1] = 0xFF     # d02 = 8, d12 = 8
    base[3, 2:5] = 0xFF    # d03 = 24, d13 = 40, d23 = 32
    ptr = np.array([0, 4], np.int32)
    rows = np.arange(4, dtype=np.int32)
    # medians: row 0 -> sorted (8, 16, 24)[1] = 16; row 1 -> (8, 40)[1] = 40; row 2 -> 32
    assert _oracle_distinctive(base, None, nb, ptr, rows)[0] == 0
    base[3] = base[2]      # now d23 = 0: row 2's median 0 wins
    assert _oracle_distinctive(base, None, nb, ptr, rows)[0] == 2
    for n in (0, 1, 2):    # N <= 2 -> index 0, N = 0 -> nothing (-1)
        assert _oracle_distinctive(base, None, nb, np.array([0, n], np.int32), rows[:n])[0] == \
            (-1 if n == 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,masked", [(32, False), (16, False), (64, False), (32, True)])
def test_gpu_distinctive_descriptors(gpu, nb, masked):
    import torch
    import mcs_amd
    # clustered descriptors (a few prototypes + noise) so medians differ and ties occur
    rng = np.random.default_rng(nb + 7 * masked)
    proto = _descs(40, nb, 11)
    nrows = 4000
    pick = rng.integers(0, 40, nrows)
    flips = rng.random((nrows, nb * 8)) < rng.choice([0.02, 0.1, 0.3], nrows)[:, None]
    desc = proto[pick] ^ np.packbits(flips, axis=1)
    masks = (_descs(nrows, nb, 5) | _descs(nrows, nb, 6)) if masked else None
    counts = np.concatenate([[0, 1, 2, 3, 4, 5, 63, 64, 65, 130, 200],
                             rng.integers(2, 30, 500)])
    ptr, rows = _observations(counts, nrows, 3)
    ref = _oracle_distinctive(desc, masks, nb, ptr, rows)
    dev = torch.device("cuda", 0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d_desc = torch.from_numpy(desc).to(dev)
    d_mask = torch.from_numpy(masks).to(dev) if masked else None
    d_ptr, d_rows = torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev)
    n = len(counts)
    d_best = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_od = torch.zeros((n, nb), dtype=torch.uint8, device=dev)
    d_om = torch.zeros((n, nb), dtype=torch.uint8, device=dev)
    rc = mcs_amd.lib().mcs_distinctive_descriptors_device(P(d_desc), P(d_mask), nb, P(d_ptr), P(d_rows),
                                                          n, P(d_best), P(d_od), P(d_om), None)
    assert rc == 0
    torch.cuda.synchronize()
    best = d_best.cpu().numpy()
    assert np.array_equal(best, ref)
    od = d_od.cpu().numpy()
    for p in range(n):
        if ref[p] >= 0:
            assert np.array_equal(od[p], desc[rows[ptr[p] + ref[p]]]), p
            if masked:
                assert np.array_equal(d_om[p].cpu().numpy(), masks[rows[ptr[p] + ref[p]]]), p
        else:
            assert not od[p].any()


@pytest.mark.gpu
def test_gpu_update_normal_depth(gpu):
    import torch
    import mcs_amd
    rng = np.random.default_rng(21)
    n, nkf, nlev = 3000, 40, 8
    pts = rng.normal(0, 3, (n, 3))
    kfc = rng.normal(0, 1, (nkf, 3))
    counts = rng.integers(0, 9, n)
    counts[:3] = [0, 1, 2]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs = rng.integers(0, nkf, int(ptr[-1])).astype(np.int32)
    ref = rng.integers(0, nkf, n).astype(np.int32)
    lvl = rng.integers(-1, nlev, n).astype(np.int32)
    sf = float(np.float32(1.2))
    scale = np.cumprod([1.0] + [sf] * (nlev - 1))          # mvScaleFactors
    on, omin, omax = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    ob.lib().oracle_update_normal_depth(ob._p(pts), n, ob._p(ptr), ob._p(obs), ob._p(kfc), ob._p(ref),
                                        ob._p(lvl), ob._p(scale), nlev, ob._p(on), ob._p(omin), ob._p(omax))
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    d = [T(pts), T(ptr), T(obs), T(kfc), T(ref), T(lvl), T(scale)]
    dn = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    dmin = torch.zeros(n, dtype=torch.float64, device=dev)
    dmax = torch.zeros(n, dtype=torch.float64, device=dev)
    rc = mcs_amd.lib().mcs_update_normal_depth_device(P(d[0]), n, P(d[1]), P(d[2]), P(d[3]), P(d[4]),
                                                      P(d[5]), P(d[6]), nlev, P(dn), P(dmin), P(dmax), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), on)
    assert np.array_equal(dmin.cpu().numpy(), omin)
    assert np.array_equal(dmax.cpu().numpy(), omax)
    assert not dn[0].any().item()   # no observation: untouched


# ------------------------------------------------------------------ edge shapes, NumPy references
def np_distinctive(desc, masks, ptr, rows):
    """ComputeDistinctiveDescriptors in plain NumPy, independent of the oracle: distances by
    np.unpackbits (masked: (popcount(x & ma) + popcount(x & mb)) // 2), per row i < N - 1 the
    element (N - 1 - i) >> 1 of sorted(d[i, i+1:]), the first strict minimum wins.
    -> (best, all row medians, whether any masked pair had an odd popcount sum)."""
    best, medians, odd = [], [], False
    for p in range(len(ptr) - 1):
        r = rows[ptr[p]:ptr[p + 1]]
        N = len(r)
        if N <= 2:
            best.append(-1 if N == 0 else 0)
            continue
        bits = np.unpackbits(desc[r], axis=1).astype(bool)
        x = bits[:, None, :] ^ bits[None, :, :]
        if masks is None:
            d = x.sum(-1)
        else:
            mb = np.unpackbits(masks[r], axis=1).astype(bool)
            s = (x & mb[:, None, :]).sum(-1) + (x & mb[None, :, :]).sum(-1)
            odd = odd or bool((s % 2).any())
            d = s // 2
        bi, bm = 0, None
        for i in range(N - 1):
            med = int(sorted(d[i, i + 1:].tolist())[(N - 1 - i) >> 1])
            medians.append(med)
            if bm is None or med < bm:
                bi, bm = i, med
        best.append(bi)
    return np.array(best, np.int32), medians, odd


def _edge_points(nb, mode):
    """Descriptor rows and per-point lists: N = 0, 1, 2, then 3, 63, 64, 65, 66 (one and two
    64-column chunks of a row), 128, 129, 193, then all-equal rows (every median 0) and
    A, ~A, ~A (row 0's median 8 * bytes: both ends of the kernel's bisection).
    mode: "plain" (no masks), "masked" (random masks), "ones" (all-ones masks)."""
    rng = np.random.default_rng(100 + nb)
    sizes = [0, 1, 2, 3, 63, 64, 65, 66, 128, 129, 193]
    proto = _descs(6, nb, 12)
    n_rand = sum(sizes)
    flips = rng.random((n_rand, nb * 8)) < rng.choice([0.02, 0.1, 0.3], n_rand)[:, None]
    desc = proto[rng.integers(0, 6, n_rand)] ^ np.packbits(flips, axis=1)
    a = _descs(1, nb, 13)
    desc = np.concatenate([desc, np.repeat(a, 5, 0), a, ~a, ~a])
    masks = None
    if mode == "masked":
        masks = np.packbits(rng.random((len(desc), nb * 8)) < 0.8, axis=1)
        masks[n_rand:] = 255                       # the constructed rows keep their distances
    elif mode == "ones":
        masks = np.full_like(desc, 255)
    counts = sizes + [5, 3]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = np.concatenate([rng.permutation(n_rand), np.arange(n_rand, len(desc))]).astype(np.int32)
    return desc, masks, ptr, rows


def _run_distinctive(desc, masks, nb, ptr, rows, n_points, with_out=True, pad=3):
    """The device entry point on the first n_points lists; outputs are `pad` points longer and
    pre-filled, so a wave of the last block that has no point must leave the tail alone."""
    import torch
    import mcs_amd
    dev = torch.device("cuda", 0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d_desc = torch.from_numpy(desc).to(dev)
    d_mask = torch.from_numpy(masks).to(dev) if masks is not None else None
    d_ptr, d_rows = torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev)
    d_best = torch.full((n_points + pad,), -7, dtype=torch.int32, device=dev)
    d_od = torch.full((n_points + pad, nb), 0x5A, dtype=torch.uint8, device=dev) if with_out else None
    d_om = torch.full((n_points + pad, nb), 0x5A, dtype=torch.uint8, device=dev) if with_out else None
    rc = mcs_amd.lib().mcs_distinctive_descriptors_device(P(d_desc), P(d_mask), nb, P(d_ptr), P(d_rows),
                                                          n_points, P(d_best), P(d_od), P(d_om), None)
    assert rc == 0
    torch.cuda.synchronize()
    best = d_best.cpu().numpy()
    assert (best[n_points:] == -7).all()
    if not with_out:
        return best[:n_points], None, None
    od, om = d_od.cpu().numpy(), d_om.cpu().numpy()
    assert (od[n_points:] == 0x5A).all() and (om[n_points:] == 0x5A).all()
    return best[:n_points], od[:n_points], om[:n_points]


def _check_outputs(best, od, om, desc, masks, ptr, rows):
    for p, b in enumerate(best):
        if b < 0:
            assert (od[p] == 0x5A).all() and (om[p] == 0x5A).all(), p
            continue
        r = rows[ptr[p] + b]
        assert np.array_equal(od[p], desc[r]), p
        assert np.array_equal(om[p], masks[r]) if masks is not None else (om[p] == 0x5A).all(), p


def test_numpy_distinctive_reference_covers_the_edges():
    """The NumPy reference agrees with the by-hand case above, and the edge lists do contain
    what they are meant to: medians 0 and 8 * bytes, and odd masked popcount sums."""
    nb = 32
    base = np.zeros((4, nb), np.uint8)
    base[1, :2], base[2, :1], base[3, 2:5] = 0xFF, 0xFF, 0xFF
    ptr, rows = np.array([0, 4], np.int32), np.arange(4, dtype=np.int32)
    best, med, _ = np_distinctive(base, None, ptr, rows)
    assert best[0] == 0 and med == [16, 40, 32]
    for nb in (16, 32, 64):
        desc, masks, ptr, rows = _edge_points(nb, "masked")
        best, med, odd = np_distinctive(desc, masks, ptr, rows)
        assert odd and 0 in med and 8 * nb in med
        assert best[-2] == 0 and best[-1] == 1 and list(best[:3]) == [-1, 0, 0]


@pytest.mark.parametrize("nb", [16, 32, 64])
@pytest.mark.parametrize("mode", ["plain", "masked", "ones"])
def test_oracle_distinctive_edge_shapes(built, nb, mode):
    """The oracle restatement on the same edge lists (CPU)."""
    desc, masks, ptr, rows = _edge_points(nb, mode)
    assert np.array_equal(_oracle_distinctive(desc, masks, nb, ptr, rows), np_distinctive(desc, masks, ptr, rows)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [16, 32, 64])
@pytest.mark.parametrize("mode", ["plain", "masked", "ones"])
def test_gpu_distinctive_edge_shapes(gpu, nb, mode):
    desc, masks, ptr, rows = _edge_points(nb, mode)
    n = len(ptr) - 1                                # 13 points: the last block has one wave busy
    ref, med, odd = np_distinctive(desc, masks, ptr, rows)
    assert 0 in med and 8 * nb in med and (odd or mode != "masked")
    best, od, om = _run_distinctive(desc, masks, nb, ptr, rows, n)
    assert np.array_equal(best, ref)
    _check_outputs(best, od, om, desc, masks, ptr, rows)
    if mode == "ones":                              # an all-ones mask is the unmasked distance
        assert np.array_equal(ref, np_distinctive(desc, None, ptr, rows)[0])
        assert np.array_equal(best, _run_distinctive(desc, None, nb, ptr, rows, n)[0])
    # d_out_desc / d_out_mask NULL: only the index is written
    assert np.array_equal(_run_distinctive(desc, masks, nb, ptr, rows, n, with_out=False)[0], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n_points", [1, 5, 7])
@pytest.mark.parametrize("nb,mode", [(16, "masked"), (32, "plain"), (64, "masked")])
def test_gpu_distinctive_points_off_the_block_grid(gpu, n_points, nb, mode):
    """n_points = 1, 5, 7 with four waves (points) per block: waves without a point."""
    desc, masks, ptr, rows = _edge_points(nb, mode)
    keep = [3, 4, 12, 0, 6, 11, 5][:n_points]       # N = 3, 63, (A, ~A, ~A), 0, 65, 5 equal, 64
    counts = np.diff(ptr)[keep]
    sub_rows = np.concatenate([rows[ptr[k]:ptr[k + 1]] for k in keep] + [np.zeros(0, np.int32)]).astype(np.int32)
    sub_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ref = np_distinctive(desc, masks, sub_ptr, sub_rows)[0]
    best, od, om = _run_distinctive(desc, masks, nb, sub_ptr, sub_rows, n_points)
    assert np.array_equal(best, ref)
    _check_outputs(best, od, om, desc, masks, sub_ptr, sub_rows)


def np_normal_depth(pts, ptr, obs, kfc, ref, lvl, scale, normal, dmin, dmax):
    """UpdateNormalAndDepth in NumPy float64, one correctly rounded operation at a time in the
    reference's order (no np.sum, no linalg.norm): ((x*x + y*y) + z*z), 1.0 / sqrt, v * (1.0 / a)."""
    f = np.float64
    nlev = len(scale)

    def norm(a):
        return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    for p in range(len(pts)):
        if ptr[p + 1] <= ptr[p]:
            continue
        X = [f(v) for v in pts[p]]
        n = [f(0.0)] * 3
        cnt = 0
        for q in range(ptr[p], ptr[p + 1]):
            a = [X[k] - f(kfc[obs[q], k]) for k in range(3)]
            ia = f(1.0) / norm(a)
            n = [n[k] + a[k] * ia for k in range(3)]
            cnt += 1
        dist = norm([X[k] - f(kfc[ref[p], k]) for k in range(3)])
        level = int(lvl[p]) if lvl[p] >= 0 else 1
        sf = f(scale[level])
        dmin[p] = (f(1.0) / sf) * dist / sf
        dmax[p] = sf * dist * f(scale[nlev - 1 - level])
        inv = f(1.0) / f(cnt)
        normal[p] = [n[k] * inv for k in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("nlev", [2, 8])
def test_gpu_update_normal_depth_edge_shapes(gpu, n, nlev):
    """n_points 1 and 257 (one thread of a second block), n_levels 2 and 8, ref_level -1 / 0 /
    n_levels - 1 (the latter reads scale[0]), 0 / 1 / 9 observing keyframes, a keyframe twice
    in one list -- bitwise against the NumPy reference."""
    import torch
    import mcs_amd
    rng = np.random.default_rng(50 + n + nlev)
    nkf = 12
    pts = rng.normal(0, 3, (n, 3))
    kfc = rng.normal(0, 1, (nkf, 3))
    counts = np.array(([9, 0, 1] * 86)[:n])
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs = rng.integers(0, nkf, int(ptr[-1])).astype(np.int32)
    obs[1] = obs[0]                                         # the same keyframe twice
    ref = rng.integers(0, nkf, n).astype(np.int32)
    lvl = np.array(([nlev - 1, 0, -1, 0, -1, nlev - 1, -1, nlev - 1, 0] * 29)[:n], np.int32)
    sf = float(np.float32(1.2))
    scale = np.cumprod([1.0] + [sf] * (nlev - 1))
    rn, rmin, rmax = np.full((n, 3), 9.0), np.full(n, -1.0), np.full(n, -2.0)
    np_normal_depth(pts, ptr, obs, kfc, ref, lvl, scale, rn, rmin, rmax)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    d = [T(pts), T(ptr), T(obs), T(kfc), T(ref), T(lvl), T(scale)]
    dn, dmin, dmax = T(np.full((n + 2, 3), 9.0)), T(np.full(n + 2, -1.0)), T(np.full(n + 2, -2.0))
    rc = mcs_amd.lib().mcs_update_normal_depth_device(P(d[0]), n, P(d[1]), P(d[2]), P(d[3]), P(d[4]),
                                                      P(d[5]), P(d[6]), nlev, P(dn), P(dmin), P(dmax), None)
    assert rc == 0
    torch.cuda.synchronize()
    gn, gmin, gmax = dn.cpu().numpy(), dmin.cpu().numpy(), dmax.cpu().numpy()
    assert gn[:n].tobytes() == rn.tobytes()
    assert gmin[:n].tobytes() == rmin.tobytes() and gmax[:n].tobytes() == rmax.tobytes()
    assert (gn[n:] == 9.0).all() and (gmin[n:] == -1.0).all() and (gmax[n:] == -2.0).all()
    if n > 1:
        assert (gn[1] == 9.0).all() and gmin[1] == -1.0      # no observing keyframe: untouched


def test_numpy_normal_depth_reference_agrees_with_oracle(built):
    """The NumPy reference the GPU edge-shape test uses equals the oracle bitwise (CPU)."""
    rng = np.random.default_rng(8)
    n, nkf, nlev = 120, 12, 8
    pts, kfc = rng.normal(0, 3, (n, 3)), rng.normal(0, 1, (nkf, 3))
    counts = rng.integers(0, 10, n)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs = rng.integers(0, nkf, int(ptr[-1])).astype(np.int32)
    ref = rng.integers(0, nkf, n).astype(np.int32)
    lvl = rng.integers(-1, nlev, n).astype(np.int32)
    scale = np.cumprod([1.0] + [float(np.float32(1.2))] * (nlev - 1))
    rn, rmin, rmax = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    np_normal_depth(pts, ptr, obs, kfc, ref, lvl, scale, rn, rmin, rmax)
    on, omin, omax = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    ob.lib().oracle_update_normal_depth(ob._p(pts), n, ob._p(ptr), ob._p(obs), ob._p(kfc), ob._p(ref),
                                        ob._p(lvl), ob._p(scale), nlev, ob._p(on), ob._p(omin), ob._p(omax))
    assert on.tobytes() == rn.tobytes() and omin.tobytes() == rmin.tobytes() and omax.tobytes() == rmax.tobytes()
