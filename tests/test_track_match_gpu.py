"""The tracking matchers with nothing downloaded (include/mcs_matcher.h device form,
csrc/track_match.hip): the cMultiFrame grid on the device, the queries of
SearchByProjection(F, MPs) (rule 0) and SearchByProjection(Current, Last) (rule 1) from device
data, and the ordered selection of rules 0, 1 and 3 in one launch.

Expected values: the oracle (oracle_frame_grid, oracle_window_match, oracle_is_in_frustum) and,
as a second witness, the host entries mcs_frame_grid_build / mcs_window_select.  Every
comparison is exact: ints, and doubles bit for bit through .view(np.int64).
"""
import ctypes

import numpy as np
import pytest

from tests import oracle_bind as ob
from tests import test_window as tw

pytestmark = pytest.mark.gpu

NC, W, H = tw.NC, tw.W, tw.H
NCELL = NC * 64 * 48


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------ grid
def _oracle_grid(gp, xy, cam):
    ptr = np.zeros(len(gp) * 64 * 48 + 1, np.int32)
    cells = np.zeros(max(len(xy), 1), np.int32)
    n = ob.lib().oracle_frame_grid(len(gp), tw._p(gp), tw._p(xy), tw._p(cam), len(xy), tw._p(ptr), tw._p(cells))
    ptr[-1] = n
    return ptr, cells[:n]


def _device_grid(ws, gp, xy, cam, count=None):
    import torch
    d_n = None if count is None else _t(np.array([count], np.int32))
    cap = len(xy)
    d_xy = _t(xy) if cap else torch.zeros((0, 2), dtype=torch.float32, device="cuda")
    d_cam = _t(cam) if cap else torch.zeros(0, dtype=torch.int32, device="cuda")
    ptr, cells, nin = ws.grid_build(d_xy, d_cam, _t(gp), d_n)
    torch.cuda.synchronize()
    return ptr.cpu().numpy(), cells.cpu().numpy(), int(nin.cpu()[0])


def _check_grid(ws, gp, xy, cam, count=None):
    from mcs_amd import window as mw
    n = len(xy) if count is None else count
    optr, ocell = _oracle_grid(gp, xy[:n], cam[:n])
    hptr, hcell = mw.grid_build(xy[:n], cam[:n], gp)
    assert np.array_equal(hptr, optr) and np.array_equal(hcell, ocell)
    ptr, cells, nin = _device_grid(ws, gp, xy, cam, count)
    assert nin == len(ocell)
    assert np.array_equal(ptr, optr)
    assert np.array_equal(cells[:nin], ocell)
    return nin


@pytest.fixture(scope="module")
def ws(gpu):
    from mcs_amd import track_match as tm
    w = tm.Workspace(8200, 2600, 400000)
    yield w
    w.close()


@pytest.mark.parametrize("n_kp", [0, 1, 63, 64, 65, 4097])
def test_grid_matches_oracle(ws, n_kp):
    fr = tw._frame(1)           # cell-boundary ties, integer positions, positions outside the image
    nin = _check_grid(ws, fr["gp"], fr["xy"][:n_kp].copy(), fr["cam"][:n_kp].copy())
    assert nin <= n_kp and (n_kp < 64 or nin > n_kp // 2)


def test_grid_camera_out_of_range_and_long_cell(ws):
    fr = tw._frame(2, n_kp=1000)
    cam = fr["cam"].copy()
    cam[5], cam[6], cam[7] = NC, -1, 1 << 20
    xy = fr["xy"].copy()
    rng = np.random.default_rng(3)
    idx = rng.choice(np.arange(400, 1000), 300, replace=False)     # 300 keypoints in one cell of camera 1
    xy[idx] = (200.0 + rng.uniform(-2, 2, (300, 2))).astype(np.float32)
    cam[idx] = 1
    nin = _check_grid(ws, fr["gp"], xy, cam)
    ptr, _ = _oracle_grid(fr["gp"], xy, cam)
    assert np.diff(ptr).max() >= 300 and nin < 1000


def test_grid_device_count_below_capacity(ws):
    import torch
    from mcs_amd import lib
    fr = tw._frame(4, n_kp=700)
    xy, cam = fr["xy"].copy(), fr["cam"].copy()
    # slots past the count hold keypoints the grid would take: reading one changes cell_ptr,
    # cell_kp and n_in_grid
    xy[500:] = np.random.default_rng(5).uniform([20, 20], [W - 20, H - 20], (200, 2)).astype(np.float32)
    cam[500:] = np.arange(200) % NC
    assert len(_oracle_grid(fr["gp"], xy, cam)[1]) >= len(_oracle_grid(fr["gp"], xy[:500], cam[:500])[1]) + 200
    nin = _check_grid(ws, fr["gp"], xy, cam, count=500)
    assert 0 < nin <= 500
    # canaries: cell_kp past n_in_grid and the words after cell_ptr stay as they were
    d_xy, d_cam, d_gp, d_n = _t(xy), _t(cam), _t(fr["gp"]), _t(np.array([500], np.int32))
    ptr = torch.full((NCELL + 1 + 32,), -77, dtype=torch.int32, device="cuda")
    cells = torch.full((700 + 32,), -77, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib().mcs_frame_grid_build_device(ws._h, P(d_xy), P(d_cam), P(d_n), 700, NC, P(d_gp), P(ptr), P(cells),
                                             None, None) == 0
    torch.cuda.synchronize()
    optr, ocell = _oracle_grid(fr["gp"], xy[:500], cam[:500])
    assert np.array_equal(ptr.cpu().numpy()[:NCELL + 1], optr) and (ptr[NCELL + 1:] == -77).all()
    assert np.array_equal(cells.cpu().numpy()[:nin], ocell) and (cells[nin:] == -77).all()
    # a count beyond the capacity is clamped to it
    ptr3, cells3, n3 = ws.grid_build(_t(fr["xy"]), _t(fr["cam"]), d_gp, _t(np.array([1 << 30], np.int32)))
    torch.cuda.synchronize()
    optr, ocell = _oracle_grid(fr["gp"], fr["xy"], fr["cam"])
    assert np.array_equal(ptr3.cpu().numpy(), optr) and np.array_equal(cells3.cpu().numpy()[:len(ocell)], ocell)


# --------------------------------------------------------------------------------- queries
_FRUSTUM = {}


def _frustum_case():
    """~500 points x 3 cameras on the Lafida rig through the oracle's isInFrustum, shared."""
    if "c" not in _FRUSTUM:
        from tests import test_frame as tf
        pose, mc, cam, masks, pts, nrm, dist, scale = tf._frustum_inputs(11, n=900)
        pts = np.ascontiguousarray(pts[400:])               # 400 map-like points and 100 random ones
        nrm, dist = nrm[400:].copy(), dist[400:].copy()
        d = np.linalg.norm(pts - pose[3:], axis=1)
        nrm[:150] = (pts[:150] - pose[3:]) / d[:150, None]  # seen head-on: viewCos close to 1
        dist[:, 0] = d / np.linspace(0.7, 4.0, len(pts))    # predicted levels 0 .. top
        dist[:, 1] = d * 3.0
        iv, pj, lv, vc = tf._oracle_frustum(pose, mc, cam, masks, pts, nrm, dist, scale)
        _FRUSTUM["c"] = dict(pose=pose, mc=np.ascontiguousarray(mc), cam=np.ascontiguousarray(cam), masks=masks,
                             pts=pts, nrm=nrm, dist=dist, scale=scale, iv=iv, pj=pj, lv=lv, vc=vc)
    return _FRUSTUM["c"]


def _rule0_expected(iv, pj, lv, vc, skip, scale, th):
    """SearchByProjection(F, MPs): the pure function of isInFrustum's outputs."""
    n, C = iv.shape
    live = (iv == 1) & (skip[:, None] == 0)
    r = np.where(vc > 0.998, 2.5, 4.0)
    if th != 1.0:
        r = r * th
    r = r * scale[np.where(live, lv, 0)]
    xyr = np.zeros((n, C, 3))
    xyr[..., :2] = pj
    xyr[..., 2] = r
    xyr[~live] = 0.0
    cl = np.stack([np.broadcast_to(np.arange(C), (n, C)), lv - 1, lv], -1).astype(np.int32)
    cl[~live] = -1
    idx = np.repeat(np.arange(n, dtype=np.int32), C)
    return xyr.reshape(-1, 3), cl.reshape(-1, 3), idx


@pytest.mark.parametrize("th", [1.0, 3.0])
def test_rule0_queries_equal_the_text(gpu, th):
    import torch
    from mcs_amd import track_match as tm
    z = _frustum_case()
    iv, pj, vc = z["iv"], z["pj"], z["vc"]
    sel = iv == 1
    lv = z["lv"].copy()
    lv[::7] = 0          # isInFrustum gives level 0 only at ratio exactly 1: set here (minLevel = -1)
    assert sel.sum() > 150 and (vc[sel] > 0.998).sum() > 10 and (vc[sel] <= 0.998).sum() > 10
    assert (lv[sel] == 0).sum() > 3 and (lv[sel] == len(z["scale"]) - 1).sum() > 3
    skip = (np.random.default_rng(5).random(len(iv)) < 0.2).astype(np.uint8)
    assert (sel & (skip[:, None] == 1)).sum() > 5
    want = _rule0_expected(iv, pj, lv, vc, skip, z["scale"], th)
    got = tm.queries_mappoints(_t(iv), _t(pj), _t(lv), _t(vc), _t(z["scale"]), th, skip=_t(skip))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want[0]))
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])
    # a level outside the scale table is an empty window, not a read past the table
    lv2 = lv.copy()
    lv2[sel] = np.where(np.arange(sel.sum()) % 2 == 0, 99, -3)
    got = tm.queries_mappoints(_t(iv), _t(pj), _t(lv2), _t(vc), _t(z["scale"]), th)
    torch.cuda.synchronize()
    assert (got[1].cpu().numpy() == -1).all()


def _rule1_case():
    z = _frustum_case()
    rng = np.random.default_rng(6)
    n = len(z["pts"])
    kp_cam = rng.integers(0, NC, n).astype(np.int32)
    octv = rng.integers(0, 8, n).astype(np.int32)
    octv[:20] = 0
    octv[20:40] = 7
    valid = (rng.random(n) < 0.85).astype(np.uint8)
    from tests import test_frame as tf
    wide = np.tile(np.array([1e-300, 1e300]), (n, 1))       # a distance range that gates nothing
    iv, pj, _, _ = tf._oracle_frustum(z["pose"], z["mc"], z["cam"], z["masks"], z["pts"], z["nrm"], wide, z["scale"])
    return z, kp_cam, octv, valid, iv, pj


def _rule1_device(z, kp_cam, octv, valid, th, count=None):
    import torch
    from mcs_amd import track_match as tm
    d_n = None if count is None else _t(np.array([count], np.int32))
    got = tm.queries_lastframe(_t(z["pose"]), _t(z["mc"]), _t(z["cam"]), _t(z["masks"]), _t(z["pts"]), _t(valid),
                               _t(kp_cam), _t(octv), _t(z["scale"]), th, n=d_n)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def test_rule1_queries_verdict_radius_levels(gpu):
    """Which slots give a query (valid, the oracle's mirror verdict in the slot's own camera), the
    radius th * scale[octave] bit for bit, the levels and the descriptor index."""
    z, kp_cam, octv, valid, iv, pj = _rule1_case()
    n = len(kp_cam)
    own = iv[np.arange(n), kp_cam] == 1
    live = own & (valid == 1)
    assert live.sum() > 100 and (~own & (valid == 1)).sum() > 10 and (valid == 0).sum() > 10
    assert (live & (octv == 0)).sum() > 2 and (live & (octv == 7)).sum() > 2
    xyr, cl, idx = _rule1_device(z, kp_cam, octv, valid, 15.0)
    assert np.array_equal(cl[:, 0], np.where(live, kp_cam, -1))
    assert np.array_equal(cl[live, 1], octv[live] - 1) and np.array_equal(cl[live, 2], octv[live] + 1)
    assert np.array_equal(_bits(xyr[live, 2]), _bits(15.0 * z["scale"][octv[live]]))
    assert (xyr[~live] == 0).all() and np.array_equal(idx, np.arange(n))
    # slots past the device count, cameras and octaves out of range: no query
    cam2, oct2 = kp_cam.copy(), octv.copy()
    cam2[:5], oct2[5:10] = [NC, -1, 9, 1 << 20, -7], [8, -1, 99, 1 << 20, -5]
    xyr2, cl2, _ = _rule1_device(z, cam2, oct2, valid, 15.0, count=300)
    assert (cl2[:10, 0] == -1).all() and (cl2[300:, 0] == -1).all()
    assert np.array_equal(cl2[10:300], cl[10:300])


def test_rule1_queries_projection_bits(gpu):
    """The projection of every live slot equals the oracle's isInFrustum projection in the slot's
    own camera bit for bit.  WorldToImg takes atan(-z / norm); the oracle calls the host libm's,
    and the rule 1 kernel a correctly rounded one (csrc/atan_cr.hpp), which is the same number
    except where the libm misrounds: about 2.5 arguments in ten thousand, one ulp apart
    (test_atan_cr_against_libm).  None of this scene's 200 angles is one of them with glibc
    2.35's libm; with another libm under the oracle one could be, and the coordinate would then
    be an ulp or two off.  (The device library's own atan put 15 of these
    400 coordinates off.)  Every other operation of the projection is correctly rounded on both
    sides."""
    z, kp_cam, octv, valid, iv, pj = _rule1_case()
    n = len(kp_cam)
    live = (iv[np.arange(n), kp_cam] == 1) & (valid == 1)
    xyr, cl, _ = _rule1_device(z, kp_cam, octv, valid, 7.0)
    assert np.array_equal(cl[:, 0] >= 0, live)
    own = pj[np.arange(n), kp_cam]
    diff = np.abs(xyr[live, :2] - own[live])
    print("rule 1 projection vs oracle: max abs diff %.3e px, %d of %d values differ"
          % (diff.max(), int((diff != 0).sum()), diff.size))
    assert np.array_equal(_bits(xyr[live, :2]), _bits(own[live]))


# ------------------------------------------------------------- selection and the whole entry
def _device_frame(ws, fr):
    from mcs_amd import track_match as tm
    d_gp, d_xy = _t(fr["gp"]), _t(fr["xy"])
    ptr, cells, _ = ws.grid_build(d_xy, _t(fr["cam"]), d_gp)
    return tm.DeviceFrame(d_gp, d_xy, _t(fr["oct"]), _t(fr["desc"]), ptr, cells,
                          None if fr["mask"] is None else _t(fr["mask"]))


def _search(ws, frame, rule, xyr, cl, qd, qm, a0, th, ratio, permute=False):
    """The device entry; permute: the descriptors through a shuffled source and its index."""
    import torch
    nq = len(xyr)
    idx = None
    if permute and nq:
        perm = np.random.default_rng(nq).permutation(nq)
        qd = qd[perm]
        qm = None if qm is None else qm[perm]
        idx = _t(np.argsort(perm).astype(np.int32))
    if nq == 0:
        qd = np.zeros((1, frame.bytes), np.uint8)
        qm = None if qm is None else np.zeros((1, frame.bytes), np.uint8)
    d_a = _t(a0)
    d_xyr = _t(xyr) if nq else torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    d_cl = _t(cl) if nq else torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    m, kq, n, st = ws.search(rule, frame, d_xyr, d_cl, _t(qd), th, ratio, d_a, q_desc_idx=idx,
                             q_mask_src=None if qm is None else _t(qm))
    torch.cuda.synchronize()
    return m.cpu().numpy(), kq.cpu().numpy(), int(n.cpu()[0]), d_a.cpu().numpy(), st.cpu().numpy()


def _for_oracle(xyr, cl):
    """The oracle indexes its grid by the query's camera: a camera outside the rig (the queries the
    reference would `continue` past) goes to it as a window far outside the image, also empty."""
    out = (cl[:, 0] < 0) | (cl[:, 0] >= NC)
    xyr, cl = xyr.copy(), cl.copy()
    xyr[out] = (-5000.0, -5000.0, 1.0)
    cl[out] = (0, -1, -1)
    return xyr, cl


def _check_match(fr, rule, xyr, cl, qd, qm, a0, got, ratio=None):
    m, kq, n, a, st = got
    ratio = tw.RATIO[rule] if ratio is None else ratio
    xyr, cl = _for_oracle(xyr, cl)
    a_o = a0.copy()
    m_o = np.full(max(len(xyr), 1), -7, np.int32)
    n_o = ob.lib().oracle_window_match(rule, *tw._frame_args(fr), len(xyr), tw._p(xyr), tw._p(cl), tw._p(qd),
                                       tw._p(qm), tw._th(fr, rule), ratio, tw._p(a_o), tw._p(m_o))
    m_o = m_o[:len(xyr)]
    assert n == n_o and np.array_equal(m, m_o) and np.array_equal(a, a_o)
    want_kq = np.full(len(a0), -1, np.int32)
    want_kq[m_o[m_o >= 0]] = np.nonzero(m_o >= 0)[0]
    assert np.array_equal(kq, want_kq)
    assert not (st[1] & 1)
    return n_o


@pytest.mark.parametrize("rule,nbytes,masks", [(0, 32, False), (1, 32, False), (3, 32, False), (0, 32, True),
                                               (1, 16, False), (3, 64, False)])
def test_search_matches_oracle(ws, rule, nbytes, masks):
    from mcs_amd import window as mw
    fr = tw._frame(60 + rule, nbytes=nbytes, masks=masks)
    xyr, cl, qd, qm = tw._queries(fr, rule, 70 + rule)
    a0 = tw._assigned0(fr, rule, 5)
    frame = _device_frame(ws, fr)
    got = _search(ws, frame, rule, xyr, cl, qd, qm, a0, tw._th(fr, rule), tw.RATIO[rule], permute=(nbytes == 32))
    assert _check_match(fr, rule, xyr, cl, qd, qm, a0, got) > 50
    # second witness: the host selection of the parent commit over the oracle's candidate lists
    ptr, kp, dist = tw._oracle_candidates(fr, xyr, cl, qd, qm)
    assert got[4][0] == len(kp)
    m_h, n_h, a_h = mw.window_select(rule, ptr, kp, dist, fr["oct"], tw._th(fr, rule), tw.RATIO[rule], a0)
    assert n_h == got[2] and np.array_equal(m_h, got[0]) and np.array_equal(a_h, got[3])


def _chain_case(rule, nq=300):
    """nq queries with the same window over the same ~40 keypoints: every query depends on all
    earlier ones."""
    rng = np.random.default_rng(80 + rule)
    fr = tw._frame(81, n_kp=600)
    fr["xy"][:40] = (np.array([300.0, 200.0]) + rng.uniform(-6, 6, (40, 2))).astype(np.float32)
    fr["cam"][:40] = 1
    far = np.abs(fr["xy"][40:] - [300.0, 200.0]).max(axis=1) < 40
    fr["cam"][40:][far] = 0
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in range(40):
        fr["desc"][k] = tw._flip(base, int(rng.integers(0, 50)), rng)
    xyr = np.tile(np.array([300.0, 200.0, 12.0]), (nq, 1))
    cl = np.tile(np.array([1, -1, -1], np.int32), (nq, 1))
    if rule == 0:
        cl[:, 1:] = (2, 3)
        fr["oct"][:40] = rng.integers(2, 4, 40)
    qd = np.stack([tw._flip(base, int(rng.integers(0, 40)), rng) for _ in range(nq)])
    return fr, xyr, cl, qd


@pytest.mark.parametrize("rule", [0, 1, 3])
def test_worst_case_chain(ws, rule):
    from mcs_amd import track_match as tm
    fr, xyr, cl, qd = _chain_case(rule)
    a0 = np.zeros(len(fr["xy"]), np.uint8)
    got = _search(ws, _device_frame(ws, fr), rule, xyr, cl, qd, None, a0, tw._th(fr, rule), tw.RATIO[rule])
    n = _check_match(fr, rule, xyr, cl, qd, None, a0, got)
    assert 1 <= n <= 40
    # one query settles per round while unassigned keypoints remain: the depth is nq
    assert tm.rounds(got[4][1]) == len(xyr) if n < 40 else n <= tm.rounds(got[4][1]) <= len(xyr)


@pytest.mark.parametrize("rule", [0, 1, 3])
def test_long_candidate_lists(ws, rule):
    """Windows of a hundred and more candidates per query, where the selection gives a query a
    wave and takes best / second as the two smallest (distance, position): equal distances from
    duplicate descriptors included."""
    rng = np.random.default_rng(170 + rule)
    fr = tw._frame(171 + rule)
    fr["desc"][1000:4000] = fr["desc"][rng.integers(0, 1000, 3000)]
    xyr, cl, qd, qm = tw._queries(fr, rule, 175 + rule, nq=600)
    xyr[:, 2] = 100.0 if rule == 0 else 70.0
    if rule != 0:
        cl[:, 1:] = -1
    ptr, kp, dist = tw._oracle_candidates(fr, xyr, cl, qd, None)
    lens = np.diff(ptr)
    for c in range(NC):          # every camera's workgroup is above the threshold of the wave path
        own = lens[(cl[:, 0] == c) & (lens > 0)]
        assert own.mean() >= 24 and own.max() > 64
    a0 = tw._assigned0(fr, rule, 13)
    got = _search(ws, _device_frame(ws, fr), rule, xyr, cl, qd, None, a0, tw._th(fr, rule), tw.RATIO[rule])
    assert _check_match(fr, rule, xyr, cl, qd, None, a0, got) > 20
    same = [q for q in range(600) if lens[q] > 1 and (np.sort(dist[ptr[q]:ptr[q + 1]])[:2] == dist[ptr[q]:ptr[q + 1]].min()).all()]
    assert len(same) > 5         # queries whose two best candidates are at the same distance


@pytest.mark.parametrize("nq", [0, 1, 1025, 2049])
def test_query_counts_around_the_workgroup(ws, nq):
    fr = tw._frame(90, n_kp=3000)
    xyr, cl, qd, _ = tw._queries(fr, 0, 91, nq=max(nq, 1))
    xyr, cl, qd = xyr[:nq], cl[:nq], qd[:nq]
    a0 = tw._assigned0(fr, 0, 7)
    got = _search(ws, _device_frame(ws, fr), 0, xyr, cl, qd, None, a0, tw._th(fr, 0), tw.RATIO[0])
    n = _check_match(fr, 0, xyr, cl, qd, None, a0, got)
    assert n >= nq // 8


def test_degenerate_queries(ws):
    fr = tw._frame(100, n_kp=3000)
    xyr, cl, qd, _ = tw._queries(fr, 3, 101, nq=400)
    xyr[:50, :2] = (-500.0, -500.0)            # no candidates
    cl[50:100, 0] = -1                         # the reference would `continue`
    cl[100:120, 0] = NC
    ptr, kp, _ = tw._oracle_candidates(fr, *_for_oracle(xyr, cl), qd, None)
    a0 = np.zeros(len(fr["xy"]), np.uint8)
    busy = [q for q in range(150, 400) if ptr[q + 1] - ptr[q] >= 2][:30]
    for q in busy:                             # every candidate already holds a point
        a0[kp[ptr[q]:ptr[q + 1]]] = 1
    frame = _device_frame(ws, fr)
    for rule in (3, 1, 0):
        got = _search(ws, frame, rule, xyr, cl, qd, None, a0, tw._th(fr, rule), tw.RATIO[rule], permute=True)
        assert _check_match(fr, rule, xyr, cl, qd, None, a0, got) > 20
        assert (got[0][:120] == -1).all() and (got[0][busy] == -1).all()
    # an index outside the descriptor source is an empty window
    import torch
    idx = np.arange(400, dtype=np.int32)
    idx[200:210] = [400, -1, 1 << 30, -(1 << 30), 401, 500, 999, -2, -3, 400]
    d_a = _t(a0)
    m, kq, n, st = ws.search(3, frame, _t(xyr), _t(cl), _t(qd), tw._th(fr, 3), tw.RATIO[3], d_a, q_desc_idx=_t(idx))
    torch.cuda.synchronize()
    cl2 = cl.copy()
    cl2[200:210, 0] = -1
    _check_match(fr, 3, xyr, cl2, qd, None, a0, (m.cpu().numpy(), kq.cpu().numpy(), int(n.cpu()[0]),
                                                  d_a.cpu().numpy(), st.cpu().numpy()))
    assert (m.cpu().numpy()[200:210] == -1).all()


def test_ties(ws):
    """Duplicate descriptors: the first in enumeration order wins under strict <.  Best and second
    at the same distance: rule 0 rejects them in the same octave and accepts across octaves."""
    rng = np.random.default_rng(110)
    fr = tw._frame(111, n_kp=500)
    fr["cam"][:] = 0
    fr["xy"][:] = (np.array([600.0, 400.0]) + rng.uniform(-30, 30, (500, 2))).astype(np.float32)
    spots = np.array([[100.0, 100.0], [300.0, 100.0], [500.0, 100.0]])
    q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    for s in range(3):
        k = 6 * s
        fr["xy"][k:k + 6] = (spots[s] + rng.uniform(-3, 3, (6, 2))).astype(np.float32)
        fr["desc"][k:k + 6] = rng.integers(0, 256, (6, 32), dtype=np.uint8)
        fr["oct"][k:k + 6] = 3
    fr["desc"][1] = fr["desc"][4] = tw._flip(q[0], 3, rng)                          # spot 0: duplicates
    fr["desc"][7], fr["desc"][10] = tw._flip(q[1], 5, rng), tw._flip(q[1], 5, rng)  # spot 1: tie, same octave
    fr["desc"][13], fr["desc"][16] = tw._flip(q[2], 5, rng), tw._flip(q[2], 5, rng)  # spot 2: tie, octaves 2 / 3
    fr["oct"][16] = 2
    xyr = np.concatenate([spots, np.full((3, 1), 8.0)], 1)
    cl = np.tile(np.array([0, 2, 3], np.int32), (3, 1))
    a0 = np.zeros(500, np.uint8)
    frame = _device_frame(ws, fr)
    got = _search(ws, frame, 0, xyr, cl, q, None, a0, tw._th(fr, 0), tw.RATIO[0])
    _check_match(fr, 0, xyr, cl, q, None, a0, got)
    ptr, kp, _ = tw._oracle_candidates(fr, xyr, cl, q, None)
    first = [[k for k in kp[ptr[s]:ptr[s + 1]] if k in pair][0] for s, pair in enumerate([(1, 4), (7, 10), (13, 16)])]
    assert got[0].tolist() == [-1, -1, first[2]]        # same octave: rejected; octaves 2 / 3: the first one
    got = _search(ws, frame, 1, xyr, cl, q, None, a0, tw._th(fr, 1), tw.RATIO[1])
    _check_match(fr, 1, xyr, cl, q, None, a0, got)
    assert got[0].tolist() == first                     # best only: the first of the equal ones
    got = _search(ws, frame, 3, xyr, cl, q, None, a0, tw._th(fr, 3), tw.RATIO[3])
    _check_match(fr, 3, xyr, cl, q, None, a0, got)
    assert got[0].tolist() == [-1, -1, -1]              # best <= 0.7 * second fails on a tie


@pytest.mark.parametrize("sc", [0, 1, 2])
def test_reference_fixture_through_the_device_entry(ws, sc):
    """The recorded reference calls of tests/golden/matcher_ref.npz (rules 0, 1 and 3) give the
    reference text's final assignment."""
    from tests import test_matcher_ref as mr
    z = mr._rename(mr._fix())
    f2 = mr._frame(z, sc, "f2")
    fr = dict(gp=f2["gp"], xy=f2["xy"], cam=f2["cam"], oct=f2["oct"], desc=f2["desc"], mask=f2["dmask"])
    frame = _device_frame(ws, fr)
    for rule, key, ratio in mr.RULES:
        if rule == 2:
            continue
        xyr, cl, qd, qm, qid, _ = mr._queries(z, sc, rule, key)
        a0 = mr._initial_assigned(z, sc, rule)
        m, kq, n, a, st = _search(ws, frame, rule, xyr, cl, qd, qm, a0, mr._th(z, sc, rule), ratio)
        assert n == int(z["w%d_r%d_%s_nmatches" % (sc, rule, key)]), (rule, key)
        assert np.array_equal(mr._assemble(z, sc, rule, m, qid), mr._expected(z, sc, rule, key)), (rule, key)
        taken = np.nonzero(kq >= 0)[0]
        assert np.array_equal(np.sort(m[m >= 0]), taken) and np.array_equal(m[kq[taken]], taken)


def test_overflow_status_and_workspace_reuse(gpu):
    import torch
    from mcs_amd import track_match as tm
    fr = tw._frame(120, n_kp=3000)
    xyr, cl, qd, _ = tw._queries(fr, 0, 121, nq=500)
    ptr, kp, _ = tw._oracle_candidates(fr, xyr, cl, qd, None)
    total = len(kp)
    assert total > 500
    a0 = tw._assigned0(fr, 0, 9)
    for cap in (7, total - 1):
        w = tm.Workspace(3000, 500, cap)
        frame = _device_frame(w, fr)
        pad = 64
        d_a = _t(np.concatenate([a0, np.full(pad, 0xAB, np.uint8)]))
        d_xyr, d_cl, d_qd = _t(xyr), _t(cl), _t(qd)
        m, kq, n, st = w.search(0, frame, d_xyr, d_cl, d_qd, tw._th(fr, 0), tw.RATIO[0], d_a)
        # canaries after every output: the entry is called again on padded buffers
        big_m = torch.full((500 + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_kq = torch.full((3000 + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_n = torch.full((1 + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_st = torch.full((2 + pad,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        f = frame.struct()
        q = tm.TrackQueries(500, 500, d_xyr.data_ptr(), d_cl.data_ptr(), None, d_qd.data_ptr(), None)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        from mcs_amd import lib
        assert lib().mcs_track_search_device(w._h, 0, ctypes.byref(f), ctypes.byref(q), tw._th(fr, 0), tw.RATIO[0],
                                             P(d_a), P(big_m), P(big_kq), P(big_n), P(big_st), None) == 0
        torch.cuda.synchronize()
        for t, used in ((big_m, 500), (big_kq, 3000), (big_n, 1), (big_st, 2)):
            assert (t[used:] == 0x5A5A5A5A).all()
        assert (d_a[3000:] == 0xAB).all()
        for mm, kk, nn, ss in ((m, kq, n, st), (big_m[:500], big_kq[:3000], big_n[:1], big_st[:2])):
            assert ss.cpu().numpy().tolist() == [total, tm.OVERFLOW]
            assert (mm == -1).all() and (kk == -1).all() and int(nn.cpu()[0]) == 0
        assert np.array_equal(d_a.cpu().numpy()[:3000], a0)      # untouched
        # the workspace that has just overflowed, on the leading queries whose lists fit its cap
        k = int(np.searchsorted(ptr, cap, side="right")) - 1
        assert (k > 0 or cap == 7) and ptr[k] <= cap < total
        got = _search(w, frame, 0, xyr[:k], cl[:k], qd[:k], None, a0, tw._th(fr, 0), tw.RATIO[0])
        n_fit = _check_match(fr, 0, xyr[:k], cl[:k], qd[:k], None, a0, got)
        assert got[4][0] == ptr[k] and (cap == 7 or n_fit > 20)
        w.close()
    # a workspace at a sufficient capacity, on two different frames in a row and back
    w = tm.Workspace(3000, 500, total + 50000)
    frame = _device_frame(w, fr)
    fr2 = tw._frame(122, n_kp=2500)
    xyr2, cl2, qd2, _ = tw._queries(fr2, 3, 123, nq=450)
    a2 = np.zeros(2500, np.uint8)
    for _ in range(2):
        got = _search(w, frame, 0, xyr, cl, qd, None, a0, tw._th(fr, 0), tw.RATIO[0])
        assert _check_match(fr, 0, xyr, cl, qd, None, a0, got) > 20 and got[4][0] == total
        got2 = _search(w, _device_frame(w, fr2), 3, xyr2, cl2, qd2, None, a2, tw._th(fr2, 3), tw.RATIO[3])
        assert _check_match(fr2, 3, xyr2, cl2, qd2, None, a2, got2) > 20
    w.close()


def test_rule1_then_rule0_share_the_assignment(ws):
    """TrackWithMotionModel's search, then TrackLocalMap's, on the same mvpMapPoints."""
    fr = tw._frame(130)
    frame = _device_frame(ws, fr)
    a = tw._assigned0(fr, 1, 11)
    for rule in (1, 0):
        xyr, cl, qd, qm = tw._queries(fr, rule, 131 + rule, nq=1500)
        got = _search(ws, frame, rule, xyr, cl, qd, None, a, tw._th(fr, rule), tw.RATIO[rule])
        assert _check_match(fr, rule, xyr, cl, qd, None, a, got) > 50
        assert got[3].sum() == a.sum() + got[2]
        a = got[3]


def _stream_case():
    """A 3-camera frame whose keypoints sit near the projections of the shared map points."""
    from mcs_amd import KEYPOINT_DTYPE
    z = _frustum_case()
    rng = np.random.default_rng(140)
    cap, C = 1200, NC
    cnt = np.array([1100, 900, 1200], np.int32)
    gp = np.array([[0.0, 0.0, 64.0 / W, 48.0 / H]] * C)
    kps = np.zeros((C, cap), KEYPOINT_DTYPE)
    desc = rng.integers(0, 256, (C, cap, 32), dtype=np.uint8)
    sel = z["iv"] == 1
    for c in range(C):
        kps[c]["x"] = rng.uniform(0, W, cap).astype(np.float32)
        kps[c]["y"] = rng.uniform(0, H, cap).astype(np.float32)
        kps[c]["octave"] = rng.integers(0, 8, cap)
        seen = np.nonzero(sel[:, c])[0]
        seen = seen[seen < cnt[c]]
        kps[c]["x"][seen] = (z["pj"][seen, c, 0] + rng.normal(0, 1.5, len(seen))).astype(np.float32)
        kps[c]["y"][seen] = (z["pj"][seen, c, 1] + rng.normal(0, 1.5, len(seen))).astype(np.float32)
        kps[c]["octave"][seen] = z["lv"][seen, c]
    n_pts = len(z["pts"])
    mp_desc = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    for c in range(C):
        seen = np.nonzero(sel[:, c])[0]
        seen = seen[seen < cnt[c]]
        for p in seen[::2]:
            desc[c, p] = tw._flip(mp_desc[p], int(rng.integers(0, 40)), rng)
    skip = (rng.random(n_pts) < 0.1).astype(np.uint8)
    return z, cap, C, cnt, gp, kps, desc, n_pts, mp_desc, skip


def test_stream_ordered_from_keypoints_to_assignment(gpu):
    """Keypoint rows per camera -> concat -> unpack -> grid -> isInFrustum -> rule 0 queries ->
    search, queued on one non-default stream with one synchronisation at the end; equal to the
    oracle chain (oracle_is_in_frustum, the query rule in numpy, oracle_window_match) on the
    same inputs."""
    import torch
    from mcs_amd import lib
    from mcs_amd import track_match as tm
    z, cap, C, cnt, gp, kps, desc, n_pts, mp_desc, skip = _stream_case()
    N = C * cap
    w = tm.Workspace(N, n_pts * C, 200000)
    up = {k: _t(z[k]) for k in ("pose", "mc", "cam", "masks", "pts", "nrm", "dist", "scale")}
    d_kps, d_cnt, d_desc, d_gp = _t(kps.view(np.int32).reshape(C, cap * 7)), _t(cnt), _t(desc), _t(gp)
    d_mpd, d_skip = _t(mp_desc), _t(skip)
    keys = torch.zeros((N, 7), dtype=torch.int32, device="cuda")
    descs = torch.zeros((N, 32), dtype=torch.uint8, device="cuda")
    k2c = torch.zeros(N, dtype=torch.int32, device="cuda")
    k2l = torch.zeros(N, dtype=torch.int32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int32, device="cuda")
    iv = torch.zeros((n_pts, C), dtype=torch.uint8, device="cuda")
    pj = torch.zeros((n_pts, C, 2), dtype=torch.float64, device="cuda")
    lv = torch.zeros((n_pts, C), dtype=torch.int32, device="cuda")
    vc = torch.zeros((n_pts, C), dtype=torch.float64, device="cuda")
    d_a = torch.zeros(N, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        st = ctypes.c_void_p(s.cuda_stream)
        assert lib().mcs_multiframe_concat_device(P(d_cnt), 1, C, cap, P(d_kps), None, P(d_desc), 32, P(d_gp),
                                                  P(keys), None, P(descs), P(k2c), P(k2l), None, P(tot), st) == 0
        xy, octv = tm.unpack_keys(keys, tot)
        ptr, cells, nin = w.grid_build(xy, k2c, d_gp, tot)
        assert lib().mcs_is_in_frustum_device(P(up["pose"]), P(up["mc"]), P(up["cam"]), C, P(up["masks"]),
                                              z["masks"].shape[2], z["masks"].shape[1], P(up["pts"]),
                                              P(up["nrm"]), P(up["dist"]), n_pts, P(up["scale"]), 8, P(iv), P(pj),
                                              P(lv), P(vc), st) == 0
        q_xyr, q_cl, q_idx = tm.queries_mappoints(iv, pj, lv, vc, up["scale"], 3.0, skip=d_skip)
        frame = tm.DeviceFrame(d_gp, xy, octv, descs, ptr, cells)
        m, kq, n, status = w.search(0, frame, q_xyr, q_cl, d_mpd, 96, 0.8, d_a, q_desc_idx=q_idx)
    s.synchronize()
    total = int(cnt.sum())
    assert int(tot.cpu()[0]) == total and not (int(status.cpu()[1]) & 1)
    cat = np.concatenate([kps[c][:cnt[c]] for c in range(C)])
    fr = dict(gp=gp, xy=np.ascontiguousarray(np.stack([cat["x"], cat["y"]], 1)),
              cam=np.repeat(np.arange(C, dtype=np.int32), cnt), oct=np.ascontiguousarray(cat["octave"]),
              desc=np.concatenate([desc[c, :cnt[c]] for c in range(C)]), mask=None, bytes=32)
    assert np.array_equal(xy.cpu().numpy()[:total], fr["xy"]) and np.array_equal(octv.cpu().numpy()[:total], fr["oct"])
    optr, ocell = _oracle_grid(gp, fr["xy"], fr["cam"])
    assert np.array_equal(ptr.cpu().numpy(), optr) and np.array_equal(cells.cpu().numpy()[:len(ocell)], ocell)
    xyr, cl, idx = _rule0_expected(z["iv"], z["pj"], z["lv"], z["vc"], skip, z["scale"], 3.0)
    xyr, cl = _for_oracle(xyr, cl)
    qd = mp_desc[idx]
    a_o = np.zeros(total, np.uint8)
    m_o = np.full(len(xyr), -7, np.int32)
    n_o = ob.lib().oracle_window_match(0, *tw._frame_args(fr), len(xyr), tw._p(xyr), tw._p(cl), tw._p(qd), None,
                                       96, 0.8, tw._p(a_o), tw._p(m_o))
    assert n_o > 40
    assert int(n.cpu()[0]) == n_o and np.array_equal(m.cpu().numpy(), m_o)
    assert np.array_equal(d_a.cpu().numpy()[:total], a_o) and not d_a.cpu().numpy()[total:].any()
    w.close()


def test_argument_errors(ws):
    import mcs_amd
    from mcs_amd import track_match as tm
    fr = tw._frame(150, n_kp=300)
    xyr, cl, qd, _ = tw._queries(fr, 3, 151, nq=40)
    frame = _device_frame(ws, fr)
    a0 = np.zeros(300, np.uint8)

    def code(fn):
        with pytest.raises(mcs_amd.McsError) as ei:
            fn()
        return ei.value.code

    run = lambda rule, frm=frame, qm=None, x=xyr, c=cl: _search(ws, frm, rule, x, c, qd, qm, a0, 96, 0.7)  # noqa: E731
    assert code(lambda: run(2)) == mcs_amd.MCS_ERR_UNSUPPORTED
    assert code(lambda: run(4)) == mcs_amd.MCS_ERR_ARG and code(lambda: run(-1)) == mcs_amd.MCS_ERR_ARG
    assert code(lambda: run(3, qm=qd)) == mcs_amd.MCS_ERR_ARG                 # masks on one side only
    bad = _device_frame(ws, fr)
    bad.bytes = 24
    assert code(lambda: run(3, frm=bad)) == mcs_amd.MCS_ERR_ARG
    bad.bytes, bad.n_cams = 32, 9
    assert code(lambda: run(3, frm=bad)) == mcs_amd.MCS_ERR_ARG
    small = tm.Workspace(299, 40, 1000)
    assert code(lambda: _search(small, frame, 3, xyr, cl, qd, None, a0, 96, 0.7)) == mcs_amd.MCS_ERR_ARG
    small.close()
    small = tm.Workspace(300, 39, 1000)
    assert code(lambda: _search(small, frame, 3, xyr, cl, qd, None, a0, 96, 0.7)) == mcs_amd.MCS_ERR_ARG
    with pytest.raises(mcs_amd.McsError):
        small.grid_build(_t(np.zeros((301, 2), np.float32)), _t(np.zeros(301, np.int32)), _t(fr["gp"]))
    small.close()
    assert code(lambda: tm.Workspace(0, 1, 1)) == mcs_amd.MCS_ERR_ARG
    # the host-buffer entry: the same answer as the device entry, and its own argument checks
    got = run(3)
    m, kq, n, a = tm.track_search_host(3, fr["gp"], fr["xy"], fr["cam"], fr["oct"], fr["desc"], xyr, cl, qd, 96, 0.7,
                                       kp_assigned=a0)
    assert n == got[2] and np.array_equal(m, got[0]) and np.array_equal(kq, got[1]) and np.array_equal(a, got[3])
    assert code(lambda: tm.track_search_host(2, fr["gp"], fr["xy"], fr["cam"], fr["oct"], fr["desc"], xyr, cl, qd,
                                             96, 0.7)) == mcs_amd.MCS_ERR_UNSUPPORTED


def test_cpp_adapters_follow_tracking(gpu, tmp_path):
    """mcs::SearchByProjection(Current, Last, th) then mcs::SearchByProjection(F, MPs, th) on the same
    frame through host/mcs_multicol.hpp (tests/cpp/track_match_demo.cpp): nmatches and mvpMapPoints
    after each equal the oracle chain (oracle_is_in_frustum for the projections, the query rules
    in numpy, oracle_window_match twice in sequence)."""
    import subprocess
    from tests.test_track_match_host_cpp import build_demo
    z, cap, C, cnt, gp, kps, desc, n_pts, mp_desc, skip = _stream_case()
    _, kp_cam, octv, valid, iv1, pj1 = _rule1_case()
    rng = np.random.default_rng(160)
    cat = np.concatenate([kps[c][:cnt[c]] for c in range(C)])
    fr = dict(gp=gp, xy=np.ascontiguousarray(np.stack([cat["x"], cat["y"]], 1)),
              cam=np.repeat(np.arange(C, dtype=np.int32), cnt), oct=np.ascontiguousarray(cat["octave"]),
              desc=np.concatenate([desc[c, :cnt[c]] for c in range(C)]), mask=None, bytes=32)
    n_cur, n_last = len(fr["xy"]), n_pts
    cur_mp = np.where(rng.random(n_cur) < 0.05, 7000 + np.arange(n_cur), -1).astype(np.int32)
    # the last frame: slot i holds map point 1000 + i at z["pts"][i], seen in camera kp_cam[i]
    own = pj1[np.arange(n_last), kp_cam]
    last_xy = (own + rng.normal(0, 2.0, own.shape)).astype(np.float32)
    last_desc = rng.integers(0, 256, (n_last, 32), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(cnt)])
    for i in np.nonzero((iv1[np.arange(n_last), kp_cam] == 1) & (valid == 1))[0][::2]:
        k = off[kp_cam[i]] + int(rng.integers(0, cnt[kp_cam[i]]))       # a current keypoint that looks like slot i
        fr["xy"][k] = (own[i] + rng.normal(0, 3.0, 2)).astype(np.float32)
        fr["oct"][k] = octv[i]
        fr["desc"][k] = tw._flip(last_desc[i], int(rng.integers(0, 30)), rng)
    last_mp = (1000 + np.arange(n_last)).astype(np.int32)
    mp_id = (5000 + np.arange(n_pts)).astype(np.int32)
    th1, th0, th_high, ratio = 15.0, 3.0, 96, 0.8
    i32 = lambda *v: np.array(v, np.int32).tobytes()  # noqa: E731
    b = lambda a, dt: np.ascontiguousarray(a, dt).tobytes()  # noqa: E731
    blob = b"".join([
        i32(C, z["masks"].shape[2], z["masks"].shape[1], 8, 32, 0, n_cur, n_last, n_pts), b(z["cam"], np.float64),
        b(z["masks"], np.uint8), b(gp, np.float64), b(z["scale"], np.float64), b(z["mc"], np.float64),
        b(z["pose"], np.float64), b(fr["xy"], np.float32), b(fr["oct"], np.int32), b(fr["cam"], np.int32),
        b(fr["desc"], np.uint8), b(last_xy, np.float32), b(octv, np.int32), b(kp_cam, np.int32), b(last_desc, np.uint8),
        b(cur_mp, np.int32), b(last_mp, np.int32), b(valid, np.uint8), b(z["pts"], np.float64), b(mp_id, np.int32),
        b(skip, np.uint8), b(z["iv"], np.uint8), b(z["pj"], np.float64), b(z["lv"], np.int32), b(z["vc"], np.float64),
        b(mp_desc, np.uint8), b([th1, th0, th_high, ratio], np.float64)])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    out = subprocess.check_output([build_demo(tmp_path), "run", str(fin), str(fout)], timeout=120).decode()
    assert "run ok" in out
    raw = np.frombuffer(fout.read_bytes(), np.int32)
    n1, n0, after1, after0 = raw[0], raw[1], raw[2:2 + n_cur], raw[2 + n_cur:]
    # the oracle chain
    live = (iv1[np.arange(n_last), kp_cam] == 1) & (valid == 1)
    xyr = np.zeros((n_last, 3))
    xyr[live, :2], xyr[live, 2] = own[live], th1 * z["scale"][octv[live]]
    cl = np.full((n_last, 3), -1, np.int32)
    cl[live] = np.stack([kp_cam, octv - 1, octv + 1], 1)[live]
    want = cur_mp.copy()
    a = (cur_mp >= 0).astype(np.uint8)
    counts = []
    for rule, (qx, qc), qd, ids in ((1, _for_oracle(xyr, cl), last_desc, last_mp),
                                    (0, _for_oracle(*_rule0_expected(z["iv"], z["pj"], z["lv"], z["vc"], skip,
                                                                     z["scale"], th0)[:2]),
                                     np.repeat(mp_desc, C, axis=0), np.repeat(mp_id, C))):
        m = np.full(len(qx), -7, np.int32)
        counts.append(ob.lib().oracle_window_match(rule, *tw._frame_args(fr), len(qx), tw._p(qx), tw._p(qc), tw._p(qd),
                                                   None, th_high, ratio, tw._p(a), tw._p(m)))
        want[m[m >= 0]] = ids[m >= 0]
        if rule == 1:
            want1 = want.copy()
    assert counts[0] > 40 and counts[1] > 40
    assert [int(n1), int(n0)] == counts
    assert np.array_equal(after1, want1) and np.array_equal(after0, want)
