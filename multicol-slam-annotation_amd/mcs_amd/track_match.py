"""The windowed matchers of tracking with nothing downloaded (include/mcs_matcher.h, the device
form of the window API; csrc/track_match.hip).

  SearchByProjection(F, vpMapPoints, th)   src/cORBmatcher.cpp:67-166     rule 0 (TrackLocalMap)
  SearchByProjection(Current, Last, th)    src/cORBmatcher.cpp:1991-2123  rule 1 (TrackWithMotionModel)
  WindowSearch(F1, F2, windowSize, ...)    src/cORBmatcher.cpp:326-473    rule 3 (TrackPreviousFrame)

The cMultiFrame grid (grid_build_device), the queries of rules 0 and 1 (queries_mappoints /
queries_lastframe) and the search with its ordered selection (Workspace.search) are enqueued on
the current torch stream; every argument and result is a torch tensor on the device and no call
synchronises.  window.py holds the host-split form of the same rules (and rule 2).
"""
import ctypes

import numpy as np

from . import _check, lib
from .window import GRID_COLS, GRID_ROWS, WindowFrame

MAX_CAMS = 8
OVERFLOW = 1


def rounds(flags):
    """Settle rounds of a call from its status flags (MCS_TRACK_ROUNDS)."""
    return (int(flags) & 0xFFFFFFFFFFFFFFFF) >> 32


class TrackFrame(ctypes.Structure):
    """Mirror of mcs_track_frame."""
    _fields_ = [("n_cams", ctypes.c_int32), ("n_kp", ctypes.c_int32), ("bytes", ctypes.c_int32),
                ("grid_params", ctypes.c_void_p), ("cell_ptr", ctypes.c_void_p),
                ("cell_kp", ctypes.c_void_p), ("kp_xy", ctypes.c_void_p),
                ("kp_octave", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("desc_mask", ctypes.c_void_p)]


class TrackQueries(ctypes.Structure):
    """Mirror of mcs_track_queries."""
    _fields_ = [("nq", ctypes.c_int32), ("n_src", ctypes.c_int32), ("q_xyr", ctypes.c_void_p),
                ("q_cam_lvl", ctypes.c_void_p), ("q_desc_idx", ctypes.c_void_p),
                ("q_desc_src", ctypes.c_void_p), ("q_mask_src", ctypes.c_void_p)]


def _dp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _stream(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class DeviceFrame:
    """A frame on the device as the search reads it: tensors kp_xy [n_kp, 2] float32, kp_octave
    [n_kp] int32, desc [n_kp, bytes] uint8 (+ desc_mask), gp [n_cams, 4] float64 and the grid
    (cell_ptr, cell_kp) of Workspace.grid_build.  The tensors are kept alive here."""

    def __init__(self, gp, kp_xy, kp_octave, desc, cell_ptr, cell_kp, desc_mask=None):
        self.gp, self.kp_xy, self.kp_octave, self.desc = gp, kp_xy, kp_octave, desc
        self.cell_ptr, self.cell_kp, self.desc_mask = cell_ptr, cell_kp, desc_mask
        self.n_cams, self.n_kp, self.bytes = gp.shape[0], kp_xy.shape[0], desc.shape[1]

    def struct(self):
        return TrackFrame(self.n_cams, self.n_kp, self.bytes, self.gp.data_ptr(), self.cell_ptr.data_ptr(),
                          self.cell_kp.data_ptr(), self.kp_xy.data_ptr(), self.kp_octave.data_ptr(),
                          self.desc.data_ptr(), None if self.desc_mask is None else self.desc_mask.data_ptr())


class Workspace:
    """mcs_track_workspace: reusable device scratch of the grid build and the search."""

    def __init__(self, max_kp, max_queries, cand_cap, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().mcs_track_workspace_create(int(device), int(max_kp), int(max_queries), int(cand_cap),
                                                ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().mcs_track_workspace_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def grid_build(self, kp_xy, kp_cam, gp, n_kp=None):
        """mcs_frame_grid_build_device -> (cell_ptr, cell_kp [cap], n_in_grid [1]) tensors.
        n_kp: int32 tensor [1] holding the keypoint count (None = all rows)."""
        import torch
        cap, C = kp_xy.shape[0], gp.shape[0]
        ptr = torch.empty(C * GRID_COLS * GRID_ROWS + 1, dtype=torch.int32, device=kp_xy.device)
        cells = torch.empty(max(cap, 1), dtype=torch.int32, device=kp_xy.device)
        nin = torch.empty(1, dtype=torch.int32, device=kp_xy.device)
        _check(lib().mcs_frame_grid_build_device(self._h, _dp(kp_xy), _dp(kp_cam), _dp(n_kp), cap, C, _dp(gp),
                                                 _dp(ptr), _dp(cells), _dp(nin), _stream(kp_xy)))
        return ptr, cells, nin

    def search(self, rule, frame, q_xyr, q_cam_lvl, q_desc_src, th_high, nnratio, kp_assigned,
               q_desc_idx=None, q_mask_src=None):
        """mcs_track_search_device.  kp_assigned [n_kp] uint8 is updated in place.
        Returns (match [nq], kp_query [n_kp], n_matches [1], status [2] int64) tensors."""
        import torch
        dev = q_xyr.device
        nq = q_xyr.shape[0]
        q = TrackQueries(nq, q_desc_src.shape[0], q_xyr.data_ptr(), q_cam_lvl.data_ptr(),
                         None if q_desc_idx is None else q_desc_idx.data_ptr(), q_desc_src.data_ptr(),
                         None if q_mask_src is None else q_mask_src.data_ptr())
        f = frame.struct()
        match = torch.empty(max(nq, 1), dtype=torch.int32, device=dev)
        kp_query = torch.empty(max(frame.n_kp, 1), dtype=torch.int32, device=dev)
        n_matches = torch.empty(1, dtype=torch.int32, device=dev)
        status = torch.empty(2, dtype=torch.int64, device=dev)
        _check(lib().mcs_track_search_device(self._h, int(rule), ctypes.byref(f), ctypes.byref(q), int(th_high),
                                             float(nnratio), _dp(kp_assigned), _dp(match), _dp(kp_query),
                                             _dp(n_matches), _dp(status), _stream(q_xyr)))
        return match[:nq], kp_query[:frame.n_kp], n_matches, status

    def select(self, rule, frame, q_cam_lvl, th_high, nnratio, kp_assigned, out):
        """mcs_track_select_device over the lists of the last search; out = the tuple search returned."""
        match, kp_query, n_matches, status = out
        _check(lib().mcs_track_select_device(self._h, int(rule), q_cam_lvl.shape[0], _dp(q_cam_lvl),
                                             _dp(frame.kp_octave), frame.n_kp, frame.n_cams, int(th_high),
                                             float(nnratio), _dp(kp_assigned), _dp(match), _dp(kp_query),
                                             _dp(n_matches), _dp(status), _stream(q_cam_lvl)))


def unpack_keys(keys, n=None):
    """mvKeys rows (mcs_keypoint, [cap, 7] int32 view) -> (kp_xy [cap, 2] float32, kp_octave [cap])."""
    import torch
    cap = keys.shape[0]
    xy = torch.zeros((cap, 2), dtype=torch.float32, device=keys.device)
    octv = torch.zeros(cap, dtype=torch.int32, device=keys.device)
    _check(lib().mcs_track_unpack_keys_device(_dp(keys), _dp(n), cap, _dp(xy), _dp(octv), _stream(keys)))
    return xy, octv


def _query_out(nq, dev):
    import torch
    return (torch.empty((nq, 3), dtype=torch.float64, device=dev),
            torch.empty((nq, 3), dtype=torch.int32, device=dev),
            torch.empty(nq, dtype=torch.int32, device=dev))


def queries_mappoints(in_view, proj, level, view_cos, scale, th, skip=None):
    """Rule 0 queries from isInFrustum's outputs ([n, C] tensors) -> (q_xyr, q_cam_lvl, q_desc_idx)."""
    n, C = in_view.shape
    out = _query_out(n * C, in_view.device)
    _check(lib().mcs_track_queries_mappoints_device(_dp(in_view), _dp(proj), _dp(level), _dp(view_cos), _dp(skip),
                                                    n, C, _dp(scale), scale.shape[0], float(th), _dp(out[0]),
                                                    _dp(out[1]), _dp(out[2]), _stream(in_view)))
    return out


def queries_lastframe(pose, mc, cam, masks, pos, valid, kp_cam, kp_octave, scale, th, n=None):
    """Rule 1 queries, one per last-frame slot -> (q_xyr, q_cam_lvl, q_desc_idx)."""
    cap = pos.shape[0]
    out = _query_out(cap, pos.device)
    _check(lib().mcs_track_queries_lastframe_device(_dp(pose), _dp(mc), _dp(cam), mc.shape[0], _dp(masks),
                                                    masks.shape[2], masks.shape[1], _dp(pos), _dp(valid),
                                                    _dp(kp_cam), _dp(kp_octave), _dp(n), cap, _dp(scale),
                                                    scale.shape[0], float(th), _dp(out[0]), _dp(out[1]),
                                                    _dp(out[2]), _stream(pos)))
    return out


def track_search_host(rule, gp, kp_xy, kp_cam, kp_octave, desc, q_xyr, q_cam_lvl, q_desc_src, th_high,
                      nnratio, q_desc_idx=None, desc_mask=None, q_mask_src=None, kp_assigned=None, device=0):
    """mcs_track_search: host buffers in, (match, kp_query, n_matches, kp_assigned) out."""
    gp = np.ascontiguousarray(gp, np.float64).reshape(-1, 4)
    xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    cam = np.ascontiguousarray(kp_cam, np.int32)
    octv = np.ascontiguousarray(kp_octave, np.int32)
    desc = np.ascontiguousarray(desc, np.uint8)
    dm = None if desc_mask is None else np.ascontiguousarray(desc_mask, np.uint8)
    f = WindowFrame(len(gp), len(xy), desc.shape[1], _hp(gp).value, _hp(xy).value, _hp(cam).value,
                    _hp(octv).value, _hp(desc).value, None if dm is None else _hp(dm).value)
    q_xyr = np.ascontiguousarray(q_xyr, np.float64).reshape(-1, 3)
    nq = len(q_xyr)
    q_cl = np.ascontiguousarray(q_cam_lvl, np.int32).reshape(nq, 3)
    src = np.ascontiguousarray(q_desc_src, np.uint8).reshape(-1, desc.shape[1])
    qm = None if q_mask_src is None else np.ascontiguousarray(q_mask_src, np.uint8)
    qi = None if q_desc_idx is None else np.ascontiguousarray(q_desc_idx, np.int32)
    q = TrackQueries(nq, len(src), _hp(q_xyr).value, _hp(q_cl).value, None if qi is None else _hp(qi).value,
                     _hp(src).value, None if qm is None else _hp(qm).value)
    a = np.zeros(max(len(xy), 1), np.uint8)
    if kp_assigned is not None:
        a[:len(xy)] = np.asarray(kp_assigned, np.uint8)
    m = np.zeros(max(nq, 1), np.int32)
    kq = np.zeros(max(len(xy), 1), np.int32)
    n = ctypes.c_int32()
    _check(lib().mcs_track_search(int(device), int(rule), ctypes.byref(f), ctypes.byref(q), int(th_high),
                                  float(nnratio), _hp(a), _hp(m), _hp(kq), ctypes.byref(n)))
    return m[:nq], kq[:len(xy)], n.value, a[:len(xy)]


__all__ = ["DeviceFrame", "TrackFrame", "TrackQueries", "Workspace", "unpack_keys", "queries_mappoints",
           "queries_lastframe", "track_search_host", "rounds", "MAX_CAMS", "OVERFLOW"]
