// Host plumbing shared by the C-ABI entries: argument errors, opening a device by ordinal, the
// device buffers of one host-buffer call and the upload of a packed keyframe set.  One definition
// each, so every entry reports and releases alike.
#pragma once
#include "common.hpp"
#include "kf_set_host.hpp"
#include <algorithm>
#include <cstdio>
#include <vector>

namespace mcs {
namespace host {

inline int bad_arg(const char* msg) { set_error(msg); return MCS_ERR_ARG; }

// MCS_OK when a HIP device is visible; *ndev = how many
inline int have_device(int* ndev) {
  if (hipGetDeviceCount(ndev) != hipSuccess || *ndev == 0) {
    set_error("no HIP device visible (no CPU fallback)");
    return MCS_ERR_NO_DEVICE;
  }
  return MCS_OK;
}

// make `device` the calling thread's device
inline int open_device(int device, const char* who) {
  int ndev = 0;
  if (int rc = have_device(&ndev)) return rc;
  if (device < 0 || device >= ndev) {
    char msg[128];
    std::snprintf(msg, sizeof msg, "%s: no such device", who);
    return bad_arg(msg);
  }
  MCS_HIP_CHECK(hipSetDevice(device));
  return MCS_OK;
}

inline int check_desc_bytes(int bytes, const char* who) {
  if (bytes == 16 || bytes == 32 || bytes == 64) return MCS_OK;
  char msg[128];
  std::snprintf(msg, sizeof msg, "%s: descriptor bytes must be 16, 32 or 64", who);
  return bad_arg(msg);
}

// device allocations of one host-buffer call, released on every return path; the first HIP error
// stays in `err` and turns the later calls into no-ops
struct DevBufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  template <class T> T* alloc(size_t n) {
    void* q = nullptr;
    if (err == hipSuccess) err = hipMalloc(&q, std::max<size_t>(1, n) * sizeof(T));
    if (q) p.push_back(q);
    return static_cast<T*>(q);
  }
  // a null host pointer stays null on the device
  template <class T> T* up(const T* h, size_t n) {
    if (!h) return nullptr;
    T* d = alloc<T>(n);
    if (err == hipSuccess && n) err = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  // a null host pointer is an output the caller does not want
  template <class T> void down(T* h, const T* d, size_t n) {
    if (err == hipSuccess && h && n) err = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
  }
  ~DevBufs() { for (void* q : p) (void)hipFree(q); }
};

// What upload_kf_set copies besides off, kp_octave, m_t, m_c and cam, which every caller reads.
constexpr unsigned kKfSearch = 1;   // kp_xy, desc, mask, mirror, grid_params, scale and the built grids
constexpr unsigned kKfCam = 2;      // kp_cam
constexpr unsigned kKfRays = 4;     // rays

// Device copy of a packed host set: *dev = host with the arrays of `fields` uploaded and every
// other pointer null.  HIP errors go to B.err; the return value is the grid build's.
inline int upload_kf_set(DevBufs& B, const mcs_fuse_targets& h, unsigned fields, mcs_fuse_targets* dev) {
  const size_t T = (size_t)h.n_targets, C = (size_t)h.n_cams, nk = (size_t)h.n_kp_total, nb = (size_t)h.bytes;
  const bool search = (fields & kKfSearch) != 0;
  std::vector<int32_t> cell_ptr, cell_kp;
  if (search)
    if (int rc = build_set_grids(h, cell_ptr, cell_kp)) return rc;
  mcs_fuse_targets d = h;
  d.off = B.up(h.off, T + 1);
  d.kp_octave = B.up(h.kp_octave, nk);
  d.m_t = B.up(h.m_t, 16 * T);
  d.m_c = B.up(h.m_c, 16 * C);
  d.cam = B.up(h.cam, 17 * C);
  d.kp_cam = (fields & kKfCam) ? B.up(h.kp_cam, nk) : nullptr;
  d.rays = (fields & kKfRays) ? B.up(h.rays, 3 * nk) : nullptr;
  d.kp_xy = search ? B.up(h.kp_xy, 2 * nk) : nullptr;
  d.desc = search ? B.up(h.desc, nk * nb) : nullptr;
  d.mask = search ? B.up(h.mask, nk * nb) : nullptr;
  d.mirror = search ? B.up(h.mirror, C * h.mirror_w * h.mirror_h) : nullptr;
  d.grid_params = search ? B.up(h.grid_params, 4 * C) : nullptr;
  d.scale = search ? B.up(h.scale, (size_t)h.n_levels) : nullptr;
  d.cell_ptr = search ? B.up(cell_ptr.data(), cell_ptr.size()) : nullptr;
  d.cell_kp = search ? B.up(cell_kp.data(), cell_kp.size()) : nullptr;
  *dev = d;
  return MCS_OK;
}

}  // namespace host
}  // namespace mcs
