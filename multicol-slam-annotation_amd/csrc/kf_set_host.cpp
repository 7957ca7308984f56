#include "kf_set_host.hpp"
#include <algorithm>
#include <cstdio>

namespace mcs {
void set_error(const char* msg);

namespace host {

static int fail(const char* who, const char* what) {
  char msg[160];
  std::snprintf(msg, sizeof msg, "%s: %s", who, what);
  set_error(msg);
  return MCS_ERR_ARG;
}

int check_set_offsets(const int32_t* off, int n_sets, int n_total, int max_per_set, const char* who) {
  if (off[0] != 0 || off[n_sets] != n_total) return fail(who, "off[0] must be 0 and off[n_targets] n_kp_total");
  for (int t = 0; t < n_sets; t++) {
    if (off[t + 1] < off[t]) return fail(who, "offsets must be non-decreasing");
    if (max_per_set > 0 && off[t + 1] - off[t] >= max_per_set) {
      char what[96];
      std::snprintf(what, sizeof what, "keypoints per target must be below %d%s", max_per_set,
                    max_per_set == (1 << 19) ? " = 2^19 (position field of the key)" : "");
      return fail(who, what);
    }
  }
  return MCS_OK;
}

int check_kp_cam(const int32_t* kp_cam, int n, int n_cams, const char* who) {
  for (int i = 0; i < n; i++)
    if (kp_cam[i] < 0 || kp_cam[i] >= n_cams) return fail(who, "kp_cam outside [0, n_cams)");
  return MCS_OK;
}

int build_set_grids(const mcs_fuse_targets& k, std::vector<int32_t>& cell_ptr, std::vector<int32_t>& cell_kp) {
  const size_t ncell = (size_t)k.n_cams * MCS_GRID_COLS * MCS_GRID_ROWS;
  cell_ptr.assign((size_t)k.n_targets * (ncell + 1), 0);
  cell_kp.assign(std::max<size_t>(1, (size_t)k.n_kp_total), 0);
  for (int t = 0; t < k.n_targets; t++) {
    const size_t o = (size_t)k.off[t];
    const int rc = mcs_frame_grid_build(k.kp_xy ? k.kp_xy + 2 * o : nullptr, k.kp_cam ? k.kp_cam + o : nullptr,
                                        k.off[t + 1] - k.off[t], k.n_cams, k.grid_params,
                                        cell_ptr.data() + (size_t)t * (ncell + 1), cell_kp.data() + o, nullptr);
    if (rc) { set_error("keyframe set: grid build failed"); return rc; }
  }
  return MCS_OK;
}

}  // namespace host
}  // namespace mcs
