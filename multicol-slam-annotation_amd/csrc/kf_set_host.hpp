// Host checks and the grid build of a packed keyframe set (mcs_fuse_targets), shared by the host
// entries mcs_fuse, mcs_search_by_sim3 and mcs_sim3_solver.  Plain C++: no device.
#pragma once
#include "../../include/mcs_matcher.h"
#include <vector>

namespace mcs {
namespace host {

// off[0] == 0, non-decreasing, off[n_sets] == n_total and, when max_per_set > 0, fewer than
// max_per_set entries per set.  MCS_ERR_ARG with "<who>: ..." as the error text otherwise.
int check_set_offsets(const int32_t* off, int n_sets, int n_total, int max_per_set, const char* who);

// every kp_cam inside [0, n_cams)
int check_kp_cam(const int32_t* kp_cam, int n, int n_cams, const char* who);

// mcs_frame_grid_build of every target: cell_ptr [n_targets][n_cams * 64 * 48 + 1], cell_kp
// [max(1, n_kp_total)] with target t's list at off[t]
int build_set_grids(const mcs_fuse_targets& host, std::vector<int32_t>& cell_ptr,
                    std::vector<int32_t>& cell_kp);

}  // namespace host
}  // namespace mcs
