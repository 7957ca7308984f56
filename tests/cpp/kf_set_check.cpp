// Stand-alone check of csrc/kf_set_host.cpp (with csrc/window_host.cpp): build_set_grids against
// per-target mcs_frame_grid_build calls, and the rejections of check_set_offsets / check_kp_cam
// with their messages.  Plain C++; exits 0 and prints "ok" when everything holds.
#include "../../multicol-slam-annotation_amd/csrc/kf_set_host.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::string g_err;
namespace mcs {
void set_error(const char* msg) { g_err = msg; }
}  // namespace mcs

static int g_fail = 0;
#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_fail++; } \
  } while (0)

static bool rejected(int rc, const char* who, const char* text) {
  const bool ok = rc == MCS_ERR_ARG && g_err.rfind(std::string(who) + ": ", 0) == 0 &&
                  g_err.find(text) != std::string::npos;
  if (!ok) std::printf("rc %d, message \"%s\", wanted \"%s: ...%s...\"\n", rc, g_err.c_str(), who, text);
  g_err.clear();
  return ok;
}

int main() {
  using namespace mcs::host;
  constexpr int T = 3, C = 2, kCells = C * MCS_GRID_COLS * MCS_GRID_ROWS;
  // targets of 1, 0 and 5 keypoints (the empty one in the middle) on two 640 x 480 cameras, the
  // second camera's grid starting at (10, 20)
  const int32_t off[T + 1] = {0, 1, 1, 6};
  const double gp[4 * C] = {0.0, 0.0, 64.0 / 640.0, 48.0 / 480.0, 10.0, 20.0, 64.0 / 640.0, 48.0 / 480.0};
  const float xy[2 * 6] = {100.5f, 200.25f,                       // target 0
                           4.0f, 7.0f, 630.0f, 470.0f, 700.0f, 10.0f /* outside the grid */, 320.0f, 240.0f,
                           12.0f, 22.0f};                          // target 2
  int32_t cam[6] = {1, 0, 1, 0, -1 /* no camera */, 1};
  mcs_fuse_targets k{};
  k.n_targets = T; k.n_kp_total = 6; k.n_cams = C;
  k.off = off; k.kp_xy = xy; k.kp_cam = cam; k.grid_params = gp;

  std::vector<int32_t> cell_ptr, cell_kp;
  REQUIRE(build_set_grids(k, cell_ptr, cell_kp) == MCS_OK);
  REQUIRE(cell_ptr.size() == (size_t)T * (kCells + 1));
  REQUIRE(cell_kp.size() == 6);
  const int want_in_grid[T] = {1, 0, 3};
  for (int t = 0; t < T; t++) {
    const int o = off[t], n = off[t + 1] - o;
    std::vector<int32_t> ptr(kCells + 1, -7), kp(n > 0 ? n : 1, 0);
    int32_t in_grid = -1;
    REQUIRE(mcs_frame_grid_build(xy + 2 * o, cam + o, n, C, gp, ptr.data(), kp.data(), &in_grid) == MCS_OK);
    REQUIRE(in_grid == want_in_grid[t]);
    REQUIRE(std::memcmp(ptr.data(), cell_ptr.data() + (size_t)t * (kCells + 1), sizeof(int32_t) * (kCells + 1)) == 0);
    REQUIRE(std::memcmp(kp.data(), cell_kp.data() + o, sizeof(int32_t) * n) == 0);
  }
  // target 2 in cell order: keypoint 0 (camera 0), then camera 1's keypoint 4 in cell (0, 0) and
  // keypoint 1 in cell (62, 45); 2 is outside the grid, 3 has no camera
  const int32_t* p2 = cell_ptr.data() + 2 * (size_t)(kCells + 1);
  REQUIRE(p2[kCells] == 3);
  REQUIRE(p2[1 * MCS_GRID_COLS * MCS_GRID_ROWS] == 1 && p2[1 * MCS_GRID_COLS * MCS_GRID_ROWS + 1] == 2);
  REQUIRE(cell_kp[off[2]] == 0 && cell_kp[off[2] + 1] == 4 && cell_kp[off[2] + 2] == 1);

  // a set of no targets
  mcs_fuse_targets none = k;
  none.n_targets = 0; none.n_kp_total = 0;
  REQUIRE(build_set_grids(none, cell_ptr, cell_kp) == MCS_OK);
  REQUIRE(cell_ptr.empty() && cell_kp.size() == 1);

  // offsets
  REQUIRE(check_set_offsets(off, T, 6, 1 << 19, "fuse") == MCS_OK);
  REQUIRE(check_set_offsets(off, T, 6, 0, "fuse") == MCS_OK);
  REQUIRE(check_set_offsets(off, T, 6, 6, "fuse") == MCS_OK);          // 5 < 6
  REQUIRE(rejected(check_set_offsets(off, T, 6, 5, "fuse"), "fuse", "below 5"));
  const int32_t off_first[T + 1] = {1, 1, 1, 6};
  REQUIRE(rejected(check_set_offsets(off_first, T, 6, 1 << 19, "fuse"), "fuse", "off[0] must be 0"));
  const int32_t off_dec[T + 1] = {0, 4, 3, 6};
  REQUIRE(rejected(check_set_offsets(off_dec, T, 6, 1 << 19, "sim3"), "sim3", "non-decreasing"));
  REQUIRE(rejected(check_set_offsets(off_dec, T, 6, 0, "sim3 solver"), "sim3 solver", "non-decreasing"));
  REQUIRE(rejected(check_set_offsets(off, T, 7, 1 << 19, "fuse"), "fuse", "off[n_targets] n_kp_total"));
  const int32_t off_big[3] = {0, 3, 3 + (1 << 19)};                      // offsets only, no arrays
  REQUIRE(rejected(check_set_offsets(off_big, 2, 3 + (1 << 19), 1 << 19, "fuse"), "fuse", "2^19"));
  const int32_t off_under[3] = {0, 3, 3 + (1 << 19) - 1};
  REQUIRE(check_set_offsets(off_under, 2, 3 + (1 << 19) - 1, 1 << 19, "fuse") == MCS_OK);
  REQUIRE(check_set_offsets(off_big, 2, 3 + (1 << 19), 0, "sim3 solver") == MCS_OK);   // no per-set bound

  // cameras
  REQUIRE(rejected(check_kp_cam(cam, 6, C, "sim3"), "sim3", "kp_cam outside [0, n_cams)"));
  cam[4] = 2;
  REQUIRE(rejected(check_kp_cam(cam, 6, C, "sim3"), "sim3", "kp_cam outside [0, n_cams)"));
  cam[4] = 1;
  REQUIRE(check_kp_cam(cam, 6, C, "sim3") == MCS_OK);
  REQUIRE(check_kp_cam(nullptr, 0, C, "sim3") == MCS_OK);

  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("ok\n");
  return 0;
}
