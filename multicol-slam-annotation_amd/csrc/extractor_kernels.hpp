// Kernel argument blocks and launch wrappers of the extractor pipeline (one .hip file per
// stage; the host orchestration lives in extractor.hip).
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include <cstdint>
#include "extractor_plan.hpp"
#include "pyr_groups.hpp"
#include "pyr_units.hpp"

namespace mcs {

// Workgroup -> (frame, item) mapping that keeps all workgroups of one frame on one XCD
// (dispatch deals workgroups round-robin over the 8 XCDs; speed only, never correctness).
// Grid = 8 * ceil(F/8) * items_per_frame workgroups; returns false for padding groups.
__device__ __forceinline__ bool xcd_frame_map(int b, int F, int items, int* frame, int* item) {
  const int x = b & 7, k = b >> 3;
  const int f = x + 8 * (k / items);
  *item = k % items;
  *frame = f;
  return f < F;
}
inline unsigned xcd_grid(int F, int items) { return (unsigned)(8 * ((F + 7) / 8) * items); }

struct LevelPtrs {
  int32_t w[kMaxLevels], h[kMaxLevels], pitch[kMaxLevels], bpitch[kMaxLevels];
  int64_t pyr_off[kMaxLevels], img_off[kMaxLevels], mask_off[kMaxLevels];
};

// ---- K1+K5 fused: resize level l-1 -> l (or take level 0) + 5x5 blur of the level
struct PyrArgs {
  const uint8_t* src; int64_t src_fstride; int sw, sh, spitch;  // level l-1 (or level 0)
  uint8_t* dst; int64_t dst_fstride; int dpitch;                // level l raw (RESIZE only)
  uint8_t* blur; int64_t blur_fstride; int bpitch;              // level l blurred
  int dw, dh;
  const int32_t* xofs; const int16_t* alpha; const int32_t* yofs; const int16_t* beta;
  int simd_end;
  int nframes;
  // waves of the level (pack_pyr_units) for groups of `gsize` frame slots: wave `u` of group g
  // takes waves[group_mask[g] * wave_mstride + u]; wave_mstride == 0: one list for every group
  const PyrWave* waves; int nwaves; int64_t wave_mstride;
  // frames of group g: group_frames[g * gsize + slot], ascending, -1 = absent (k_pyr_groups);
  // nullptr: the consecutive frames g * gsize + slot < nframes, and mask 0
  const int32_t* group_frames; const int32_t* group_mask; int ngroups, gsize;
  // the full-frame geometry of pyr_strips (not read by the kernel)
  int tiles_x, tiles_y;            // tiles_x = column strips, tiles_y = row segments
  int core, seg_rows;              // strip width (px, multiple of 4, <= 244), segment height
};
// the geometry rule lives in pyr_units.hpp (host only); the kernel takes its strips and
// segments from the unit table built with it (build_pyr_units)
inline void pyr_strips(int dw, int dh, int F, PyrArgs& a) {
  pyr_strip_geometry(dw, dh, F, &a.core, &a.tiles_x, &a.seg_rows, &a.tiles_y);
}
// wide: source tiles for scale factors in (1.5, 2.2] (larger LDS footprint)
void launch_pyr_blur(const PyrArgs& a, bool resize, bool wide, hipStream_t st);
// group_frames / group_mask of a batch from its mask indices (pyr_groups.hpp), one workgroup.
// Its counters are in LDS up to kPyrGroupMasks masks; beyond, in `scratch` (5 * nmasks entries)
constexpr int kPyrGroupMasks = 256;
void launch_pyr_groups(const int32_t* d_mask_index, int F, int nmasks, int G,
                       int32_t* group_frames, int32_t* group_mask, int32_t* scratch,
                       hipStream_t st);

void launch_mask_pyramids(const Plan& pl, const uint8_t* d_masks, int n, uint8_t* dst,
                          hipStream_t st);
// ---- K2: FAST over runs of cells (row-streaming), one wave per FastWave (one or two runs)
struct FastRowArgs {
  const uint8_t* img0; int64_t img0_fstride;
  const uint8_t* pyr; int64_t pyr_fstride;
  const uint8_t* mask_pyr; int64_t mask_fstride;  // mask pyramids (nullable = no mask)
  const int32_t* mask_index; int nmasks;           // index clamped to [0, nmasks)
  const FastWave* units; int nunits;
  int64_t unit_mstride;   // per-mask unit lists (pack_fast_units): units of mask m at
                          // units + m * unit_mstride; 0 = one list for every frame
  const CellDesc* cells; int ncells;
  uint32_t* slots; int64_t slots_fstride;
  int32_t* cell_counts;
  int threshold;
  uint32_t kk, rbits;     // byte-wise compare constants (v_lerp_u8), see launch_fast_rows
  int pattern;            // FAST circle: 16 (TYPE_9_16), 12 (TYPE_7_12) or 8 (TYPE_5_8)
  int32_t* frame_count;   // per-frame keypoint counts the octree adds into: zeroed here (unit 0)
  int nframes;
  LevelPtrs lp;
};
void launch_fast_rows(const FastRowArgs& a, hipStream_t st);

// ---- K3: octree
struct OctArgs {
  LevelPlan lv[kMaxLevels];
  const CellDesc* cells;
  const int32_t* cell_counts; int ncells;
  const uint32_t* slots; int64_t slots_fstride;
  uint32_t* cand; int32_t* cnode; int64_t cand_fstride;
  uint32_t* sel; int64_t sel_fstride;
  int32_t* sel_count; int nlevels;
  int32_t* frame_count;
  int nframes;
};
void launch_octree(const OctArgs& a, int max_list, hipStream_t st);

// ---- K4+K6: orientation + descriptors
struct DescArgs {
  LevelPlan lv[kMaxLevels];
  int nlevels;
  const uint8_t* img0; int64_t img0_fstride;
  const uint8_t* pyr; int64_t pyr_fstride;
  const uint8_t* blur; int64_t blur_fstride;
  const uint32_t* sel; int64_t sel_fstride; int sel_per_frame;
  const int32_t* sel_count;
  mcs_keypoint* kps; uint8_t* desc; int cap; int desc_size;
  int nframes;
  // dBRIEF / mdBRIEF (mode 1 / 2; mode 0 = ORB)
  int mode, do_dbrief;
  const mcs_cam_model* cams; const int32_t* cam_index;
  uint8_t* desc_masks;
};
void launch_orient_desc(const DescArgs& a, hipStream_t st);
int upload_desc_constants();

}  // namespace mcs
