// Extractor plan: all per-configuration geometry computed once on the host at
// mcs_extractor_create() (the reference recomputes it every call inside
// ComputePyramid / ComputeKeyPointsOctTree, src/mdBRIEFextractorOct.cpp:1158-1201,
// 863-971).  Plain structs so they can be passed to kernels by value.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/mcs_extractor.h"

namespace mcs {

constexpr int kMaxLevels = 12;
constexpr int kEdgeThreshold = 25;             // src/mdBRIEFextractorOct.cpp:86
constexpr int kMinBorder = kEdgeThreshold - 3; // :876
constexpr int kPatchSize = 32;                 // :84
constexpr int kHalfPatch = 16;                 // :85
constexpr int kMaxCellDim = 64;                // window bound per FAST cell (host-checked)
constexpr int kMaxCellsPerLevel = 2048;        // LDS prefix table in the octree kernel
constexpr int kOctMaxL = 1024;                 // octree node-list bound (host-checked)
// pyramid source-tile bound (k_pyramid.hip).  The plan holds double((float)scale_factor), so the
// bound is the float 2.2f widened, not the double 2.2 (which lies below it and would reject a
// caller who passes the documented maximum).
constexpr double kMaxScaleFactor = (double)2.2f;

// One FAST cell of ComputeKeyPointsOctTree (:892-948): the detection window is the
// cell ROI shrunk by 3 px (FAST_t rows/cols [3, n-3)), absolute level coordinates.
struct CellDesc {
  int32_t level;
  int16_t wx0, wy0, wx1, wy1;  // window [wx0,wx1) x [wy0,wy1)
  int32_t slot_off;            // first candidate slot of this cell within a frame
  int32_t slot_cap;            // ceil(ww/2)*ceil(wh/2): max survivors of strict 8-NMS
};

// One run of the row-streaming FAST kernel (k_fast_rows): consecutive cells of one cell row of
// one level, as split_runs / build_masked_units cut them (host only: the pyramid's need sets
// are built from these, and pack_fast_units makes the kernel's waves of them).  A run alone in
// a wave holds columns [xa + 4L, xa + 4L + 4) in lane L and is sized so that every detection
// pixel's 7x7 neighbourhood lies in lanes 0..62 (ux0 - 3 >= xa, ux1 + 3 <= xa + 252).  Cell k of
// the run starts at ux0 + k * wcell (every cell of a level is wcell wide except a clamped last
// one, which ends at ux1).
struct FastUnit {
  int16_t level, ncells;
  int16_t wy0, wy1;    // detection rows of the cell row
  int16_t ux0, ux1;    // detection columns [first cell wx0, last cell wx1)
  int16_t xa, wcell;
  int32_t cell0;       // global index of the run's first cell
};
constexpr int kFastUnitSpan = 252;   // lanes 0..62 x 4 px

// One wave of k_fast_rows: one or two runs of cells side by side in the wave's lanes
// (pack_fast_units).  Run s holds columns [xa + 4 (L - lane0), +4), xa = (ux0 - 3) & ~3, in lane L of its lanes: run 0
// the lanes [0, split), run 1 the lanes [split, 64).  A run of n = ceil((ux1 + 3 - xa) / 4)
// dwords needs n lanes where the level's rows are dword-aligned and n + 1 where they are not
// (the kernel undoes a row's byte offset with the next lane's dword), so every detection pixel's
// 7x7 neighbourhood lies in its own run's lanes.  Both runs are on one level and equally high
// (wh rows from their wy0); the cells of run 1 follow those of run 0 in the wave's per-lane cell
// counters (lane k: cell k of the concatenation).  A wave of one run has split = 64 and an empty
// run 1 (ncells = 0, ux0 = ux1) laid over run 0's rows; wh = 0 is a count-zeroing wave of run
// 0's cells; all zero is a pad.
struct FastRun {
  int16_t wy0;         // first detection row
  int16_t ux0, ux1;    // detection columns [first cell wx0, last cell wx1); the run's first
                       // lane starts at column xa = (ux0 - 3) & ~3
  int16_t ncells;
  int32_t cell0;       // global index of the run's first cell
};
struct FastWave {
  int16_t level, wcell;
  int16_t wh;          // detection rows wy1 - wy0 of both runs
  int16_t split;       // first lane of run 1
  FastRun r[2];
};
static_assert(sizeof(FastWave) == 32, "read as eight dwords");
constexpr int kFastWaveLanes = 64;

struct LevelPlan {
  int32_t w, h;               // level size (cvRound(W / 1.2^l))
  int32_t pitch;              // row pitch of raw level l (level 0: the input width) and of
                              // the blurred level (all levels: align64(w))
  int32_t bpitch;
  int64_t pyr_off;            // offset of the level inside a frame's pyramid workspace (l >= 1)
  int64_t img_off;            // offset inside a frame's blurred-level workspace (pitch bpitch)
  int64_t mask_off;           // offset inside a mask pyramid (pitch bpitch: aligned dword loads)
  int32_t cell_begin, cell_end;
  int32_t cand_off, cand_cap; // candidate gather area within a frame (sum of cell caps)
  int32_t sel_off, sel_cap;   // octree output area within a frame
  int32_t nfeat;              // mnFeaturesPerLevel[l] (:167-179)
  int32_t nini;               // cvRound((maxX-minX)/(maxY-minY)) (:641)
  double hx;                  // (maxX-minX)/nIni (:643)
  int32_t width_rel, height_rel;  // maxX-minX, maxY-minY of the octree domain
  int32_t simd_end;           // first dx computed by the scalar vertical resize form
  int32_t wcell;              // FAST cell width (every cell but a clamped last one)
  int32_t patch_size_scaled;  // (int)(PATCH_SIZE * scaleFactor^l)  (:959)
  float scale;                // (float)mvScaleFactor[l]  (:1305)
};

struct Plan {
  mcs_extractor_params p;
  int32_t W = 0, H = 0, nlevels = 0;
  double scale_factor = 1.2;  // double((float)p.scale_factor)  (:147)
  LevelPlan lv[kMaxLevels];
  std::vector<CellDesc> cells;
  std::vector<FastUnit> fast_units;       // the runs of every cell row, sorted by level
  std::vector<FastWave> fast_waves;       // the same runs packed into waves (pack_fast_units)
  int32_t unit_begin[kMaxLevels + 1] = {};  // first unit of each level
  int64_t pyr_frame_bytes = 0;   // levels 1..L-1
  int64_t img_frame_bytes = 0;   // levels 0..L-1 (blurred levels, padded pitch)
  int64_t mask_frame_bytes = 0;  // levels 0..L-1 (mask pyramid, pitch bpitch)
  int32_t slots_per_frame = 0;   // sum of cell caps
  int32_t cand_per_frame = 0;    // == slots_per_frame
  int32_t sel_per_frame = 0;     // sum of level sel caps == mcs_extractor_capacity
  int32_t max_cells_level = 0;
  int32_t max_win_w = 0, max_win_h = 0;  // largest FAST window (LDS sizing)
  // resize tables (concatenated over levels 1..L-1)
  std::vector<int32_t> xofs, yofs;
  std::vector<int16_t> alpha, beta;
  std::vector<int64_t> xtab_off, ytab_off;  // per level offsets into the tables
};

// Returns MCS_OK or an error (unsupported geometry / parameters).
int build_plan(const mcs_extractor_params& p, int W, int H, Plan& plan);

// k_fast_rows units for frames of one registered mask (its host copy of the mask pyramid,
// plan layout).  A cell whose detection window holds no mask pixel emits nothing (runByPixels-
// Mask drops every keypoint; NMS never looks across a cell): such cells become `dead` units
// that only zero the cell's count, and each cell row's live range is re-split into the fewest
// runs (`live`), so a wave covers live cells only.
void build_masked_units(const Plan& pl, const uint8_t* mask_pyr, std::vector<FastUnit>& live,
                        std::vector<FastUnit>& dead);

// Lanes a run with detection columns [ux0, ux1) of `level` takes in a wave (see FastWave).
int fast_run_lanes(const Plan& pl, int level, int ux0, int ux1);

// The waves of k_fast_rows for `units` (the plan's fast_units, or a mask's live units followed
// by its dead ones; sorted by level, cell rows in order).  The runs of a cell row are merged
// back into the row's live range and re-cut greedily: a wave takes as many cells of the row as
// its lanes hold, and where a row ends with lanes to spare, the head of the next cell row of the
// same level and height goes into them as the wave's second run.  Never more waves on a level
// than units; count-zeroing units (wy1 <= wy0) become one wave each, in place.
void pack_fast_units(const Plan& pl, const std::vector<FastUnit>& units, std::vector<FastWave>& out);

}  // namespace mcs
