// Work units of the pyramid kernel (k_pyr_rows): which strips of which rows of each level a
// frame's waves compute.  Host code only (no device header), run at mask registration and on
// the first batch of a new size.
//
// Without a registered mask every pixel of every level is computed.  With one, a pixel is
// computed only where an output can depend on it: a keypoint exists only on a
// mask pixel inside a live FAST cell, IC_Angle and the rotated pattern stay within a fixed
// reach of it, and a level is otherwise only the source of the next one.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "extractor_plan.hpp"

namespace mcs {

// One strip of k_pyr_rows: output columns [x0, x0 + core) (cut at the level's width) of rows
// [row0, row0 + rows).  x0 and core are multiples of 4, core <= kPyrMaxCore, rows <= 64.
// The kernel reads the waves made of them (PyrWave below): a whole strip, or runs of the strips'
// span in two frames.
struct alignas(8) PyrUnit {
  int16_t x0, core, row0, rows;
};
constexpr int kPyrMaxCore = 244;   // 61 lanes x 4 px: a level-0 strip + halo is <= 64 dwords

#ifndef MCS_PYR_TARGET
#define MCS_PYR_TARGET 8192
#endif
#ifndef MCS_PYR_WAVES_PER_FRAME
#define MCS_PYR_WAVES_PER_FRAME 32
#endif
#ifndef MCS_PYR_MAXROWS
#define MCS_PYR_MAXROWS 64
#endif
#ifndef MCS_PYR_MINROWS
#define MCS_PYR_MINROWS 8
#endif
// strips of <= 244 columns; segment height chosen for ~32 waves per frame, at least 8k waves
// per launch (latency hiding for small batches), between 8 and 64 rows.  Per frame that is a
// fixed geometry, so the production step's two halves on two streams (bench.py --split 2: two
// launches of ~256 frames side by side) cut their segments as tall as one launch of the whole
// batch; a fixed 16k-wave target had halved the segments of a half (more halo rows per output
// row).  Round 6: 399 -> 410 M keypoints/s.
// (more waves per frame for the levels under 200 rows only, 48 or 64 with segments down to
// 6 / 4 rows, and segments down to 4 rows alone measured flat or slower at the end of round 6)
inline void pyr_strip_geometry(int dw, int dh, int F, int* core, int* tiles_x, int* seg_rows,
                               int* tiles_y) {
  const int n = (dw + kPyrMaxCore - 1) / kPyrMaxCore;
  *core = ((dw + n - 1) / n + 3) & ~3;
  *tiles_x = (dw + *core - 1) / *core;
  const long target = std::max<long>(MCS_PYR_TARGET, (long)MCS_PYR_WAVES_PER_FRAME * (F > 0 ? F : 1));
  const long per_seg = (long)*tiles_x * (F > 0 ? F : 1);
  const int segs = (int)std::max<long>(1, (target + per_seg - 1) / per_seg);
  int rows = (dh + segs - 1) / segs;
  rows = std::min(MCS_PYR_MAXROWS, std::max(MCS_PYR_MINROWS, rows));
  *seg_rows = rows;
  *tiles_y = (dh + rows - 1) / rows;
}
// The geometry depends on the batch size only below this many frames (target = 32 F from there)
constexpr int kPyrFrameClasses = (MCS_PYR_TARGET + MCS_PYR_WAVES_PER_FRAME - 1) / MCS_PYR_WAVES_PER_FRAME;
inline int pyr_frame_class(int F) { return std::min(std::max(F, 1), kPyrFrameClasses); }

// Largest distance (per axis, pixels) at which compute_ORB samples the blurred level around a
// keypoint: the largest radius of a pattern point, rounded up (a rotation keeps the radius,
// cvRound moves a coordinate to at most the next integer).
int pyr_pattern_reach();

// Per level and row, the columns [lo, hi) that must be computed (hi <= lo: none).
struct PyrNeed {
  std::vector<int16_t> lo, hi;              // rows of all levels, level l at row_off[l]
  int32_t row_off[kMaxLevels + 1] = {};
};

// The need sets of one registered mask (its host copy of the mask pyramid, plan layout) and the
// live FAST units build_masked_units made for it.
void build_pyr_need(const Plan& pl, const uint8_t* mask_pyr, const std::vector<FastUnit>& live,
                    PyrNeed& need);

// Units of every level for batches of F frames; need == nullptr: every pixel (then exactly the
// strips x segments of pyr_strip_geometry, segment-major).  With a need set: per segment the
// fewest strips over the columns its rows need, none for an empty segment, tall units first.
void build_pyr_units(const Plan& pl, const PyrNeed* need, int F,
                     std::vector<PyrUnit> (&lists)[kMaxLevels]);

// ---- second stage: strips of frames of one mask side by side in a wave
//
// A wave costs per row, not per column, and the strips of a level seldom fill its lanes
// (628 -> 3 x 212).  Frames of one mask share everything wave-uniform of a level's row segment,
// so the segment's span of G such frames ("slots") is laid end to end and cut into waves of one
// or two runs.  Run 0 takes lanes [0, r[0].core / 4 + 2), run 1 the lanes after them: each run
// has its own halo lane before and after its core, so no 5-sum crosses from one run into the
// other.  Run 1 (core > 0) always belongs to slot + 1.  rows == 0 pads a list: the wave exits
// without a store.  16 bytes, aligned: the kernel reads a wave with one scalar load (a 2-byte
// aligned struct would be read with vector loads).
struct PyrRun {
  int16_t x0, core;    // output columns [x0, x0 + core) (cut at the level's width), multiples of 4
};
struct alignas(16) PyrWave {
  int16_t row0, rows;  // of both runs
  int16_t slot;        // of run 0
  int16_t pad;
  PyrRun r[2];
};
static_assert(sizeof(PyrWave) == 16, "read as four dwords");
constexpr int kPyrMaxCore2 = kPyrMaxCore - 8;   // both cores of a two-run wave: a second halo pair
// frame slots per group: 4 takes most of what the count offers (17-19 % fewer waves
// with the Lafida masks, 8 slots 19-20 %) and leaves less of a batch in partly filled groups
#ifndef MCS_PYR_GROUP
#define MCS_PYR_GROUP 4
#endif
constexpr int kPyrGroup = MCS_PYR_GROUP;
constexpr int kPyrStageDW = 192;                // k_pyr_rows' staged source row (dwords)

// Source frames of level l as k_pyr_rows reads them: the input (levels 0 and 1) or level l - 1
inline int pyr_src_pitch(const Plan& pl, int l) { return l <= 1 ? pl.lv[0].pitch : pl.lv[l - 1].pitch; }
inline int64_t pyr_src_fstride(const Plan& pl, int l) { return l <= 1 ? (int64_t)pl.W * pl.H : pl.pyr_frame_bytes; }
inline int pyr_stage_ndw(const Plan& pl, int l) { return l == 0 ? 1 : (pl.scale_factor <= 1.5 ? 2 : 3); }
// Two runs share a wave only where their source bytes sit alike in their dwords, so that a
// row's byte shift is one value per wave: the frame stride must be a multiple of 4, and both
// runs of such a wave stage from their first source column rounded down to a multiple of 4.
// Where the source pitch is a multiple of 4 the staged dwords are counted from a byte shift of
// 0, that is from dword-aligned frames: the pyramid workspace is, and run_batch rejects input
// images that are not when W % 4 == 0.
inline bool pyr_level_packs(const Plan& pl, int l) { return pyr_src_fstride(pl, l) % 4 == 0; }

// Waves of every level for a group of G frame slots of one mask, from that mask's unit lists
// (build_pyr_units; tall units first, and so the waves).  Per row segment the span its units
// cover is cut greedily: a run takes what is left of its slot, at most kPyrMaxCore columns; where
// a slot ends with lanes to spare, the head of the next slot's span goes into them, as far as
// kPyrMaxCore2 and the wave's staged dwords (NDW x 64, kPyrStageDW) allow.  G == 1, or a level
// that does not pack: one run per wave.  A group with one frame present runs as many live waves
// as build_pyr_units has units for it.
void pack_pyr_units(const Plan& pl, const std::vector<PyrUnit> (&lists)[kMaxLevels], int G,
                    std::vector<PyrWave> (&waves)[kMaxLevels]);

}  // namespace mcs
