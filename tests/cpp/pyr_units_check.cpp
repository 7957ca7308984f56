// CPU check of the pyramid unit planner (csrc/pyr_units.cpp) for tests/test_pyr_mask_units.py.
// Host code only: nothing here touches a device.
//
// For every mask the program simulates, on its own and without the planner's need sets, which
// pixels can influence an output: from every mask pixel inside a live FAST cell it marks what
// FAST (with its 3x3 non-maximum suppression inside the cell), IC_Angle and the rotated pattern
// read there, the raw +-2 window of every blurred read, and the four bilinear sources level by
// level.  Every marked pixel must lie in the output rectangle of a unit of its level, and every
// source of a marked raw pixel must be written or be the input.  The units themselves must
// keep the kernel's bounds, and the unmasked table must be today's strips x segments.
//
// Input file (argv[1]): per case five int32 (W, H, nlevels, scale as float32 bits, print flag)
// and W * H mask bytes.  Output: per case and level `waves <case> <level> <w> <h> <full>
// <masked>` at 256 frames, then `ok cases N`.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../multicol-slam-annotation_amd/csrc/extractor_plan.hpp"
#include "../../multicol-slam-annotation_amd/csrc/pyr_units.hpp"

namespace mcs {
void set_error(const char*) {}
}  // namespace mcs

using namespace mcs;

static int g_fail = 0;
#define REQUIRE(cond, ...)                                              \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (g_fail < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
      g_fail++;                                                         \
    }                                                                   \
  } while (0)

static const int kPat[2048] = {
#include "../../multicol-slam-annotation_amd/csrc/pattern_orb64.inc"
};

// rows x (w + 1) difference array: mark(y, x0, x1) adds the run [x0, x1], cut at the level
struct Marks {
  int w, h;
  std::vector<int> d;
  Marks(int w_, int h_) : w(w_), h(h_), d((size_t)(w_ + 1) * h_, 0) {}
  void mark(int y, int x0, int x1) {
    if (y < 0 || y >= h) return;
    x0 = std::max(x0, 0); x1 = std::min(x1, w - 1);
    if (x0 > x1) return;
    d[(size_t)y * (w + 1) + x0]++;
    d[(size_t)y * (w + 1) + x1 + 1]--;
  }
  void into(std::vector<uint8_t>& out) const {   // out |= marked
    for (int y = 0; y < h; y++) {
      int acc = 0;
      for (int x = 0; x < w; x++) {
        acc += d[(size_t)y * (w + 1) + x];
        if (acc > 0) out[(size_t)y * w + x] = 1;
      }
    }
  }
};

// pyr_strips as it stood before the unit table (extractor_kernels.hpp), restated
static void old_strips(int dw, int dh, int F, int* core, int* tiles_x, int* seg_rows, int* tiles_y) {
  const int n = (dw + 243) / 244;
  *core = ((dw + n - 1) / n + 3) & ~3;
  *tiles_x = (dw + *core - 1) / *core;
  const long target = std::max<long>(8192, 32L * F);
  const long per_seg = (long)*tiles_x * F;
  const int segs = (int)std::max<long>(1, (target + per_seg - 1) / per_seg);
  *seg_rows = std::min(64, std::max(8, (dh + segs - 1) / segs));
  *tiles_y = (dh + *seg_rows - 1) / *seg_rows;
}

static void check_units(const Plan& pl, int l, const std::vector<PyrUnit>& units, int ci, int F,
                        std::vector<uint8_t>& written) {
  const int w = pl.lv[l].w, h = pl.lv[l].h;
  written.assign((size_t)w * h, 0);
  const int ndw = l == 0 ? 1 : (pl.scale_factor <= 1.5 ? 2 : 3);
  for (const PyrUnit& u : units) {
    REQUIRE(u.core % 4 == 0 && u.x0 % 4 == 0 && u.core > 0 && u.core <= 244, "case %d F %d l %d core %d x0 %d", ci, F, l, u.core, u.x0);
    REQUIRE(u.rows >= 1 && u.rows <= 64 && u.rows + 4 <= 128, "case %d F %d l %d rows %d", ci, F, l, u.rows);
    REQUIRE(u.x0 >= 0 && u.x0 < w && u.row0 >= 0 && u.row0 + u.rows <= h, "case %d F %d l %d unit outside", ci, F, l);
    if (g_fail) return;
    // staged source row of the wave (k_pyr_rows c_lo / c_hi): inside NDW dwords per lane
    int c_lo, c_hi;
    if (l) {
      const int32_t* xofs = pl.xofs.data() + pl.xtab_off[l];
      c_lo = xofs[std::max(u.x0 - 4, 0)];
      c_hi = std::min(xofs[std::min(u.x0 + u.core + 3, w - 1)] + 1, pl.lv[l - 1].w - 1);
    } else {
      c_lo = std::max(u.x0 - 4, 0);
      c_hi = std::min(u.x0 + u.core + 3, w - 1);
    }
    REQUIRE(c_lo <= c_hi && 3 + (c_hi - c_lo + 1) + (l ? 1 : 0) <= 256 * ndw, "case %d l %d staged %d..%d", ci, l, c_lo, c_hi);
    for (int y = u.row0; y < u.row0 + u.rows; y++)
      for (int x = u.x0; x < std::min(u.x0 + u.core, w); x++) {
        REQUIRE(written[(size_t)y * w + x] == 0, "case %d F %d l %d units overlap at %d,%d", ci, F, l, x, y);
        written[(size_t)y * w + x] = 1;
      }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  // IC_Angle's circle (ctor :187-202) and the pattern's radius, from the reference's own rules
  int umax[kHalfPatch + 2] = {};
  {
    int v, v0, vmax = (int)std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1);
    int vmin = (int)std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (v = 0; v <= vmax; ++v) umax[v] = (int)std::lrint(std::sqrt(hp2 - v * v));
    for (v = kHalfPatch, v0 = 0; v >= vmin; --v) {
      while (umax[v0] == umax[v0 + 1]) ++v0;
      umax[v] = v0;
      ++v0;
    }
  }
  double rmax = 0;
  for (int i = 0; i < 1024; i++) rmax = std::max(rmax, std::hypot((double)kPat[2 * i], (double)kPat[2 * i + 1]));
  // a rotated pattern point keeps its radius rmax: cvRound takes a coordinate to at most
  // floor(rmax + 0.5), and the rounded point at most sqrt(2) / 2 further out
  const int R = (int)std::floor(rmax + 0.5);
  const double disc2 = (rmax + 0.70711) * (rmax + 0.70711);
  REQUIRE(R <= 21, "pattern reach %d, k_orient_desc stages +-21", R);
  REQUIRE(pyr_pattern_reach() >= R && pyr_pattern_reach() == (int)std::ceil(rmax), "pyr_pattern_reach %d", pyr_pattern_reach());

  int32_t hdr[5];
  int ci = 0;
  for (; std::fread(hdr, 4, 5, fp) == 5; ci++) {
    const int W = hdr[0], H = hdr[1];
    std::vector<uint8_t> mask((size_t)W * H);
    if (std::fread(mask.data(), 1, mask.size(), fp) != mask.size()) return 2;
    mcs_extractor_params p;
    std::memset(&p, 0, sizeof(p));
    p.nfeatures = 500; p.nlevels = hdr[2]; p.fast_threshold = 20; p.fast_agast_type = 2; p.desc_size = 32;
    std::memcpy(&p.scale_factor, &hdr[3], 4);
    Plan pl;
    const int rc = build_plan(p, W, H, pl);
    REQUIRE(rc == 0, "case %d build_plan %d", ci, rc);
    if (rc) continue;
    const int nl = pl.nlevels;
    // mask pyramid: cv::resize(INTER_NEAREST) chain (k_mask_nearest), plan layout
    std::vector<uint8_t> mp((size_t)pl.mask_frame_bytes, 0);
    for (int y = 0; y < H; y++) std::memcpy(&mp[(size_t)y * pl.lv[0].bpitch], &mask[(size_t)y * W], W);
    for (int l = 1; l < nl; l++) {
      const LevelPlan& S = pl.lv[l - 1];
      const LevelPlan& D = pl.lv[l];
      const double ifx = 1. / ((double)D.w / S.w), ify = 1. / ((double)D.h / S.h);
      for (int y = 0; y < D.h; y++)
        for (int x = 0; x < D.w; x++) {
          const int sx = std::min((int)std::floor(x * ifx), S.w - 1), sy = std::min((int)std::floor(y * ify), S.h - 1);
          mp[D.mask_off + (size_t)y * D.bpitch + x] = mp[S.mask_off + (size_t)sy * S.bpitch + sx];
        }
    }

    // ---- what can influence an output
    std::vector<std::vector<uint8_t>> rawM(nl), blurM(nl);
    bool any_cap = false;
    for (int l = 0; l < nl; l++) {
      const LevelPlan& L = pl.lv[l];
      Marks mr(L.w, L.h), mb(L.w, L.h);
      const uint8_t* m = &mp[L.mask_off];
      for (int c = L.cell_begin; c < L.cell_end; c++) {
        const CellDesc& cd = pl.cells[c];
        for (int y = cd.wy0; y < cd.wy1; y++)
          for (int x = cd.wx0; x < cd.wx1; x++) {
            if (!m[(size_t)y * L.bpitch + x]) continue;
            any_cap = true;
            // FAST at the pixel and at its 8 neighbours inside the cell (NMS), circle radius 3
            for (int yy = std::max(y - 1, (int)cd.wy0); yy <= std::min(y + 1, cd.wy1 - 1); yy++)
              for (int dy = -3; dy <= 3; dy++)
                mr.mark(yy + dy, std::max(x - 1, (int)cd.wx0) - 3, std::min(x + 1, cd.wx1 - 1) + 3);
            for (int v = -kHalfPatch; v <= kHalfPatch; v++) mr.mark(y + v, x - umax[std::abs(v)], x + umax[std::abs(v)]);
            for (int dy = -R; dy <= R; dy++) {
              int e = R;
              while (e >= 0 && (double)e * e + (double)dy * dy > disc2) e--;
              if (e >= 0) mb.mark(y + dy, x - e, x + e);
            }
          }
      }
      rawM[l].assign((size_t)L.w * L.h, 0);
      blurM[l].assign((size_t)L.w * L.h, 0);
      mb.into(blurM[l]);
      // the blur's 5x5 raw window (its BORDER_REFLECT_101 mirrors lie inside the cut window)
      for (int y = 0; y < L.h; y++)
        for (int x = 0; x < L.w; x++)
          if (blurM[l][(size_t)y * L.w + x])
            for (int dy = -2; dy <= 2; dy++) mr.mark(y + dy, x - 2, x + 2);
      mr.into(rawM[l]);
    }
    auto taps = [&](int l, int x, int y, int (&sx)[2], int (&sy)[2]) {   // sources of (x, y) of level l
      const int sw = pl.lv[l - 1].w, sh = pl.lv[l - 1].h;
      const int xo = pl.xofs[pl.xtab_off[l] + x], yo = pl.yofs[pl.ytab_off[l] + y];
      sx[0] = std::min(std::max(xo, 0), sw - 1); sx[1] = std::min(std::max(xo + 1, 0), sw - 1);
      sy[0] = std::min(std::max(yo, 0), sh - 1); sy[1] = std::min(std::max(yo + 1, 0), sh - 1);
    };
    for (int l = nl - 1; l >= 1; l--)
      for (int y = 0; y < pl.lv[l].h; y++)
        for (int x = 0; x < pl.lv[l].w; x++) {
          if (!rawM[l][(size_t)y * pl.lv[l].w + x]) continue;
          int sx[2], sy[2];
          taps(l, x, y, sx, sy);
          for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) rawM[l - 1][(size_t)sy[a] * pl.lv[l - 1].w + sx[b]] = 1;
        }

    // ---- the planner's units
    std::vector<FastUnit> live, dead;
    build_masked_units(pl, mp.data(), live, dead);
    PyrNeed need;
    build_pyr_need(pl, mp.data(), live, need);
    static const int kFrames[] = {1, 5, 64, 255, 256, 513};
    for (int F : kFrames) {
      std::vector<PyrUnit> full[kMaxLevels], mk[kMaxLevels];
      build_pyr_units(pl, nullptr, F, full);
      build_pyr_units(pl, &need, F, mk);
      std::vector<std::vector<uint8_t>> wr(nl);
      for (int l = 0; l < nl; l++) {
        const int w = pl.lv[l].w, h = pl.lv[l].h;
        // unmasked: today's strips x segments, unit for unit
        int core, tx, sr, ty;
        old_strips(w, h, F, &core, &tx, &sr, &ty);
        REQUIRE((int)full[l].size() == tx * ty, "case %d F %d l %d: %zu units, %d x %d", ci, F, l, full[l].size(), tx, ty);
        for (int u = 0; u < tx * ty && u < (int)full[l].size(); u++) {
          const PyrUnit& q = full[l][u];
          const int r0 = (u / tx) * sr;
          REQUIRE(q.x0 == (u % tx) * core && q.core == core && q.row0 == r0 && q.rows == std::min(h, r0 + sr) - r0,
                  "case %d F %d l %d unit %d differs from pyr_strips", ci, F, l, u);
        }
        std::vector<uint8_t> wf;
        check_units(pl, l, full[l], ci, F, wf);
        REQUIRE(std::count(wf.begin(), wf.end(), 1) == (long)w * h, "case %d F %d l %d full table leaves pixels", ci, F, l);
        check_units(pl, l, mk[l], ci, F, wr[l]);
        for (size_t i = 1; i < mk[l].size(); i++)
          REQUIRE(mk[l][i - 1].rows >= mk[l][i].rows, "case %d F %d l %d not tall units first", ci, F, l);
        if (!any_cap) REQUIRE(mk[l].empty(), "case %d l %d: units for an empty mask", ci, l);
        if (F == 256)
          std::printf("waves %d %d %d %d %zu %zu\n", ci, l, w, h, full[l].size(), mk[l].size());
      }
      if (g_fail) break;
      for (int l = 0; l < nl; l++) {
        const int w = pl.lv[l].w, h = pl.lv[l].h;
        long missB = 0, missR = 0, missS = 0;
        for (int y = 0; y < h; y++)
          for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            if (blurM[l][i] && !wr[l][i]) missB++;
            if (l >= 1 && rawM[l][i]) {
              if (!wr[l][i]) missR++;
              if (l >= 2) {
                int sx[2], sy[2];
                taps(l, x, y, sx, sy);
                for (int a = 0; a < 2; a++)
                  for (int b = 0; b < 2; b++)
                    if (!wr[l - 1][(size_t)sy[a] * pl.lv[l - 1].w + sx[b]]) missS++;
              }
            }
          }
        REQUIRE(missB == 0 && missR == 0 && missS == 0, "case %d F %d l %d: %ld blurred, %ld raw, %ld source pixels not written",
                ci, F, l, missB, missR, missS);
      }
    }
  }
  std::fclose(fp);
  if (g_fail) { std::printf("failed %d\n", g_fail); return 1; }
  std::printf("ok cases %d\n", ci);
  return 0;
}
