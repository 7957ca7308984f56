// Per-mask work units of the pyramid kernel (see pyr_units.hpp).  Host only.
#include "pyr_units.hpp"
#include <cmath>

namespace mcs {

namespace {

const int kPattern[2048] = {
#include "pattern_orb64.inc"
};

using Map = std::vector<uint8_t>;   // w x h, 0 / 1

// out |= in dilated by the (2r+1) x (2r+1) square, cut at the level
void dilate_or(const Map& in, int w, int h, int r, Map& out) {
  Map tmp((size_t)w * h, 0);
  std::vector<int> pre((size_t)std::max(w, h) + 1);
  for (int y = 0; y < h; y++) {
    const uint8_t* s = &in[(size_t)y * w];
    pre[0] = 0;
    for (int x = 0; x < w; x++) pre[x + 1] = pre[x] + (s[x] != 0);
    if (pre[w] == 0) continue;
    uint8_t* d = &tmp[(size_t)y * w];
    for (int x = 0; x < w; x++) d[x] = pre[std::min(w, x + r + 1)] - pre[std::max(0, x - r)] > 0;
  }
  for (int x = 0; x < w; x++) {
    pre[0] = 0;
    for (int y = 0; y < h; y++) pre[y + 1] = pre[y] + tmp[(size_t)y * w + x];
    if (pre[h] == 0) continue;
    for (int y = 0; y < h; y++)
      if (pre[std::min(h, y + r + 1)] - pre[std::max(0, y - r)] > 0) out[(size_t)y * w + x] = 1;
  }
}

}  // namespace

int pyr_pattern_reach() {
  double r2 = 0;
  for (int i = 0; i < 1024; i++)
    r2 = std::max(r2, (double)kPattern[2 * i] * kPattern[2 * i] + (double)kPattern[2 * i + 1] * kPattern[2 * i + 1]);
  return (int)std::ceil(std::sqrt(r2));
}

void build_pyr_need(const Plan& pl, const uint8_t* mask_pyr, const std::vector<FastUnit>& live,
                    PyrNeed& need) {
  const int nl = pl.nlevels;
  const int reach = pyr_pattern_reach();
  need.lo.clear(); need.hi.clear();
  int32_t rows = 0;
  for (int l = 0; l < nl; l++) { need.row_off[l] = rows; rows += pl.lv[l].h; }
  for (int l = nl; l <= kMaxLevels; l++) need.row_off[l] = rows;
  need.lo.assign(rows, 0); need.hi.assign(rows, 0);

  Map up;   // needR of level l + 1
  for (int l = nl - 1; l >= 0; l--) {
    const LevelPlan& L = pl.lv[l];
    const int w = L.w, h = L.h;
    // keypoint-capable pixels: mask != 0 inside a FAST cell's detection window (such a cell is
    // live; the windows of a cell row tile it without gaps)
    Map cap((size_t)w * h, 0);
    const uint8_t* m = mask_pyr + L.mask_off;
    for (int c = L.cell_begin; c < L.cell_end; c++) {
      const CellDesc& cd = pl.cells[c];
      for (int y = cd.wy0; y < cd.wy1; y++)
        for (int x = cd.wx0; x < cd.wx1; x++)
          if (m[(int64_t)y * L.bpitch + x]) cap[(size_t)y * w + x] = 1;
    }
    // blurred pixels compute_ORB can sample
    Map needB((size_t)w * h, 0);
    dilate_or(cap, w, h, reach, needB);
    // raw pixels: IC_Angle's patch (its circle lies in the +-kHalfPatch square) ...
    Map needR((size_t)w * h, 0);
    dilate_or(cap, w, h, kHalfPatch, needR);
    // ... every pixel a live FAST unit reads: its detection span and rows, +-3 ...
    for (const FastUnit& u : live) {
      if (u.level != l || u.wy1 <= u.wy0) continue;
      const int x0 = std::max(0, u.ux0 - 3), x1 = std::min(w, u.ux1 + 3);
      for (int y = std::max(0, u.wy0 - 3); y < std::min(h, u.wy1 + 3); y++)
        std::fill(needR.begin() + (size_t)y * w + x0, needR.begin() + (size_t)y * w + x1, 1);
    }
    // ... the raw +-2 window of every needed blurred pixel (a wave recomputes the raw halo of
    // its strip from the source level, so the halo's sources must hold) ...
    dilate_or(needB, w, h, 2, needR);
    // ... and the bilinear sources of the next level's raw pixels (both taps, clamped as
    // k_pyr_rows clamps them)
    if (l + 1 < nl) {
      const LevelPlan& U = pl.lv[l + 1];
      const int32_t* xofs = pl.xofs.data() + pl.xtab_off[l + 1];
      const int32_t* yofs = pl.yofs.data() + pl.ytab_off[l + 1];
      for (int y = 0; y < U.h; y++) {
        const int y0 = std::min(std::max(yofs[y], 0), h - 1), y1 = std::min(std::max(yofs[y] + 1, 0), h - 1);
        for (int x = 0; x < U.w; x++) {
          if (!up[(size_t)y * U.w + x]) continue;
          const int x0 = std::min(std::max(xofs[x], 0), w - 1), x1 = std::min(x0 + 1, w - 1);
          needR[(size_t)y0 * w + x0] = needR[(size_t)y0 * w + x1] = 1;
          needR[(size_t)y1 * w + x0] = needR[(size_t)y1 * w + x1] = 1;
        }
      }
    }
    // level 0 is the input: only its blur is computed
    const Map& span = l == 0 ? needB : needR;   // needB is inside needR
    for (int y = 0; y < h; y++) {
      int lo = w, hi = 0;
      const uint8_t* s = &span[(size_t)y * w];
      for (int x = 0; x < w; x++)
        if (s[x]) { lo = std::min(lo, x); hi = x + 1; }
      need.lo[need.row_off[l] + y] = (int16_t)lo;
      need.hi[need.row_off[l] + y] = (int16_t)hi;
    }
    up.swap(needR);
  }
}

void build_pyr_units(const Plan& pl, const PyrNeed* need, int F,
                     std::vector<PyrUnit> (&lists)[kMaxLevels]) {
  for (int l = 0; l < kMaxLevels; l++) lists[l].clear();
  for (int l = 0; l < pl.nlevels; l++) {
    const int w = pl.lv[l].w, h = pl.lv[l].h;
    int core, tiles_x, seg_rows, tiles_y;
    pyr_strip_geometry(w, h, F, &core, &tiles_x, &seg_rows, &tiles_y);
    std::vector<PyrUnit>& out = lists[l];
    for (int s = 0; s < tiles_y; s++) {
      const int r0 = s * seg_rows, r1 = std::min(h, r0 + seg_rows);
      if (!need) {
        for (int t = 0; t < tiles_x; t++)
          out.push_back(PyrUnit{(int16_t)(t * core), (int16_t)core, (int16_t)r0, (int16_t)(r1 - r0)});
        continue;
      }
      int lo = w, hi = 0;
      for (int y = r0; y < r1; y++) {
        const int a = need->lo[need->row_off[l] + y], b = need->hi[need->row_off[l] + y];
        if (b > a) { lo = std::min(lo, a); hi = std::max(hi, b); }
      }
      if (hi <= lo) continue;
      lo &= ~3;
      const int n = (hi - lo + kPyrMaxCore - 1) / kPyrMaxCore;
      const int c = ((hi - lo + n - 1) / n + 3) & ~3;
      for (int x = lo; x < hi; x += c)
        out.push_back(PyrUnit{(int16_t)x, (int16_t)c, (int16_t)r0, (int16_t)(r1 - r0)});
    }
    if (need)
      std::stable_sort(out.begin(), out.end(),
                       [](const PyrUnit& a, const PyrUnit& b) { return a.rows > b.rows; });
  }
}

namespace {

// Dwords a run stages per source row at most (k_pyr_rows c_lo / c_hi; the resize reads one
// byte past its last column).  Rows of a pitch that is no multiple of 4 start at any byte of a
// dword; otherwise the frames are dword aligned and the shift is that of the first column.
int run_stage_dw(const Plan& pl, int l, const PyrRun& r, bool two) {
  const int w = pl.lv[l].w;
  int c_lo, c_hi;
  if (l) {
    const int32_t* xofs = pl.xofs.data() + pl.xtab_off[l];
    c_lo = xofs[std::max(r.x0 - 4, 0)];
    c_hi = std::min(xofs[std::min(r.x0 + r.core + 3, w - 1)] + 1, pl.lv[l - 1].w - 1);
  } else {
    c_lo = std::max(r.x0 - 4, 0);
    c_hi = std::min(r.x0 + r.core + 3, w - 1);
  }
  if (two) c_lo &= ~3;
  const int shift = pyr_src_pitch(pl, l) % 4 == 0 ? (c_lo & 3) : 3;
  return (shift + (c_hi - c_lo + 1) + (l ? 1 : 0) + 3) >> 2;
}

}  // namespace

void pack_pyr_units(const Plan& pl, const std::vector<PyrUnit> (&lists)[kMaxLevels], int G,
                    std::vector<PyrWave> (&waves)[kMaxLevels]) {
  for (int l = 0; l < kMaxLevels; l++) waves[l].clear();
  for (int l = 0; l < pl.nlevels; l++) {
    const std::vector<PyrUnit>& in = lists[l];
    const int w = pl.lv[l].w;
    const bool packs = G > 1 && pyr_level_packs(pl, l);
    const int max_dw = std::min(64 * pyr_stage_ndw(pl, l), kPyrStageDW);
    for (size_t i = 0; i < in.size();) {
      // the units of one row segment are consecutive: their span [lo, hi)
      size_t j = i;
      int lo = in[i].x0, hi = in[i].x0 + in[i].core;
      for (; j < in.size() && in[j].row0 == in[i].row0 && in[j].rows == in[i].rows; j++) {
        lo = std::min<int>(lo, in[j].x0);
        hi = std::max<int>(hi, in[j].x0 + in[j].core);
      }
      const int len = (std::min(hi, w) - lo + 3) & ~3;
      int s = 0, x = lo;
      while (s < G) {
        PyrWave wv{in[i].row0, in[i].rows, (int16_t)s, 0, {{0, 0}, {0, 0}}};
        const int c0 = std::min(lo + len - x, kPyrMaxCore);
        wv.r[0] = PyrRun{(int16_t)x, (int16_t)c0};
        x += c0;
        if (x >= lo + len) {
          s++; x = lo;
          if (packs && s < G) {
            int c1 = std::min(len, kPyrMaxCore2 - c0) & ~3;
            while (c1 > 0 && run_stage_dw(pl, l, wv.r[0], true) +
                                 run_stage_dw(pl, l, PyrRun{(int16_t)lo, (int16_t)c1}, true) > max_dw)
              c1 -= 4;
            if (c1 > 0) {
              wv.r[1] = PyrRun{(int16_t)lo, (int16_t)c1};
              x = lo + c1;
              if (c1 >= len) { s++; x = lo; }
            }
          }
        }
        waves[l].push_back(wv);
      }
      i = j;
    }
  }
}

}  // namespace mcs
