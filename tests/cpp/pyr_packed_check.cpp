// CPU check of the second stage of the pyramid unit planner (pack_pyr_units, csrc/pyr_units.cpp)
// and of the frame grouping rule (csrc/pyr_groups.hpp) for tests/test_pyr_packed_units.py.
// Host code only: nothing here touches a device.
//
// Per case, batch-size class and group size G the packed waves must cover, slot by slot, exactly
// the pixels of the mask's unpacked units, and keep what k_pyr_rows needs of a wave: multiples
// of 4, both runs with their halo lanes inside 64 lanes, the staged source dwords of both runs
// inside NDW x 64 and the staging row, rows <= 64, and source bytes of both runs alike in
// their dwords.  All of it is restated here, not taken from the packer.
//
// Input file (argv[1]): per case five int32 (W, H, nlevels, scale as float32 bits, 1 = no mask)
// and W * H mask bytes.  Output: per case, G and level `waves <case> <G> <level> <unpacked per
// frame> <packed per group>` at 256 frames, `sort ok N`, then `ok cases N`.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../multicol-slam-annotation_amd/csrc/extractor_plan.hpp"
#include "../../multicol-slam-annotation_amd/csrc/pyr_groups.hpp"
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

// first staged source column and worst-case dwords of a run (k_pyr_rows' c_lo / c_hi)
static void staged(const Plan& pl, int l, int x0, int core, bool two, int* c_lo_out, int* dwords) {
  const int w = pl.lv[l].w;
  int c_lo, c_hi;
  if (l) {
    const int32_t* xofs = pl.xofs.data() + pl.xtab_off[l];
    c_lo = xofs[std::max(x0 - 4, 0)];
    c_hi = std::min(xofs[std::min(x0 + core + 3, w - 1)] + 1, pl.lv[l - 1].w - 1);
  } else {
    c_lo = std::max(x0 - 4, 0);
    c_hi = std::min(x0 + core + 3, w - 1);
  }
  if (two) c_lo -= c_lo % 4;
  const int pitch = l <= 1 ? pl.W : pl.lv[l - 1].pitch;
  const int shift = pitch % 4 ? 3 : c_lo % 4;
  *c_lo_out = c_lo;
  *dwords = (shift + (c_hi - c_lo + 1) + (l ? 1 : 0) + 3) / 4;   // resize reads column + 1
}

static void check_case(const Plan& pl, const PyrNeed* need, int ci) {
  const int nl = pl.nlevels;
  static const int kFrames[] = {1, 5, 64, 256};
  static const int kG[] = {1, 2, 4, 8};
  for (int F : kFrames) {
    std::vector<PyrUnit> units[kMaxLevels];
    build_pyr_units(pl, need, F, units);
    for (int G : kG) {
      std::vector<PyrWave> waves[kMaxLevels];
      pack_pyr_units(pl, units, G, waves);
      for (int l = 0; l < nl; l++) {
        const int w = pl.lv[l].w, h = pl.lv[l].h;
        const int ndw = l == 0 ? 1 : (pl.scale_factor <= 1.5 ? 2 : 3);
        const int64_t fstride = l <= 1 ? (int64_t)pl.W * pl.H : pl.pyr_frame_bytes;
        std::vector<uint8_t> want((size_t)w * h, 0);
        for (const PyrUnit& u : units[l])
          for (int y = u.row0; y < u.row0 + u.rows; y++)
            for (int x = u.x0; x < std::min(u.x0 + u.core, w); x++) want[(size_t)y * w + x] = 1;
        std::vector<uint8_t> got((size_t)G * w * h, 0);
        long slot0 = 0, two_runs = 0;
        for (size_t i = 0; i < waves[l].size(); i++) {
          const PyrWave& q = waves[l][i];
          const bool two = q.r[1].core > 0;
          two_runs += two;
          slot0 += q.slot == 0;
          REQUIRE(q.rows >= 1 && q.rows <= 64 && q.row0 >= 0 && q.row0 + q.rows <= h, "case %d F %d G %d l %d rows", ci, F, G, l);
          REQUIRE(q.slot >= 0 && q.slot + (two ? 1 : 0) < G, "case %d F %d G %d l %d slot %d", ci, F, G, l, q.slot);
          REQUIRE(i == 0 || waves[l][i - 1].rows >= q.rows, "case %d F %d G %d l %d not tall first", ci, F, G, l);
          int lanes = 0, dws = 0, c_lo[2] = {0, 0};
          for (int k = 0; k < (two ? 2 : 1); k++) {
            const PyrRun& r = q.r[k];
            REQUIRE(r.core > 0 && r.core % 4 == 0 && r.x0 % 4 == 0 && r.x0 >= 0 && r.x0 < w, "case %d F %d G %d l %d run %d,%d", ci, F, G, l, r.x0, r.core);
            if (g_fail) return;
            lanes += r.core / 4 + 2;   // halo lane before and after the core
            int d;
            staged(pl, l, r.x0, r.core, two, &c_lo[k], &d);
            dws += d;
            uint8_t* gs = &got[(size_t)(q.slot + k) * w * h];
            for (int y = q.row0; y < q.row0 + q.rows; y++)
              for (int x = r.x0; x < std::min(r.x0 + r.core, w); x++) {
                REQUIRE(gs[(size_t)y * w + x] == 0, "case %d F %d G %d l %d slot %d: %d,%d twice", ci, F, G, l, q.slot + k, x, y);
                gs[(size_t)y * w + x] = 1;
              }
          }
          REQUIRE(lanes <= 64, "case %d F %d G %d l %d lanes %d", ci, F, G, l, lanes);
          REQUIRE(dws <= 64 * ndw && dws <= 192, "case %d F %d G %d l %d staged dwords %d", ci, F, G, l, dws);
          if (two) {
            REQUIRE(q.r[0].core + q.r[1].core <= 236, "case %d F %d G %d l %d cores", ci, F, G, l);
            // any later frame may sit in the next slot
            for (int64_t df = 1; df <= 5; df++)
              REQUIRE((df * fstride + c_lo[1] - c_lo[0]) % 4 == 0, "case %d F %d G %d l %d: runs not congruent", ci, F, G, l);
          } else {
            REQUIRE(q.r[0].core <= 244 && q.r[1].core == 0, "case %d F %d G %d l %d core", ci, F, G, l);
          }
        }
        for (int s = 0; s < G; s++)
          REQUIRE(std::memcmp(&got[(size_t)s * w * h], want.data(), want.size()) == 0,
                  "case %d F %d G %d l %d slot %d: packed runs cover other pixels than the units", ci, F, G, l, s);
        // a frame alone in its group costs what it costs unpacked
        REQUIRE(slot0 == (long)units[l].size(), "case %d F %d G %d l %d: %ld waves for slot 0, %zu units", ci, F, G, l, slot0, units[l].size());
        if (G == 1) REQUIRE(two_runs == 0, "case %d l %d: two runs with one slot", ci, l);
        if (fstride % 4) REQUIRE(two_runs == 0, "case %d F %d G %d l %d: packed over a frame stride of %lld", ci, F, G, l, (long long)fstride);
        if (F == 256 && G > 1)
          std::printf("waves %d %d %d %zu %zu\n", ci, G, l, units[l].size(), waves[l].size());
      }
      if (g_fail) return;
    }
  }
}

// ---- the grouping rule against a plain restatement
static void check_sort(const std::vector<int32_t>& mi, bool null_index, int nmasks, int G, int ti) {
  const int F = (int)mi.size();
  const int ng = pyr_groups_max(F, G, nmasks);
  std::vector<int32_t> gf((size_t)ng * G, 12345), gm(ng, 12345), scratch(nmasks, 12345);
  pyr_group_frames(null_index ? nullptr : mi.data(), F, nmasks, G, gf.data(), gm.data(), scratch.data());
  // restated: per mask in order, its frames in order, G to a group
  std::vector<std::vector<int32_t>> exp;
  std::vector<int32_t> exp_mask;
  for (int m = 0; m < nmasks; m++) {
    std::vector<int32_t> mine;
    for (int f = 0; f < F; f++) {
      const int v = null_index ? 0 : std::min(std::max(mi[f], 0), nmasks - 1);
      if (v == m) mine.push_back(f);
    }
    for (size_t i = 0; i < mine.size(); i += G) {
      exp.emplace_back(mine.begin() + i, mine.begin() + std::min(mine.size(), i + G));
      exp_mask.push_back(m);
    }
  }
  REQUIRE((int)exp.size() <= ng, "sort %d: %zu groups, room for %d", ti, exp.size(), ng);
  std::vector<int> seen(F, 0), partial(nmasks, 0);
  for (int g = 0; g < ng; g++) {
    int n = 0;
    for (int s = 0; s < G; s++) {
      const int f = gf[(size_t)g * G + s];
      const int e = g < (int)exp.size() && s < (int)exp[g].size() ? exp[g][s] : -1;
      REQUIRE(f == e, "sort %d G %d: group %d slot %d holds %d, expected %d", ti, G, g, s, f, e);
      if (f < 0) continue;
      REQUIRE(f < F && s == n, "sort %d G %d: group %d slot %d", ti, G, g, s);   // no hole before a frame
      if (f >= F) return;
      n++;
      seen[f]++;
      const int v = null_index ? 0 : std::min(std::max(mi[f], 0), nmasks - 1);
      REQUIRE(v == gm[g], "sort %d G %d: frame %d of mask %d in a group of mask %d", ti, G, f, v, gm[g]);
      if (s) REQUIRE(gf[(size_t)g * G + s - 1] < f, "sort %d G %d: group %d not ascending", ti, G, g);
    }
    if (g < (int)exp.size()) REQUIRE(gm[g] == exp_mask[g], "sort %d G %d: group %d mask", ti, G, g);
    else REQUIRE(gm[g] >= 0 && gm[g] < nmasks, "sort %d G %d: empty group %d mask %d", ti, G, g, gm[g]);
    if (n > 0 && n < G) partial[gm[g]]++;
  }
  for (int f = 0; f < F; f++) REQUIRE(seen[f] == 1, "sort %d G %d: frame %d appears %d times", ti, G, f, seen[f]);
  for (int m = 0; m < nmasks; m++) REQUIRE(partial[m] <= 1, "sort %d G %d: mask %d has %d partial groups", ti, G, m, partial[m]);
}

static int check_sorts() {
  std::vector<std::vector<int32_t>> arrays;
  arrays.push_back({0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2});          // sorted
  arrays.push_back({0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0});          // interleaved
  arrays.push_back(std::vector<int32_t>(11, 1));                       // all equal
  arrays.push_back({2, 0, 1});                                         // all different
  arrays.push_back({0, -1, 2, 7, 1, -1, 7, 1, 0});                     // clamped at both ends
  arrays.push_back({2});                                               // F = 1
  arrays.push_back({0, 1, 2, 1, 0});
  std::vector<int32_t> big(513);                                       // the flagship's batch
  for (int f = 0; f < 513; f++) big[f] = f % 3;
  arrays.push_back(big);
  std::vector<int32_t> lcg(77);
  uint32_t s = 12345;
  for (auto& v : lcg) { s = s * 1664525u + 1013904223u; v = (int32_t)((s >> 24) % 5) - 1; }
  arrays.push_back(lcg);
  int n = 0;
  for (size_t a = 0; a < arrays.size(); a++)
    for (int G : {1, 2, 3, 4, 8})                                      // F is no multiple of most
      for (int nmasks : {1, 3, 4}) {
        check_sort(arrays[a], false, nmasks, G, (int)a);
        check_sort(arrays[a], true, nmasks, G, (int)a);                // no index: consecutive frames
        n += 2;
      }
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  const int nsort = check_sorts();
  if (!g_fail) std::printf("sort ok %d\n", nsort);
  int32_t hdr[5];
  int ci = 0;
  for (; !g_fail && std::fread(hdr, 4, 5, fp) == 5; ci++) {
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
    if (hdr[4]) { check_case(pl, nullptr, ci); continue; }
    // mask pyramid: cv::resize(INTER_NEAREST) chain (k_mask_nearest), plan layout
    std::vector<uint8_t> mp((size_t)pl.mask_frame_bytes, 0);
    for (int y = 0; y < H; y++) std::memcpy(&mp[(size_t)y * pl.lv[0].bpitch], &mask[(size_t)y * W], W);
    for (int l = 1; l < pl.nlevels; l++) {
      const LevelPlan& S = pl.lv[l - 1];
      const LevelPlan& D = pl.lv[l];
      const double ifx = 1. / ((double)D.w / S.w), ify = 1. / ((double)D.h / S.h);
      for (int y = 0; y < D.h; y++)
        for (int x = 0; x < D.w; x++) {
          const int sx = std::min((int)(x * ifx), S.w - 1), sy = std::min((int)(y * ify), S.h - 1);
          mp[D.mask_off + (size_t)y * D.bpitch + x] = mp[S.mask_off + (size_t)sy * S.bpitch + sx];
        }
    }
    std::vector<FastUnit> live, dead;
    build_masked_units(pl, mp.data(), live, dead);
    PyrNeed need;
    build_pyr_need(pl, mp.data(), live, need);
    check_case(pl, &need, ci);
  }
  std::fclose(fp);
  if (g_fail) { std::printf("failed %d\n", g_fail); return 1; }
  std::printf("ok cases %d\n", ci);
  return 0;
}
