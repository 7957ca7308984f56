// The device part of cORBmatcher::Fuse (src/cORBmatcher.cpp:1265-1719) as plain single-thread
// C++: per (target, query, camera) the projection, mirror mask, distance window, predicted level,
// GetFeaturesInArea over the keyframe grid and the best-distance scan.  The CPU baseline of
// tools/bench_fuse.py, which also compares its best_kp with the device's.
//   fuse_cpu <in.bin> <out.bin> <repeats>   ->  "ms <best of repeats> hits <n>"
// in.bin: int32 {rule, use_dist, T, nq, C, bytes, L, mw, mh, th_low, n_kp_total}, double th, then
// off, kp_xy, kp_octave, kp_cam, desc, m_t, m_c, cam, mirror, grid_params, scale, q_pos, q_dist,
// q_desc as raw arrays.  out.bin: best_kp int32 [T][nq][C].
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 11);
  const int rule = h[0], use_dist = h[1], T = h[2], nq = h[3], C = h[4], B = h[5], L = h[6], mw = h[7], mh = h[8],
            th_low = h[9], ntot = h[10];
  const double th = rd<double>(f, 1)[0];
  const auto off = rd<int32_t>(f, T + 1);
  const auto xy = rd<float>(f, 2 * (size_t)ntot);
  const auto oct = rd<int32_t>(f, ntot);
  const auto kcam = rd<int32_t>(f, ntot);
  const auto desc = rd<uint8_t>(f, (size_t)ntot * B);
  const auto m_t = rd<double>(f, 16 * (size_t)T);
  const auto m_c = rd<double>(f, 16 * (size_t)C);
  const auto cam = rd<double>(f, 17 * (size_t)C);
  const auto mirror = rd<uint8_t>(f, (size_t)C * mw * mh);
  const auto gp = rd<double>(f, 4 * (size_t)C);
  const auto scale = rd<double>(f, L);
  const auto qpos = rd<double>(f, 3 * (size_t)nq);
  const auto qdist = rd<double>(f, 2 * (size_t)nq);
  const auto qdesc = rd<uint8_t>(f, (size_t)nq * B);
  std::fclose(f);
  const int COLS = 64, ROWS = 48;
  // the keyframe grids (part of the keyframe constructor, not timed)
  std::vector<std::vector<std::vector<int>>> grid(T, std::vector<std::vector<int>>((size_t)C * COLS * ROWS));
  for (int t = 0; t < T; t++)
    for (int k = off[t]; k < off[t + 1]; k++) {
      const int c = kcam[k];
      const float fx = xy[2 * k] - (float)gp[4 * c], fy = xy[2 * k + 1] - (float)gp[4 * c + 1];
      const int px = (int)std::lrint((double)fx * gp[4 * c + 2]), py = (int)std::lrint((double)fy * gp[4 * c + 3]);
      if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
      grid[t][((size_t)c * COLS + px) * ROWS + py].push_back(k - off[t]);
    }
  std::vector<int32_t> best_kp((size_t)T * nq * C);
  const int reps = std::atoi(argv[3]);
  double best_ms = 1e300;
  long hits = 0;
  for (int rep = 0; rep < reps; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    hits = 0;
    for (int t = 0; t < T; t++) {
      const double* Mt = &m_t[16 * (size_t)t];
      for (int c = 0; c < C; c++) {
        double M[12];   // rows 0..2 of M_t M_c
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += Mt[4 * i + k] * m_c[16 * (size_t)c + 4 * k + j];
            M[4 * i + j] = s;
          }
        double ti[3];
        for (int i = 0; i < 3; i++) ti[i] = -M[i] * M[3] + -M[4 + i] * M[7] + -M[8 + i] * M[11];
        const double* cm = &cam[17 * (size_t)c];
        for (int i = 0; i < nq; i++) {
          int32_t& out = best_kp[((size_t)t * nq + i) * C + c];
          out = -1;
          const double* P = &qpos[3 * (size_t)i];
          const double x = M[0] * P[0] + M[4] * P[1] + M[8] * P[2] + ti[0];
          const double y = M[1] * P[0] + M[5] * P[1] + M[9] * P[2] + ti[1];
          const double z = M[2] * P[0] + M[6] * P[1] + M[10] * P[2] + ti[2];
          double norm = std::sqrt(x * x + y * y);
          if (norm == 0.0) norm = 1e-14;
          const double theta = std::atan(-z / norm);
          double rho = 0;
          for (int k = 11; k >= 0; k--) rho = rho * theta + cm[5 + k];
          const double uu = x / norm * rho, vv = y / norm * rho;
          const double u = uu * cm[0] + vv * cm[1] + cm[3], v = uu * cm[2] + vv + cm[4];
          const int ur = (int)std::lrint(u), vr = (int)std::lrint(v);
          if (ur >= mw || ur <= 0 || vr >= mh || vr <= 0) continue;
          if (!mirror[(size_t)c * mw * mh + (size_t)vr * mw + ur]) continue;
          const double maxD = 1.2 * qdist[2 * i + 1], minD = 0.8 * qdist[2 * i];
          const double PO[3] = {P[0] - Mt[3], P[1] - Mt[7], P[2] - Mt[11]};
          double d = std::sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
          if (rule != 2) d = (double)(float)d;
          if (d < minD || d > maxD) continue;
          const double ratio = d / minD;
          int lv = (int)(std::lower_bound(scale.begin(), scale.end(), ratio) - scale.begin());
          lv = std::min(lv, L - 1);
          const double r = th * scale[lv];
          const double* g = &gp[4 * (size_t)c];
          int x0 = std::max(0, (int)std::floor((u - g[0] - r) * g[2]));
          if (x0 >= COLS) continue;
          int x1 = std::min(COLS - 1, (int)std::ceil((u - g[0] + r) * g[2]));
          if (x1 < 0) continue;
          int y0 = std::max(0, (int)std::floor((v - g[1] - r) * g[3]));
          if (y0 >= ROWS) continue;
          int y1 = std::min(ROWS - 1, (int)std::ceil((v - g[1] + r) * g[3]));
          if (y1 < 0) continue;
          int bd = INT_MAX, bi = -1;
          const uint64_t* qd = reinterpret_cast<const uint64_t*>(&qdesc[(size_t)i * B]);
          for (int ix = x0; ix <= x1; ix++)
            for (int iy = y0; iy <= y1; iy++)
              for (int k : grid[t][((size_t)c * COLS + ix) * ROWS + iy]) {
                const size_t gk = (size_t)off[t] + k;
                if (!(std::fabs((double)xy[2 * gk] - u) <= r && std::fabs((double)xy[2 * gk + 1] - v) <= r)) continue;
                if (oct[gk] < lv - 1 || oct[gk] > lv) continue;
                int dist = 0;
                if (use_dist) {
                  const uint64_t* kd = reinterpret_cast<const uint64_t*>(&desc[gk * B]);
                  for (int w = 0; w < B / 8; w++) dist += __builtin_popcountll(qd[w] ^ kd[w]);
                }
                if (dist < bd) { bd = dist; bi = k; }
              }
          if (bi >= 0 && bd <= th_low) { out = bi; hits++; }
        }
      }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    best_ms = std::min(best_ms, ms);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(best_kp.data(), sizeof(int32_t), best_kp.size(), o);
  std::fclose(o);
  std::printf("ms %.4f hits %ld\n", best_ms, hits);
  return 0;
}
