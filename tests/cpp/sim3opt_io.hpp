// The case file of tests/sim3opt_cases.py and the result lines both programs print
// (sim3opt_host.cpp over csrc/sim3_opt_math.hpp, sim3opt_g2o_driver.cpp over the reference's
// g2o).  A case is whitespace-separated numbers, doubles as %.17g:
//   T n1 C L flags
//   std_sim its_round1 its_clean its_culled terminate_max_iter gain_threshold tau max_trials
//   KF1: n1 x (x y octave cam), m_t 16, pos n1 x 3, ok1 n1
//   m_c C x 16, cam C x 17, inv_sigma2_1 L, sigma2_2 L
//   per candidate: n2, n2 x (x y octave cam), m_t 16, pos n2 x 3, ok2 n2, first2 n2,
//                  matches12 n1, s12, R12 9, t12 3
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace s3io {

struct Kf {
  int n = 0;
  std::vector<float> xy;
  std::vector<int32_t> oct, cam;
  double m_t[16];
  std::vector<double> pos;
};

struct Cand {
  Kf kf;
  std::vector<uint8_t> ok2;
  std::vector<int32_t> first2, matches12;
  double s, R[9], t[3];
};

struct Case {
  int T = 0, n1 = 0, C = 0, L = 0, flags = 0;
  double std_sim, gain, tau;
  int its1, its_clean, its_culled, term_max, max_trials;
  Kf kf1;
  std::vector<uint8_t> ok1;
  std::vector<double> m_c, cam, inv_sigma2_1, sigma2_2;
  std::vector<Cand> cands;
};

struct Reader {
  FILE* f;
  bool ok = true;
  double d() { double v = 0; if (std::fscanf(f, "%lf", &v) != 1) ok = false; return v; }
  int i() { return (int)d(); }
  void kf(Kf& k, int n) {
    k.n = n; k.xy.resize(2 * n); k.oct.resize(n); k.cam.resize(n); k.pos.resize(3 * n);
    for (int j = 0; j < n; j++) { k.xy[2 * j] = (float)d(); k.xy[2 * j + 1] = (float)d(); k.oct[j] = i(); k.cam[j] = i(); }
    for (double& v : k.m_t) v = d();
    for (double& v : k.pos) v = d();
  }
};

inline bool read_case(const char* path, Case& c) {
  Reader r{std::fopen(path, "r")};
  if (!r.f) return false;
  c.T = r.i(); c.n1 = r.i(); c.C = r.i(); c.L = r.i(); c.flags = r.i();
  c.std_sim = r.d(); c.its1 = r.i(); c.its_clean = r.i(); c.its_culled = r.i(); c.term_max = r.i();
  c.gain = r.d(); c.tau = r.d(); c.max_trials = r.i();
  if (!r.ok || c.T < 0 || c.T > 64 || c.n1 < 0 || c.n1 > (1 << 19) || c.C < 1 || c.C > 8 || c.L < 1 || c.L > 64) {
    std::fclose(r.f);
    return false;
  }
  r.kf(c.kf1, c.n1);
  c.ok1.resize(c.n1);
  for (auto& v : c.ok1) v = (uint8_t)r.i();
  c.m_c.resize(16 * c.C); c.cam.resize(17 * c.C); c.inv_sigma2_1.resize(c.L); c.sigma2_2.resize(c.L);
  for (double& v : c.m_c) v = r.d();
  for (double& v : c.cam) v = r.d();
  for (double& v : c.inv_sigma2_1) v = r.d();
  for (double& v : c.sigma2_2) v = r.d();
  c.cands.resize(c.T);
  for (Cand& k : c.cands) {
    const int n2 = r.i();
    if (!r.ok || n2 < 0 || n2 > (1 << 19)) { std::fclose(r.f); return false; }
    r.kf(k.kf, n2);
    k.ok2.resize(n2); k.first2.resize(n2); k.matches12.resize(c.n1);
    for (auto& v : k.ok2) v = (uint8_t)r.i();
    for (auto& v : k.first2) v = r.i();
    for (auto& v : k.matches12) v = r.i();
    k.s = r.d();
    for (double& v : k.R) v = r.d();
    for (double& v : k.t) v = r.d();
  }
  std::fclose(r.f);
  return r.ok;
}

// one candidate's result, one line per field
struct Out {
  int n_in = 0, n_corr = 0, n_bad = 0, n_undefined = 0;
  double s = 0, q[4] = {0, 0, 0, 0}, t[3] = {0, 0, 0};
  int iters[2] = {0, 0};
  double chi2[2] = {0, 0}, lambda[2] = {0, 0};
  int trials[2][16] = {};
  std::vector<int32_t> matches12;
  std::vector<double> edge_chi2;   // [n1][2]
  std::vector<double> edge_chi2_r1;   // [n1][2] after round 1 (the driver's, for the generator's margin check)
};

inline void print_out(int t, const Out& o) {
  std::printf("cand %d\n", t);
  std::printf("counts %d %d %d %d\n", o.n_in, o.n_corr, o.n_bad, o.n_undefined);
  std::printf("sim3 %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", o.s, o.q[0], o.q[1], o.q[2], o.q[3], o.t[0],
              o.t[1], o.t[2]);
  std::printf("iters %d %d\n", o.iters[0], o.iters[1]);
  std::printf("chi2 %.17g %.17g\n", o.chi2[0], o.chi2[1]);
  std::printf("lambda %.17g %.17g\n", o.lambda[0], o.lambda[1]);
  for (int r = 0; r < 2; r++) {
    std::printf("trials%d", r);
    for (int k = 0; k < 16; k++) std::printf(" %d", o.trials[r][k]);
    std::printf("\n");
  }
  std::printf("matches");
  for (int32_t m : o.matches12) std::printf(" %d", m);
  std::printf("\nedge_chi2");
  for (double v : o.edge_chi2) std::printf(" %.17g", v);
  std::printf("\n");
  if (!o.edge_chi2_r1.empty()) {
    std::printf("edge_chi2_r1");
    for (double v : o.edge_chi2_r1) std::printf(" %.17g", v);
    std::printf("\n");
  }
}

}  // namespace s3io
