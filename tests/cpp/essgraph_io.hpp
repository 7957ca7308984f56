// The text form of one case of tests/essgraph_cases.py (write_case_file) and of the result lines
// (parse_results), shared by essgraph_g2o_driver.cpp and essgraph_host.cpp.
//
//   N P cur loop min_weight iterations terminate_max_iter max_trials gain lambda0
//   N lines   id parent has_corrected  Scw (s qw qx qy qz tx ty tz)  Snc (likewise)
//   N lines   n  l_0 .. l_n-1                  loop edges (keyframe indices)
//   N lines   n  c_0 w_0 .. c_n-1 w_n-1        covisible neighbours and weights
//   N lines   n  j_0 w_0 .. j_n-1 w_n-1        LoopConnections with GetWeight
//   P lines   x y z corrected_by corrected_ref ref_kf bad      (keyframe ids)
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

namespace egio {

struct Case {
  int N = 0, P = 0, cur = 0, loop = 0, min_weight = 100, iterations = 20, term_max = 15, max_trials = 10;
  double gain = 1e-6, lambda0 = 1e-6;
  std::vector<int64_t> id;
  std::vector<int32_t> parent, has_corr;
  std::vector<double> Scw, Snc;                       // [N][8]
  std::vector<int32_t> loop_ptr, loop_idx, cov_ptr, cov_idx, cov_w, lc_ptr, lc_idx, lc_w;
  std::vector<double> pos;                            // [P][3]
  std::vector<int64_t> corrected_by, corrected_ref, ref_kf;
  std::vector<int32_t> bad;
};

inline bool read_case(const char* path, Case& c) {
  std::ifstream f(path);
  if (!f) return false;
  f >> c.N >> c.P >> c.cur >> c.loop >> c.min_weight >> c.iterations >> c.term_max >> c.max_trials >> c.gain >>
      c.lambda0;
  c.id.resize(c.N); c.parent.resize(c.N); c.has_corr.resize(c.N);
  c.Scw.resize(8 * (size_t)c.N); c.Snc.resize(8 * (size_t)c.N);
  for (int i = 0; i < c.N; i++) {
    f >> c.id[i] >> c.parent[i] >> c.has_corr[i];
    for (int k = 0; k < 8; k++) f >> c.Scw[8 * i + k];
    for (int k = 0; k < 8; k++) f >> c.Snc[8 * i + k];
  }
  auto csr = [&](std::vector<int32_t>& ptr, std::vector<int32_t>& idx, std::vector<int32_t>* w) {
    ptr.assign(1, 0);
    for (int i = 0; i < c.N; i++) {
      int n = 0;
      f >> n;
      for (int k = 0; k < n; k++) {
        int a = 0, b = 0;
        f >> a;
        if (w) f >> b;
        idx.push_back(a);
        if (w) w->push_back(b);
      }
      ptr.push_back((int32_t)idx.size());
    }
  };
  csr(c.loop_ptr, c.loop_idx, nullptr);
  csr(c.cov_ptr, c.cov_idx, &c.cov_w);
  csr(c.lc_ptr, c.lc_idx, &c.lc_w);
  c.pos.resize(3 * (size_t)c.P); c.corrected_by.resize(c.P); c.corrected_ref.resize(c.P); c.ref_kf.resize(c.P);
  c.bad.resize(c.P);
  for (int j = 0; j < c.P; j++)
    f >> c.pos[3 * j] >> c.pos[3 * j + 1] >> c.pos[3 * j + 2] >> c.corrected_by[j] >> c.corrected_ref[j] >>
        c.ref_kf[j] >> c.bad[j];
  return (bool)f;
}

struct Out {
  int iterations = 0;
  std::vector<int> trials;
  std::vector<double> chi2;
  double chi2_initial = 0.0, lambda = 0.0, branch_margin = 1e300;
  std::vector<double> sim3, pose, points, edge_chi2;   // [N][8], [N][16], [P][3], [E]
  std::vector<int32_t> edges;                          // [E][3]
  int counts[4] = {0, 0, 0, 0};
};

inline void print_vec(const char* tag, const double* v, size_t n) {
  std::printf("%s", tag);
  for (size_t k = 0; k < n; k++) std::printf(" %.17g", v[k]);
  std::printf("\n");
}

inline void print_edges(const Out& o) {
  std::printf("counts %d %d %d %d\n", o.counts[0], o.counts[1], o.counts[2], o.counts[3]);
  std::printf("edges");
  for (int32_t v : o.edges) std::printf(" %d", v);
  std::printf("\n");
}

inline void print_out(const Out& o) {
  print_edges(o);
  std::printf("iterations %d\n", o.iterations);
  std::printf("trials");
  for (int t : o.trials) std::printf(" %d", t);
  std::printf("\n");
  print_vec("chi2", o.chi2.data(), o.chi2.size());
  print_vec("chi2_initial", &o.chi2_initial, 1);
  print_vec("lambda", &o.lambda, 1);
  print_vec("branch_margin", &o.branch_margin, 1);
  print_vec("sim3", o.sim3.data(), o.sim3.size());
  print_vec("pose", o.pose.data(), o.pose.size());
  print_vec("points", o.points.data(), o.points.size());
  print_vec("edge_chi2", o.edge_chi2.data(), o.edge_chi2.size());
}

}  // namespace egio
