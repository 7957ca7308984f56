// mcs::OptimizeEssentialGraph of the host mirror with its solver argument, on a case file
// (tests/cpp/essgraph_io.hpp) and with the case's own options:
//   essgraph_sparse_demo CASE auto|dense|sparse
// prints "sparse 0|1" (which solver ran), "iterations", "edges", "pose i ..." and "points ...".
// Needs libmcs_amd.so; the run itself needs a GPU, compiling and linking do not.
#include <cstdio>
#include <cstring>

#include "../../multicol-slam-annotation_amd/host/mcs_multicol.hpp"
#include "essgraph_io.hpp"

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: essgraph_sparse_demo CASE auto|dense|sparse\n"); return 2; }
  egio::Case c;
  if (!egio::read_case(argv[1], c)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const mcs::EssentialGraphSolver solver = !std::strcmp(argv[2], "sparse") ? mcs::EssentialGraphSolver::Sparse
                                           : !std::strcmp(argv[2], "dense") ? mcs::EssentialGraphSolver::Dense
                                                                            : mcs::EssentialGraphSolver::Auto;
  std::vector<mcs::EssentialGraphKeyFrame> kfs(c.N);
  for (int i = 0; i < c.N; i++) {
    mcs::EssentialGraphKeyFrame& k = kfs[i];
    k.id = c.id[i];
    k.parent = c.parent[i];
    k.has_corrected = true;              // the case carries Sim3s: hand both tables over as they are
    for (int j = 0; j < 8; j++) { k.corrected[j] = c.Scw[8 * i + j]; k.non_corrected[j] = c.Snc[8 * i + j]; }
    k.loop_edges.assign(c.loop_idx.begin() + c.loop_ptr[i], c.loop_idx.begin() + c.loop_ptr[i + 1]);
    k.covisibles.assign(c.cov_idx.begin() + c.cov_ptr[i], c.cov_idx.begin() + c.cov_ptr[i + 1]);
    k.cov_weights.assign(c.cov_w.begin() + c.cov_ptr[i], c.cov_w.begin() + c.cov_ptr[i + 1]);
    k.loop_connections.assign(c.lc_idx.begin() + c.lc_ptr[i], c.lc_idx.begin() + c.lc_ptr[i + 1]);
    k.lc_weights.assign(c.lc_w.begin() + c.lc_ptr[i], c.lc_w.begin() + c.lc_ptr[i + 1]);
  }
  mcs::EssentialGraphPoints pts;
  pts.pos = c.pos;
  pts.corrected_by = c.corrected_by; pts.corrected_ref = c.corrected_ref; pts.ref_kf = c.ref_kf;
  pts.bad.assign(c.bad.begin(), c.bad.end());
  mcs_essgraph_options o;
  mcs_essgraph_default_options(&o);
  o.iterations = c.iterations; o.terminate_max_iter = c.term_max; o.max_trials = c.max_trials;
  o.gain_threshold = c.gain; o.lambda0 = c.lambda0;
  try {
    const mcs::EssentialGraphReport r = mcs::OptimizeEssentialGraph(kfs, pts, c.loop, c.cur, &o, 0, solver);
    std::printf("sparse %d\niterations %d\nedges %d\n", r.sparse ? 1 : 0, r.iterations, r.n_edges);
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 1;
  }
  for (int i = 0; i < c.N; i++) egio::print_vec("pose", kfs[i].pose, 16);
  egio::print_vec("points", pts.pos.data(), pts.pos.size());
  return 0;
}
