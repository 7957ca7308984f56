// The edge list of cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:355-470) from
// flat arrays (C-ABI of include/mcs_essgraph.h).  Pure integer bookkeeping, no device work.
// Keyframes come in ascending id order, which is the order the loops run in here; insertedEdges
// (:351, :380) is filled but never consulted in the text, so nothing is deduplicated.
#include <cstdint>

#include "../../include/mcs_essgraph.h"

// common.hpp's, declared here so that a host compiler without the HIP headers takes this file
// (tests/cpp/essgraph_host.cpp)
namespace mcs { void set_error(const char* msg); }

extern "C" int mcs_essgraph_select_edges(const mcs_essgraph_map* m, int32_t* edges, int32_t cap, int32_t* n_edges,
                                         int32_t* counts) {
  using mcs::set_error;
  if (!m || !n_edges || !counts || m->n_kf < 0 || cap < 0 || (cap > 0 && !edges) ||
      (m->n_kf > 0 && (!m->kf_id || !m->parent || !m->has_corrected || !m->loop_ptr || !m->cov_ptr || !m->lc_ptr))) {
    set_error("mcs_essgraph_select_edges: null or invalid argument");
    return MCS_ERR_ARG;
  }
  const int N = m->n_kf;
  *n_edges = 0;
  for (int k = 0; k < 4; k++) counts[k] = 0;
  if (N == 0) return MCS_OK;
  if (m->current_index < 0 || m->current_index >= N || m->loop_index < 0 || m->loop_index >= N) {
    set_error("mcs_essgraph_select_edges: current_index / loop_index outside the keyframes");
    return MCS_ERR_ARG;
  }
  auto row_ok = [&](const int32_t* ptr, const int32_t* idx, const int32_t* w, bool need_w) {
    if (ptr[0] != 0) return false;
    for (int i = 0; i < N; i++)
      if (ptr[i + 1] < ptr[i]) return false;
    if (ptr[N] > 0 && (!idx || (need_w && !w))) return false;
    for (int k = 0; k < ptr[N]; k++)
      if (idx[k] < 0 || idx[k] >= N) return false;
    return true;
  };
  for (int i = 0; i < N; i++)
    if (m->parent[i] < -1 || m->parent[i] >= N || (i > 0 && m->kf_id[i] <= m->kf_id[i - 1])) {
      set_error("mcs_essgraph_select_edges: parent index out of range or keyframe ids not ascending");
      return MCS_ERR_ARG;
    }
  if (!row_ok(m->loop_ptr, m->loop_idx, nullptr, false) || !row_ok(m->cov_ptr, m->cov_idx, m->cov_weight, true) ||
      !row_ok(m->lc_ptr, m->lc_idx, m->lc_weight, true)) {
    set_error("mcs_essgraph_select_edges: a neighbour list is malformed or names a keyframe out of range");
    return MCS_ERR_ARG;
  }
  int64_t n = 0;
  auto add = [&](int v0, int v1, int kind, int source) {
    if (n < cap) { edges[3 * n] = v0; edges[3 * n + 1] = v1; edges[3 * n + 2] = kind; }
    n++;
    counts[source]++;
  };
  // the non-corrected table differs from vScw only at a keyframe with a corrected Sim3
  auto kind_of = [&](int a, int b) { return (m->has_corrected[a] || m->has_corrected[b]) ? 1 : 0; };
  // loop-connection edges (:355-382): kept at weight >= min_weight, and (current, loop) always
  for (int i = 0; i < N; i++)
    for (int k = m->lc_ptr[i]; k < m->lc_ptr[i + 1]; k++) {
      const int j = m->lc_idx[k];
      if ((i != m->current_index || j != m->loop_index) && m->lc_weight[k] < m->min_weight) continue;
      add(i, j, 0, 0);
    }
  for (int i = 0; i < N; i++) {
    if (m->parent[i] >= 0) add(i, m->parent[i], kind_of(i, m->parent[i]), 1);        // :401-417
    for (int k = m->loop_ptr[i]; k < m->loop_ptr[i + 1]; k++) {                      // :421-443
      const int l = m->loop_idx[k];
      if (m->kf_id[l] < m->kf_id[i]) add(i, l, kind_of(i, l), 2);
    }
    for (int k = m->cov_ptr[i]; k < m->cov_ptr[i + 1]; k++) {                        // :447-469
      if (m->cov_weight[k] < m->min_weight) continue;
      const int c = m->cov_idx[k];
      if (m->kf_id[c] < m->kf_id[i]) add(i, c, kind_of(i, c), 3);
    }
  }
  if (n > INT32_MAX) { set_error("mcs_essgraph_select_edges: more than 2^31 edges"); return MCS_ERR_UNSUPPORTED; }
  *n_edges = (int32_t)n;
  if (n > cap) { set_error("mcs_essgraph_select_edges: edge buffer too small"); return MCS_ERR_CAPACITY; }
  return MCS_OK;
}
