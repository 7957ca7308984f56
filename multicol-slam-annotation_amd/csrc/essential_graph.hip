// cOptimizer::OptimizeEssentialGraph on the device (C-ABI of include/mcs_essgraph.h).
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cOptimizer::OptimizeEssentialGraph                   src/cOptimizerLoopStuff.cpp:273-519
//   simpleVertexSim3Expmap, edgeSim3                     include/g2o_MultiCol_sim3_expmap.h:51-115
//   g2o::Sim3 (exp, log, *, inverse, map)                ThirdParty/g2o/g2o/types/sim3.h:41-292
//   numeric Jacobians of a binary edge                   ThirdParty/g2o/g2o/core/base_binary_edge.hpp:147-199
//   OptimizationAlgorithmLevenberg::solve                ThirdParty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
// The math is csrc/essential_graph_math.hpp (the functions the host program of the tests runs), the
// LM control csrc/lm_control.hpp, the linear solve csrc/ldlt.hpp on the 7 (N - 1) system without a
// Schur step (there are no landmarks).
//
// One call, all on the caller's stream:
//   k_init, k_check     the control block; range check of the device data into its status word
//   k_edge_keys + sort  the edges in (v0, v1, kind) order: every sum below runs in that order, so a
//                       permuted edge list gives the same bits (equal triples contribute equal terms)
//   k_setup + sort      measurements C_e once per edge; the (block, edge) items of the system sorted
//                       by block, stable, so a block's items stay in edge order
//   k_chi2, k_end       chi2 partials per workgroup in a fixed lane / stride order, added in index
//                       order by one workgroup, which also runs lm_step
//   per bounded step    k_linearise (14 columns per edge), k_zero, k_assemble (gather per block),
//                       k_damp (copy + lambda), ldlt pad / solve, k_update (push, exp(x) S), k_chi2,
//                       k_end (model decrease, lm_step, pop on reject)
//   k_poses, k_points, k_edge_chi2    the write-back (:479-518) and the outputs
// The LM control block lives in device memory: the host enqueues iterations x max_trials steps and
// the kernels of a step that is no longer needed return at once (BA's device-driven loop).
// FP64, -ffp-contract=off, no floating-point atomics: identical bits from run to run.
#include "host_util.hpp"
#include "ldlt.hpp"
#include "essential_graph_math.hpp"
#include "../../include/mcs_essgraph.h"
#include <climits>
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace mcs {
namespace esg {

constexpr int kChiBlocks = 64;           // chi2 partials (workgroups of k_chi2)
constexpr uint32_t kPadKey = 0xFFFFFFFFu;

struct Ctl {
  ba::LmCtl lm;
  int32_t trials[kMaxIterations];
  int32_t status;      // 0, MCS_ERR_ARG from k_check
  int32_t flag;        // the solve's ldlt:: status bits of the current trial
  double lambda0;
};

struct Dev {
  Ctl* ctl;
  int N, E, P, loop, n, T, D;
  const double* Scw; const double* Snc;
  const int32_t* edges_in;
  double* S; double* Sbak; double* C; double* err; double* J;
  int32_t* edges;            // [E][3] in sorted order
  const int32_t* perm;       // sorted edge -> the caller's edge
  uint32_t* ikey; uint32_t* ival;            // unsorted items [3E]
  const uint32_t* skey; const uint32_t* sval;   // sorted
  double* A0; double* b0; double* A; double* b; double* x;
  double* part;              // [kChiBlocks]
  double* point_pos; const int32_t* point_ref; const uint8_t* point_bad;
};

__device__ __forceinline__ bool step_off(const Dev& d) { return d.ctl->lm.done != 0; }

__global__ void k_init(Ctl h0, Ctl* c) {
  constexpr int nw = (int)(sizeof(Ctl) / 4);
  static_assert(sizeof(Ctl) % 4 == 0, "word copy");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&h0);
  uint32_t* dst = reinterpret_cast<uint32_t*>(c);
  for (int i = threadIdx.x; i < nw; i += blockDim.x) dst[i] = src[i];
}

// tile span of the 7 x 7 block of the free keyframes lo <= hi
__host__ __device__ inline int tile_span(int lo, int hi) { return (7 * hi + 6) / ldlt::TB - (7 * lo) / ldlt::TB + 1; }

// every index of the device data before anything reads through it
__global__ __launch_bounds__(256) void k_check(Dev d) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (k < d.E) {
    const int v0 = d.edges_in[3 * k], v1 = d.edges_in[3 * k + 1], kind = d.edges_in[3 * k + 2];
    bad = v0 < 0 || v0 >= d.N || v1 < 0 || v1 >= d.N || v0 == v1 || kind < 0 || kind > 1;
    if (!bad && d.D < d.T) {
      const int u0 = free_index(v0, d.loop), u1 = free_index(v1, d.loop);
      const int lo = u0 < 0 ? u1 : (u1 < 0 ? u0 : min(u0, u1)), hi = max(u0, u1);
      bad = tile_span(lo, hi) > d.D;
    }
  }
  if (k < d.P && !d.point_bad[k]) bad = bad || d.point_ref[k] < 0 || d.point_ref[k] >= d.N;
  if (bad) atomicMin(&d.ctl->status, (int32_t)MCS_ERR_ARG);
}

__global__ __launch_bounds__(256) void k_edge_keys(Dev d, uint64_t* key, int32_t* val) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d.E) return;
  const uint64_t v0 = (uint32_t)d.edges_in[3 * k], v1 = (uint32_t)d.edges_in[3 * k + 1];
  key[k] = (v0 << 33) | (v1 << 1) | (uint64_t)(d.edges_in[3 * k + 2] & 1);
  val[k] = k;
}

__device__ __forceinline__ uint32_t block_key(int a, int b) { return (uint32_t)((int64_t)a * (a + 1) / 2 + b); }

// per sorted edge: its triple, C_e = S_v1^meas (S_v0^meas)^-1 and its three items -- the diagonal
// blocks of both vertices and the block of the pair; per keyframe: the estimate
__global__ __launch_bounds__(256) void k_setup(Dev d) {
  if (d.ctl->status) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < d.N)
    for (int j = 0; j < 8; j++) d.S[8 * k + j] = d.Scw[8 * k + j];
  if (k >= d.E) return;
  const int o = d.perm[k];
  const int v0 = d.edges_in[3 * o], v1 = d.edges_in[3 * o + 1], kind = d.edges_in[3 * o + 2];
  d.edges[3 * k] = v0; d.edges[3 * k + 1] = v1; d.edges[3 * k + 2] = kind;
  const double* tab = kind ? d.Snc : d.Scw;
  sim3_store(edge_measurement(sim3_load(tab + 8 * v0), sim3_load(tab + 8 * v1)), d.C + 8 * (size_t)k);
  const int u0 = free_index(v0, d.loop), u1 = free_index(v1, d.loop);
  const uint32_t e4 = (uint32_t)k * 4u;
  d.ikey[3 * k] = u0 >= 0 ? block_key(u0, u0) : kPadKey;
  d.ival[3 * k] = e4;
  d.ikey[3 * k + 1] = u1 >= 0 ? block_key(u1, u1) : kPadKey;
  d.ival[3 * k + 1] = e4 + 1;
  d.ikey[3 * k + 2] = (u0 >= 0 && u1 >= 0) ? (u0 > u1 ? block_key(u0, u1) : block_key(u1, u0)) : kPadKey;
  d.ival[3 * k + 2] = e4 + (u0 > u1 ? 2u : 3u);
}

// chi2 of every edge at S; the workgroup's partial in a fixed order (thread t adds edges t,
// t + stride, ...; the 256 sums by a fixed tree).  edge_out (nullable): per edge, caller's order.
__global__ __launch_bounds__(256) void k_chi2(Dev d, int final_pass, double* edge_out) {
  if (d.ctl->status) return;
  if (final_pass ? (d.ctl->lm.dev_err != 0) : step_off(d)) return;
  __shared__ double sm[256];
  double acc = 0.0;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < d.E; e += gridDim.x * 256) {
    double err[7];
    edge_error(sim3_load(d.C + 8 * (size_t)e), sim3_load(d.S + 8 * d.edges[3 * e]),
               sim3_load(d.S + 8 * d.edges[3 * e + 1]), err);
    const double c = edge_chi2(err);
    if (edge_out) edge_out[d.perm[e]] = c;
    acc += c;
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) d.part[blockIdx.x] = sm[0];
}

// One workgroup after k_chi2: the partials in index order; start = the optimize() call's first
// chi2 (lm_start_body, lambda of iteration 0 = setUserLambdaInit), else the end of a trial: the
// model decrease sum x (lambda x + b), lm_step, and the pop of a rejected trial.
__global__ __launch_bounds__(256) void k_end(Dev d, int nparts, int start, int iterations) {
  Ctl* ctl = d.ctl;
  ba::LmCtl* c = &ctl->lm;
  __shared__ double sm[256];
  __shared__ int restore;
  if (start) {
    if (threadIdx.x != 0) return;
    if (ctl->status) { c->done = 1; return; }
    double chi = 0.0;
    for (int i = 0; i < nparts; i++) chi += d.part[i];
    ba::lm_start_body(c, chi);
    c->lambda = ctl->lambda0;
    c->done = (iterations <= 0 || d.n <= 0 || d.E <= 0) ? 1 : 0;   // "0 vertices to optimize"
    return;
  }
  if (c->done) return;
  const double lambda = c->lambda;
  double acc = 0.0;
  for (int i = threadIdx.x; i < d.n; i += 256) acc += d.x[i] * (lambda * d.x[i] + d.b0[i]);
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double chi = 0.0;
    for (int i = 0; i < nparts; i++) chi += d.part[i];
    const double sc[3] = {chi, 0.0, sm[0]};
    const int it = c->iter, flag = ctl->flag;
    ba::lm_step(c, sc, (flag & ldlt::kFlagZeroPivot) != 0, (flag & ldlt::kFlagTimeout) != 0, 0);
    if (it < kMaxIterations) ctl->trials[it]++;
    ctl->flag = 0;
    restore = c->restore;
  }
  __syncthreads();
  if (restore)
    for (int i = threadIdx.x; i < 8 * d.N; i += 256) d.S[i] = d.Sbak[i];
}

// one lane per (edge, vertex, column): the central difference through exp(delta e_k) S; the lane
// of column 0 of vertex 0 also leaves the edge's error.  Columns of the fixed vertex stay unread.
__global__ __launch_bounds__(256) void k_linearise(Dev d) {
  if (step_off(d) || !d.ctl->lm.lin) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int e = g / 14, r = g % 14, w = r / 7, k = r % 7;
  if (e >= d.E) return;
  const int v0 = d.edges[3 * e], v1 = d.edges[3 * e + 1];
  const Sim3 C = sim3_load(d.C + 8 * (size_t)e), S0 = sim3_load(d.S + 8 * v0), S1 = sim3_load(d.S + 8 * v1);
  if (r == 0) edge_error(C, S0, S1, d.err + 7 * (size_t)e);
  if ((w ? v1 : v0) == d.loop) return;
  double col[7];
  edge_jac_col(C, S0, S1, w, k, kDiffStep, col);
  double* J = d.J + 98 * (size_t)e + 49 * w + k;
  for (int q = 0; q < 7; q++) J[7 * q] = col[q];
}

__global__ __launch_bounds__(256) void k_zero(Dev d, size_t na) {
  if (step_off(d) || !d.ctl->lm.lin) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (size_t)gridDim.x * 256) d.A0[i] = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)ldlt::TB * d.T; i += (size_t)gridDim.x * 256)
    d.b0[i] = 0.0;
}

// One wave per sorted item; the wave of a block's first item adds the block over its items in
// order (lane = entry of the 7 x 7), a diagonal block's wave also b = -J^T e of its vertex.
__global__ __launch_bounds__(256) void k_assemble(Dev d) {
  if (step_off(d) || !d.ctl->lm.lin) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, M = 3 * d.E;
  if (i >= M) return;
  const uint32_t key = d.skey[i];
  if (key == kPadKey || (i > 0 && d.skey[i - 1] == key)) return;
  const int i7 = lane / 7, j7 = lane % 7;
  double sum = 0.0, bsum = 0.0;
  int a = 0, b = 0;
  bool diag = false;
  for (int j = i; j < M && d.skey[j] == key; j++) {
    const uint32_t val = d.sval[j];
    const int e = (int)(val >> 2), t = (int)(val & 3u);
    const int rs = (t == 0 || t == 2) ? 0 : 1, cs = (t == 0 || t == 3) ? 0 : 1;
    if (j == i) {
      const int u0 = free_index(d.edges[3 * e], d.loop), u1 = free_index(d.edges[3 * e + 1], d.loop);
      a = rs ? u1 : u0;
      b = cs ? u1 : u0;
      diag = t < 2;
    }
    const double* Ja = d.J + 98 * (size_t)e + 49 * rs;
    const double* Jb = d.J + 98 * (size_t)e + 49 * cs;
    if (lane < 49) {
      double s = 0.0;
      for (int r = 0; r < 7; r++) s += Ja[7 * r + i7] * Jb[7 * r + j7];
      sum += s;
    }
    if (diag && lane < 7) {
      double s = 0.0;
      for (int r = 0; r < 7; r++) s += Ja[7 * r + lane] * d.err[7 * (size_t)e + r];
      bsum += -s;
    }
  }
  const int row = 7 * a + i7, col = 7 * b + j7;
  if (lane < 49 && row >= col) d.A0[ldlt::sidx(row, col, d.T)] = sum;
  if (diag && lane < 7) d.b0[7 * a + lane] = bsum;
}

// the trial's copy: A = A0 + lambda I on the leading n rows, b = b0
__global__ __launch_bounds__(256) void k_damp(Dev d, size_t na) {
  if (step_off(d)) return;
  const double lambda = d.ctl->lm.lambda;
  const size_t tt = (size_t)ldlt::TB * ldlt::TB;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (size_t)gridDim.x * 256) {
    double v = d.A0[i];
    const size_t tile = i / tt;
    if (tile < (size_t)d.T) {
      const int r = (int)(i % tt) / ldlt::TB, c = (int)(i % ldlt::TB);
      if (r == c && (int)tile * ldlt::TB + r < d.n) v += lambda;
    }
    d.A[i] = v;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)ldlt::TB * d.T; i += (size_t)gridDim.x * 256)
    d.b[i] = d.b0[i];
}

// push the estimates and apply oplusImpl: exp(x_i) S_i
__global__ __launch_bounds__(256) void k_update(Dev d) {
  if (step_off(d)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.N) return;
  const Sim3 S = sim3_load(d.S + 8 * i);
  sim3_store(S, d.Sbak + 8 * i);
  const int u = free_index(i, d.loop);
  if (u >= 0) sim3_store(s3o::sim3_mul(s3o::sim3_exp(d.x + 7 * u), S), d.S + 8 * i);
}

// :479-491 and the run's figures; status decides whether anything is written at all
__global__ __launch_bounds__(256) void k_poses(Dev d, mcs_essgraph_out o) {
  const Ctl* ctl = d.ctl;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int status = ctl->status ? ctl->status : (ctl->lm.dev_err ? (int)MCS_ERR_HIP : 0);
  if (i == 0) *o.status = status;
  if (status) return;
  if (i == 0) {
    const int it = ctl->lm.iter;
    if (o.iterations) *o.iterations = it;
    if (o.lambda) *o.lambda = it > 0 ? ctl->lm.lambda_final : 0.0;
    for (int k = 0; k < kMaxIterations; k++) {
      if (o.trials) o.trials[k] = ctl->trials[k];
      if (o.chi2) o.chi2[k] = k < it ? ctl->lm.trace[k] : 0.0;
    }
  }
  if (i >= d.N) return;
  const Sim3 S = sim3_load(d.S + 8 * i);
  double M[16], R[9];
  pose_from_sim3(S, M, R);
  if (o.sim3) sim3_store(S, o.sim3 + 8 * (size_t)i);
  if (o.rot) for (int k = 0; k < 9; k++) o.rot[9 * (size_t)i + k] = R[k];
  if (o.pose) for (int k = 0; k < 16; k++) o.pose[16 * (size_t)i + k] = M[k];
}

// :496-518
__global__ __launch_bounds__(256) void k_points(Dev d) {
  if (d.ctl->status || d.ctl->lm.dev_err) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d.P || d.point_bad[j]) return;
  const int ref = d.point_ref[j];
  double x[3] = {d.point_pos[3 * (size_t)j], d.point_pos[3 * (size_t)j + 1], d.point_pos[3 * (size_t)j + 2]}, y[3];
  correct_point(sim3_load(d.Scw + 8 * ref), sim3_load(d.S + 8 * ref), x, y);
  for (int k = 0; k < 3; k++) d.point_pos[3 * (size_t)j + k] = y[k];
}

// :501-507 with the id -> index search over the ascending ids
__global__ __launch_bounds__(256) void k_resolve_refs(int N, const int64_t* kf_id, int P, const int64_t* by,
                                                      const int64_t* cref, const int64_t* ref_kf, int64_t current_id,
                                                      int32_t* out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  const int64_t id = point_ref_id(by[j], cref[j], ref_kf[j], current_id);
  int lo = 0, hi = N;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (kf_id[m] < id) lo = m + 1; else hi = m;
  }
  out[j] = (lo < N && kf_id[lo] == id) ? lo : -1;
}

static int tiles_of_kf(int n_kf) { return ldlt::tiles_for(std::max(1, 7 * (n_kf - 1))); }

static int supported(int n_kf, int band) {
  const int T = tiles_of_kf(n_kf);
  if (T == 1) return MCS_OK;
  if (T > ldlt::kPipeMaxT || !ldlt::pipe_supported(T, band)) {
    set_error("essential graph: the system exceeds the solver (a workspace holds a dense system of at most 96 tiles, "
              "878 keyframes)");
    return MCS_ERR_UNSUPPORTED;
  }
  return MCS_OK;
}

// everything the host can see, before any device use
static int check_call(int32_t N, const double* Scw, const double* Snc, int32_t loop, int32_t E, const int32_t* edges,
                      int32_t P, const double* pos, const int32_t* ref, const uint8_t* bad,
                      const mcs_essgraph_options* o, const mcs_essgraph_out* out) {
  using host::bad_arg;
  if (!o || !out || !out->status) return bad_arg("essential graph: null options, out or out->status");
  if (N < 1 || E < 0 || P < 0 || (int64_t)E * 14 >= INT_MAX / 8) return bad_arg("essential graph: bad counts");
  if (!Scw || !Snc || (E > 0 && !edges) || (P > 0 && (!pos || !ref || !bad)))
    return bad_arg("essential graph: null buffer");
  if (loop < 0 || loop >= N) return bad_arg("essential graph: loop_index outside the keyframes");
  if (o->iterations < 0 || o->iterations > MCS_ESSGRAPH_MAX_ITERATIONS)
    return bad_arg("essential graph: iterations outside [0, 64]");
  if (o->max_trials < 1 || o->max_trials > MCS_ESSGRAPH_MAX_TRIALS)
    return bad_arg("essential graph: max_trials outside [1, 64]");
  if (o->tile_band < 0) return bad_arg("essential graph: negative tile_band");
  return supported(N, o->tile_band);
}

}  // namespace esg
}  // namespace mcs

using namespace mcs;

struct mcs_essgraph_workspace {
  int device = 0, max_kf = 0, max_edges = 0, max_points = 0, Tmax = 1;
  esg::Ctl* ctl = nullptr;
  double *S = nullptr, *Sbak = nullptr, *C = nullptr, *err = nullptr, *J = nullptr;
  double *A0 = nullptr, *b0 = nullptr, *A = nullptr, *b = nullptr, *x = nullptr, *part = nullptr;
  uint64_t *ekey_in = nullptr, *ekey_out = nullptr;
  int32_t *eval_in = nullptr, *perm = nullptr, *edges = nullptr;
  uint32_t *ikey = nullptr, *ival = nullptr, *skey = nullptr, *sval = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0, tasks_cap = 0;
  ldlt::Work lw;
  int up_T = 0, up_D = 0;      // the task table on the device
  std::vector<void*> owned;
};

extern "C" {

void mcs_essgraph_default_options(mcs_essgraph_options* o) {
  if (!o) return;
  o->iterations = 20; o->terminate_max_iter = 15; o->gain_threshold = 1e-6; o->lambda0 = 1e-6; o->max_trials = 10;
  o->tile_band = 0;
}

int32_t mcs_essgraph_tile_band(int32_t n_kf, int32_t loop_index, const int32_t* edges, int32_t n_edges) {
  if (n_kf < 1 || n_edges < 0 || (n_edges > 0 && !edges)) return 0;
  int D = (n_kf > 1 && esg::tiles_of_kf(n_kf) > 1) ? 2 : 1;    // a 7 x 7 block can straddle two tiles
  for (int e = 0; e < n_edges; e++) {
    const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
    if (v0 < 0 || v0 >= n_kf || v1 < 0 || v1 >= n_kf) continue;
    const int u0 = esg::free_index(v0, loop_index), u1 = esg::free_index(v1, loop_index);
    if (u0 < 0 || u1 < 0) continue;
    D = std::max(D, esg::tile_span(std::min(u0, u1), std::max(u0, u1)));
  }
  return D;
}

int mcs_essgraph_supported(int32_t n_kf, int32_t tile_band) {
  if (n_kf < 1 || tile_band < 0) return host::bad_arg("essential graph: bad counts");
  return esg::supported(n_kf, tile_band);
}

void mcs_essgraph_workspace_destroy(mcs_essgraph_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  for (void* p : w->owned) (void)hipFree(p);
  delete w;
}

int mcs_essgraph_workspace_create(int32_t device, int32_t max_kf, int32_t max_edges, int32_t max_points,
                                  mcs_essgraph_workspace** out) {
  if (!out || max_kf < 1 || max_edges < 0 || max_points < 0 || (int64_t)max_edges * 14 >= INT_MAX / 8)
    return host::bad_arg("essential graph workspace: bad argument");
  if (int rc = esg::supported(max_kf, 0)) return rc;
  if (int rc = host::open_device(device, "essential graph workspace")) return rc;
  mcs_essgraph_workspace* w = new mcs_essgraph_workspace;
  w->device = device; w->max_kf = max_kf; w->max_edges = max_edges; w->max_points = max_points;
  const int T = w->Tmax = esg::tiles_of_kf(max_kf);
  const size_t Em = std::max(1, max_edges), Nm = (size_t)max_kf;
  hipError_t e = hipSuccess;
  auto get = [&](auto** p, size_t bytes) {
    void* q = nullptr;
    if (e == hipSuccess) e = hipMalloc(&q, std::max<size_t>(16, bytes));
    if (q) w->owned.push_back(q);
    *p = static_cast<std::remove_pointer_t<decltype(p)>>(q);
  };
  const size_t nt = ldlt::tile_doubles(T), nb = (size_t)ldlt::TB * T;
  get(&w->ctl, sizeof(esg::Ctl));
  get(&w->S, 64 * Nm); get(&w->Sbak, 64 * Nm); get(&w->C, 64 * Em); get(&w->err, 56 * Em); get(&w->J, 784 * Em);
  get(&w->A0, 8 * nt); get(&w->A, 8 * nt); get(&w->b0, 8 * nb); get(&w->b, 8 * nb); get(&w->x, 8 * nb);
  get(&w->part, 8 * esg::kChiBlocks);
  get(&w->ekey_in, 8 * Em); get(&w->ekey_out, 8 * Em); get(&w->eval_in, 4 * Em); get(&w->perm, 4 * Em);
  get(&w->edges, 12 * Em);
  get(&w->ikey, 12 * Em); get(&w->ival, 12 * Em); get(&w->skey, 12 * Em); get(&w->sval, 12 * Em);
  size_t b1 = 0, b2 = 0;
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, b1, w->ekey_in, w->ekey_out, w->eval_in, w->perm, Em, 0u, 64u, (hipStream_t)0);
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, b2, w->ikey, w->skey, w->ival, w->sval, 3 * Em, 0u, 32u, (hipStream_t)0);
  w->tmp_bytes = std::max<size_t>(16, std::max(b1, b2));
  get(&w->tmp, w->tmp_bytes);
  if (T >= 2) {
    get(&w->lw.L, 8 * nt); get(&w->lw.Linv, 8 * (size_t)T * ldlt::TB * ldlt::TB); get(&w->lw.z, 8 * nb);
    get(&w->lw.W, 8 * nt); get(&w->lw.du, 8 * (size_t)T * 128);
    get(&w->lw.sync, 4 * ldlt::pipe_sync_words(T, T));
    w->tasks_cap = ldlt::pipe_tasks_host(T, T).size();
    get(&w->lw.tasks, sizeof(int4) * w->tasks_cap);
  }
  if (e != hipSuccess) {
    mcs_essgraph_workspace_destroy(w);
    set_hip_error(e, "essential graph workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

int mcs_essgraph_resolve_point_refs_device(int32_t N, const int64_t* d_kf_id, int32_t P, const int64_t* d_corrected_by,
                                           const int64_t* d_corrected_ref, const int64_t* d_ref_kf, int64_t current_id,
                                           int32_t* d_point_ref, void* stream) {
  if (N < 1 || P < 0) return host::bad_arg("essential graph point refs: bad counts");
  if (P == 0) return MCS_OK;
  if (!d_kf_id || !d_corrected_by || !d_corrected_ref || !d_ref_kf || !d_point_ref)
    return host::bad_arg("essential graph point refs: null buffer");
  hipLaunchKernelGGL(esg::k_resolve_refs, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, d_kf_id, P,
                     d_corrected_by, d_corrected_ref, d_ref_kf, current_id, d_point_ref);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_optimize_essential_graph_device(mcs_essgraph_workspace* ws, int32_t N, const double* d_Scw,
                                        const double* d_Snc, int32_t loop_index, int32_t E, const int32_t* d_edges,
                                        int32_t P, double* d_point_pos, const int32_t* d_point_ref,
                                        const uint8_t* d_point_bad, const mcs_essgraph_options* opts,
                                        const mcs_essgraph_out* out, void* stream) {
  if (int rc = esg::check_call(N, d_Scw, d_Snc, loop_index, E, d_edges, P, d_point_pos, d_point_ref, d_point_bad, opts,
                               out))
    return rc;
  if (ws && (N > ws->max_kf || E > ws->max_edges || P > ws->max_points))
    return host::bad_arg("essential graph: more keyframes, edges or points than the workspace holds");
  hipStream_t st = (hipStream_t)stream;
  mcs_essgraph_workspace* tmp = nullptr;
  if (!ws) {
    int dev = 0;
    MCS_HIP_CHECK(hipGetDevice(&dev));
    if (int rc = mcs_essgraph_workspace_create(dev, N, E, P, &tmp)) return rc;
    ws = tmp;
  } else {
    MCS_HIP_CHECK(hipSetDevice(ws->device));
  }
  auto finish = [&](int rc, hipError_t e) {
    if (tmp) {
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      mcs_essgraph_workspace_destroy(tmp);
    }
    if (rc) return rc;
    if (e != hipSuccess) { set_hip_error(e, "essential graph", __FILE__, __LINE__); return (int)MCS_ERR_HIP; }
    return (int)MCS_OK;
  };

  esg::Dev d{};
  d.ctl = ws->ctl;
  d.N = N; d.E = E; d.P = P; d.loop = loop_index; d.n = 7 * (N - 1);
  d.T = esg::tiles_of_kf(N);
  d.D = d.T >= 2 ? ldlt::pipe_band(d.T, opts->tile_band) : 1;
  d.Scw = d_Scw; d.Snc = d_Snc; d.edges_in = d_edges;
  d.S = ws->S; d.Sbak = ws->Sbak; d.C = ws->C; d.err = ws->err; d.J = ws->J;
  d.edges = ws->edges; d.perm = ws->perm; d.ikey = ws->ikey; d.ival = ws->ival; d.skey = ws->skey; d.sval = ws->sval;
  d.A0 = ws->A0; d.b0 = ws->b0; d.A = ws->A; d.b = ws->b; d.x = ws->x; d.part = ws->part;
  d.point_pos = d_point_pos; d.point_ref = d_point_ref; d.point_bad = d_point_bad;

  ldlt::Work lw = ws->lw;
  if (d.T >= 2) {
    const std::vector<int4>& tq = ldlt::pipe_tasks_host(d.T, d.D);
    if (tq.size() > ws->tasks_cap) return finish(host::bad_arg("essential graph: task table above the workspace's"), hipSuccess);
    if (ws->up_T != d.T || ws->up_D != d.D) {
      if (!tq.empty()) {
        hipError_t e = hipMemcpyAsync(ws->lw.tasks, tq.data(), tq.size() * sizeof(int4), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return finish(0, e);
      }
      ws->up_T = d.T; ws->up_D = d.D;
    }
    lw.ntasks = (int)tq.size();
    lw.pipe_T = d.T;
    lw.band = d.D;
  }

  esg::Ctl h0{};
  mcs_ba_options bo{};
  bo.max_iterations = opts->iterations; bo.gain_threshold = opts->gain_threshold;
  bo.terminate_max_iter = opts->terminate_max_iter; bo.max_trials = opts->max_trials; bo.tau = 0.0;
  ba::lm_init(h0.lm, bo);
  h0.lm.done = 1;              // until k_end's start pass has the first chi2
  h0.lambda0 = opts->lambda0;
  auto gb = [](int n) { return dim3((unsigned)((std::max(n, 1) + 255) / 256)); };
  const int nchi = std::max(1, std::min(esg::kChiBlocks, (E + 255) / 256));
  const size_t na = ldlt::band_tiles(d.T >= 2 ? d.D : 1, d.T) * ldlt::TB * ldlt::TB;
  const unsigned gz = (unsigned)std::min<size_t>(2048, (na + 255) / 256);
  int* d_flag = &ws->ctl->flag;
  const int* skip = &ws->ctl->lm.done;

  hipLaunchKernelGGL(esg::k_init, dim3(1), dim3(256), 0, st, h0, ws->ctl);
  hipLaunchKernelGGL(esg::k_check, gb(std::max(E, P)), dim3(256), 0, st, d);
  if (E > 0) {
    hipLaunchKernelGGL(esg::k_edge_keys, gb(E), dim3(256), 0, st, d, ws->ekey_in, ws->eval_in);
    size_t b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b, ws->ekey_in, ws->ekey_out, ws->eval_in, ws->perm, (size_t)E, 0u,
                                             64u, st);
    if (e == hipSuccess && b > ws->tmp_bytes) { set_error("essential graph: sort storage above the workspace's"); return finish(MCS_ERR_CAPACITY, hipSuccess); }
    b = ws->tmp_bytes;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(ws->tmp, b, ws->ekey_in, ws->ekey_out, ws->eval_in, ws->perm, (size_t)E, 0u,
                                             64u, st);
    if (e != hipSuccess) return finish(0, e);
  }
  hipLaunchKernelGGL(esg::k_setup, gb(std::max(N, E)), dim3(256), 0, st, d);
  if (E > 0) {
    size_t b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b, ws->ikey, ws->skey, ws->ival, ws->sval, 3 * (size_t)E, 0u, 32u, st);
    if (e == hipSuccess && b > ws->tmp_bytes) { set_error("essential graph: sort storage above the workspace's"); return finish(MCS_ERR_CAPACITY, hipSuccess); }
    b = ws->tmp_bytes;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(ws->tmp, b, ws->ikey, ws->skey, ws->ival, ws->sval, 3 * (size_t)E, 0u, 32u, st);
    if (e != hipSuccess) return finish(0, e);
  }
  hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 1, (double*)nullptr);
  hipLaunchKernelGGL(esg::k_end, dim3(1), dim3(256), 0, st, d, nchi, 1, (int)opts->iterations);
  const int steps = (d.n > 0 && E > 0) ? opts->iterations * opts->max_trials : 0;
  for (int g = 0; g < steps; g++) {
    hipLaunchKernelGGL(esg::k_linearise, gb(14 * E), dim3(256), 0, st, d);
    hipLaunchKernelGGL(esg::k_zero, dim3(gz), dim3(256), 0, st, d, na);
    hipLaunchKernelGGL(esg::k_assemble, dim3((unsigned)((3 * E + 3) / 4)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(esg::k_damp, dim3(gz), dim3(256), 0, st, d, na);
    hipError_t e;
    if (d.T == 1) {
      e = ldlt::solve_one_tile(d.A, d.b, d.x, d.n, 1.0, d_flag, st, skip);
    } else {
      e = ldlt::pad(d.A, d.b, d.n, d.T, 1.0, st, skip);
      if (e == hipSuccess) e = ldlt::solve(d.A, d.b, d.x, d.T, lw, d_flag, st, skip);
    }
    if (e != hipSuccess) return finish(0, e);
    hipLaunchKernelGGL(esg::k_update, gb(N), dim3(256), 0, st, d);
    hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 0, (double*)nullptr);
    hipLaunchKernelGGL(esg::k_end, dim3(1), dim3(256), 0, st, d, nchi, 0, (int)opts->iterations);
  }
  hipLaunchKernelGGL(esg::k_poses, gb(N), dim3(256), 0, st, d, *out);
  if (P > 0) hipLaunchKernelGGL(esg::k_points, gb(P), dim3(256), 0, st, d);
  if (out->edge_chi2 && E > 0) hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 1, out->edge_chi2);
  return finish(0, hipGetLastError());
}

int mcs_optimize_essential_graph(int32_t device, int32_t N, const double* Scw, const double* Snc, int32_t loop_index,
                                 int32_t E, const int32_t* edges, int32_t P, double* point_pos,
                                 const int32_t* point_ref, const uint8_t* point_bad,
                                 const mcs_essgraph_options* opts, const mcs_essgraph_out* out) {
  if (int rc = esg::check_call(N, Scw, Snc, loop_index, E, edges, P, point_pos, point_ref, point_bad, opts, out))
    return rc;
  for (int e = 0; e < E; e++)
    if (edges[3 * e] == edges[3 * e + 1]) return host::bad_arg("essential graph: an edge joins a keyframe to itself");
  if (int rc = host::open_device(device, "essential graph")) return rc;
  host::DevBufs B;
  const size_t n = (size_t)N, ne = (size_t)E, np = (size_t)P, K = MCS_ESSGRAPH_MAX_ITERATIONS;
  const double* dScw = B.up(Scw, 8 * n);
  const double* dSnc = B.up(Snc, 8 * n);
  const int32_t* dE = B.up(edges, 3 * ne);
  double* dpos = B.up(point_pos, 3 * np);
  const int32_t* dref = B.up(point_ref, np);
  const uint8_t* dbad = B.up(point_bad, np);
  mcs_essgraph_out d{};
  d.sim3 = B.alloc<double>(8 * n); d.rot = B.alloc<double>(9 * n); d.pose = B.alloc<double>(16 * n);
  d.iterations = B.alloc<int32_t>(1); d.trials = B.alloc<int32_t>(K); d.chi2 = B.alloc<double>(K);
  d.lambda = B.alloc<double>(1);
  d.edge_chi2 = out->edge_chi2 ? B.alloc<double>(ne) : nullptr;
  d.status = B.alloc<int32_t>(1);
  if (B.err != hipSuccess) { set_hip_error(B.err, "essential graph upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (int rc = mcs_optimize_essential_graph_device(nullptr, N, dScw, dSnc, loop_index, E, dE, P, dpos, dref, dbad, opts,
                                                   &d, nullptr))
    return rc;
  MCS_HIP_CHECK(hipDeviceSynchronize());
  int32_t status = 0;
  B.down(&status, d.status, 1);
  *out->status = status;
  if (B.err == hipSuccess && status == 0) {
    B.down(point_pos, dpos, 3 * np);
    B.down(out->sim3, d.sim3, 8 * n); B.down(out->rot, d.rot, 9 * n); B.down(out->pose, d.pose, 16 * n);
    B.down(out->iterations, d.iterations, 1); B.down(out->trials, d.trials, K); B.down(out->chi2, d.chi2, K);
    B.down(out->lambda, d.lambda, 1); B.down(out->edge_chi2, d.edge_chi2, ne);
  }
  if (B.err != hipSuccess) { set_hip_error(B.err, "essential graph download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (status == MCS_ERR_ARG) return host::bad_arg("essential graph: an index of the edge or point data is out of range");
  if (status) { set_error("essential graph: the solver's hand-off wait gave up"); return status; }
  return MCS_OK;
}

}  // extern "C"

// the block-sparse path over a plan (the mcs_essgraph_plan entries)
#include "essential_graph_sparse.hpp"
