// OptimizeEssentialGraph over a plan: the block-sparse LDL^T path (the mcs_essgraph_plan entries of
// include/mcs_essgraph.h).  Included at the end of essential_graph.hip, whose kernels it reuses
// unchanged up to the solve: k_init, k_check, the two sorts, k_setup, k_linearise, k_chi2, k_end,
// k_update, k_poses, k_points.  The plan is essential_graph_plan.hpp / .cpp, the arithmetic of a
// supernode essential_graph_sparse_math.hpp (shared with tests/cpp/essgraph_sparse_host.cpp).
//
// New kernels:
//   k_sp_check     after k_check: N or loop_index other than the plan's, or an edge whose pair of
//                  free keyframes is no block of A in the plan -> MCS_ERR_ARG in the status word
//   k_sp_zero      A0 (all panels, fill included) and b0
//   k_sp_assemble  k_assemble's gather per block, stored at the block's place in its panel; a
//                  block whose permuted row is above its column is stored transposed
//   k_sp_factor    one workgroup per supernode of a level: copy from A0 with lambda on the
//                  diagonal (the damp step), left-looking update from the sources, dense LDL^T of
//                  the panel, the forward and diagonal solves riding along (sn_factor)
//   k_sp_backward  the levels downwards: x in keyframe order (sn_backward)
// A launch is one level; the chain of levels at the top that hold one supernode each is one launch
// of one workgroup.  No workgroup waits on another: every dependency is a launch boundary or a
// barrier inside a workgroup, so there is no hand-off wait and no timeout flag on this path.
// VALU FP64 throughout: a 7 x 7 block does not fill the 16 x 16 x 4 FP64 MFMA shape, and the
// panels' updates are rank-1 steps and dot products over rows of differing length.
#pragma once
#include "essential_graph_sparse_math.hpp"

namespace mcs {
namespace esg {

constexpr int kSpBlock = 7;              // the block size; the numeric code is a template over it
constexpr int kSpThreads = 1024;

struct DevExec {
  int tid, nt;
  int* flag;
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ void raise(int bits) { atomicOr(flag, bits); }
};

__global__ __launch_bounds__(256) void k_sp_check(Dev d, SpView v, int plan_n_kf, int plan_loop) {
  if (d.N != plan_n_kf || d.loop != plan_loop) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(&d.ctl->status, (int32_t)MCS_ERR_ARG);
    return;
  }
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d.E) return;
  const int v0 = d.edges_in[3 * k], v1 = d.edges_in[3 * k + 1];
  if (v0 < 0 || v0 >= d.N || v1 < 0 || v1 >= d.N || v0 == v1) return;      // k_check's
  const int u0 = free_index(v0, d.loop), u1 = free_index(v1, d.loop);
  if (u0 < 0 || u1 < 0) return;
  const int a = v.perm[u0], b = v.perm[u1];
  const int blk = find_block(v, max(a, b), min(a, b));
  if (blk < 0 || !v.ablk[blk]) atomicMin(&d.ctl->status, (int32_t)MCS_ERR_ARG);
}

__global__ __launch_bounds__(256) void k_sp_zero(Dev d, double* A0, size_t na) {
  if (step_off(d) || !d.ctl->lm.lin) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (size_t)gridDim.x * 256) A0[i] = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)d.n; i += (size_t)gridDim.x * 256) d.b0[i] = 0.0;
}

// k_assemble with the plan's slots: one wave per sorted item, the wave of a block's first item
// adds the block over its items in order
__global__ __launch_bounds__(256) void k_sp_assemble(Dev d, SpView v, double* A0) {
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
  const int pa = v.perm[a], pb = v.perm[b];
  int W = 0;
  const int64_t off = block_entry(v, 7, max(pa, pb), min(pa, pb), &W);      // k_sp_check: the block exists
  if (lane < 49 && off >= 0) {
    if (pa > pb) A0[off + (int64_t)i7 * W + j7] = sum;
    else if (pa < pb) A0[off + (int64_t)j7 * W + i7] = sum;
    else if (i7 >= j7) A0[off + (int64_t)i7 * W + j7] = sum;
  }
  if (diag && lane < 7) d.b0[7 * a + lane] = bsum;
}

// levels [lo, hi): one level with a workgroup per supernode, or several levels of one supernode
// each run by workgroup 0 in order
__global__ __launch_bounds__(kSpThreads) void k_sp_factor(Dev d, SpView v, SpNum m, int lo, int hi) {
  if (step_off(d)) return;
  m.lambda = d.ctl->lm.lambda;
  DevExec ex{(int)threadIdx.x, (int)blockDim.x, &d.ctl->flag};
  if (hi - lo == 1) {
    sn_factor<kSpBlock>(v, m, v.lvlsn[v.lvlptr[lo] + blockIdx.x], ex);
    return;
  }
  if (blockIdx.x != 0) return;
  for (int l = lo; l < hi; l++) sn_factor<kSpBlock>(v, m, v.lvlsn[v.lvlptr[l]], ex);
}

__global__ __launch_bounds__(kSpThreads) void k_sp_backward(Dev d, SpView v, SpNum m, int lo, int hi) {
  if (step_off(d)) return;
  DevExec ex{(int)threadIdx.x, (int)blockDim.x, &d.ctl->flag};
  if (hi - lo == 1) {
    sn_backward<kSpBlock>(v, m, v.lvlsn[v.lvlptr[lo] + blockIdx.x], ex);
    return;
  }
  if (blockIdx.x != 0) return;
  for (int l = hi - 1; l >= lo; l--) sn_backward<kSpBlock>(v, m, v.lvlsn[v.lvlptr[l]], ex);
}

}  // namespace esg
}  // namespace mcs

struct mcs_essgraph_plan {
  int device = -1, max_edges = 0, max_points = 0;
  mcs::esg::SparsePlan hp;
  mcs::esg::SpView dv{};
  mcs::esg::Ctl* ctl = nullptr;
  double *S = nullptr, *Sbak = nullptr, *C = nullptr, *err = nullptr, *J = nullptr;
  double *A0 = nullptr, *L = nullptr, *LT = nullptr, *D = nullptr, *b0 = nullptr, *y = nullptr, *u = nullptr, *xp = nullptr,
         *x = nullptr, *part = nullptr;
  uint64_t *ekey_in = nullptr, *ekey_out = nullptr;
  int32_t *eval_in = nullptr, *perm = nullptr, *edges = nullptr;
  uint32_t *ikey = nullptr, *ival = nullptr, *skey = nullptr, *sval = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0, device_bytes = 0;
  std::vector<void*> owned;
};

extern "C" {

void mcs_essgraph_plan_default_options(mcs_essgraph_plan_options* o) {
  if (o) o->leaf_size = mcs::esg::kPlanDefaultLeaf;
}

void mcs_essgraph_plan_destroy(mcs_essgraph_plan* p) {
  if (!p) return;
  if (p->device >= 0) (void)hipSetDevice(p->device);
  for (void* q : p->owned) (void)hipFree(q);
  delete p;
}

int mcs_essgraph_plan_create(int32_t device, int32_t n_kf, int32_t loop_index, const int32_t* edges, int32_t n_edges,
                             int32_t max_edges, int32_t max_points, const mcs_essgraph_plan_options* options,
                             mcs_essgraph_plan** out) {
  using namespace mcs;
  if (!out || n_kf < 1 || n_edges < 0 || max_edges < 0 || max_points < 0)
    return host::bad_arg("essential graph plan: bad argument");
  max_edges = std::max(max_edges, n_edges);
  if ((int64_t)max_edges * 14 >= INT_MAX / 8) return host::bad_arg("essential graph plan: bad counts");
  mcs_essgraph_plan* p = new mcs_essgraph_plan;
  std::string err;
  if (int rc = esg::plan_build(n_kf, loop_index, edges, n_edges, options ? options->leaf_size : 0, esg::kSpBlock, &p->hp,
                               &err)) {
    delete p;
    set_error(err.c_str());
    return rc;
  }
  p->max_edges = max_edges; p->max_points = max_points;
  if (device < 0) {            // a host-only plan: info and arrays, no device storage
    *out = p;
    return MCS_OK;
  }
  if (int rc = host::open_device(device, "essential graph plan")) { delete p; return rc; }
  p->device = device;
  hipError_t e = hipSuccess;
  auto get = [&](auto** q, size_t bytes) {
    void* r = nullptr;
    bytes = std::max<size_t>(16, bytes);
    if (e == hipSuccess) e = hipMalloc(&r, bytes);
    if (r) { p->owned.push_back(r); p->device_bytes += bytes; }
    *q = static_cast<std::remove_pointer_t<decltype(q)>>(r);
  };
  auto up = [&](auto** q, const auto& vec) {
    using T = std::remove_const_t<std::remove_pointer_t<std::remove_pointer_t<decltype(q)>>>;
    T* r = nullptr;
    get(&r, vec.size() * sizeof(T));
    if (e == hipSuccess && !vec.empty()) e = hipMemcpy(r, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice);
    *q = r;
  };
  const esg::SparsePlan& h = p->hp;
  esg::SpView& v = p->dv;
  v.n = h.n; v.S = h.S;
  up(&v.perm, h.perm); up(&v.iperm, h.iperm); up(&v.sn_of, h.sn_of); up(&v.col0, h.col0); up(&v.rowptr, h.rowptr);
  up(&v.rows, h.rows); up(&v.blkoff, h.blkoff); up(&v.srcptr, h.srcptr); up(&v.src_s, h.src_s); up(&v.src_p0, h.src_p0);
  up(&v.src_p1, h.src_p1); up(&v.src_map, h.src_map); up(&v.relmap, h.relmap); up(&v.lvlptr, h.lvlptr);
  up(&v.lvlsn, h.lvlsn); up(&v.ablk, h.ablk);
  const size_t Em = std::max(1, max_edges), Nm = (size_t)n_kf, B = esg::kSpBlock;
  const size_t na = (size_t)h.panel_blocks * B * B, nb = B * (size_t)std::max(1, h.n);
  get(&p->ctl, sizeof(esg::Ctl));
  get(&p->S, 64 * Nm); get(&p->Sbak, 64 * Nm); get(&p->C, 64 * Em); get(&p->err, 56 * Em); get(&p->J, 784 * Em);
  get(&p->A0, 8 * na); get(&p->L, 8 * na); get(&p->LT, 8 * na); get(&p->D, 8 * nb); get(&p->b0, 8 * nb); get(&p->y, 8 * nb);
  get(&p->u, 8 * B * (size_t)std::max<int64_t>(1, h.row_blocks)); get(&p->xp, 8 * nb); get(&p->x, 8 * nb);
  get(&p->part, 8 * esg::kChiBlocks);
  get(&p->ekey_in, 8 * Em); get(&p->ekey_out, 8 * Em); get(&p->eval_in, 4 * Em); get(&p->perm, 4 * Em);
  get(&p->edges, 12 * Em);
  get(&p->ikey, 12 * Em); get(&p->ival, 12 * Em); get(&p->skey, 12 * Em); get(&p->sval, 12 * Em);
  size_t b1 = 0, b2 = 0;
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, b1, p->ekey_in, p->ekey_out, p->eval_in, p->perm, Em, 0u, 64u, (hipStream_t)0);
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, b2, p->ikey, p->skey, p->ival, p->sval, 3 * Em, 0u, 32u, (hipStream_t)0);
  p->tmp_bytes = std::max<size_t>(16, std::max(b1, b2));
  get(&p->tmp, p->tmp_bytes);
  if (e != hipSuccess) {
    mcs_essgraph_plan_destroy(p);
    set_hip_error(e, "essential graph plan", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = p;
  return MCS_OK;
}

int mcs_essgraph_plan_get_info(const mcs_essgraph_plan* p, mcs_essgraph_plan_info* o) {
  using namespace mcs;
  if (!p || !o) return host::bad_arg("essential graph plan info: null argument");
  const esg::SparsePlan& h = p->hp;
  o->n_kf = h.N; o->loop_index = h.loop; o->free_blocks = h.n; o->leaf_size = h.leaf; o->supernodes = h.S;
  o->levels = h.levels; o->max_supernode_columns = h.max_cols;
  o->solver_launches_per_trial = 2 * (int32_t)h.launch_lo.size();
  o->launches_per_trial = esg::kPlanFixedLaunches + o->solver_launches_per_trial;
  o->a_blocks = h.a_blocks; o->l_blocks = h.l_blocks; o->panel_blocks = h.panel_blocks;
  o->flops_per_factor = h.flops; o->device_bytes = (int64_t)p->device_bytes; o->digest = h.digest;
  return MCS_OK;
}

int mcs_essgraph_plan_get_arrays(const mcs_essgraph_plan* p, mcs_essgraph_plan_arrays* o) {
  using namespace mcs;
  if (!p || !o) return host::bad_arg("essential graph plan arrays: null argument");
  const esg::SparsePlan& h = p->hp;
  o->perm = h.perm.data(); o->col0 = h.col0.data(); o->row_ptr = h.rowptr.data(); o->rows = h.rows.data();
  o->n_rows = (int32_t)h.rows.size(); o->parent = h.parent.data(); o->level = h.level.data();
  o->block_off = h.blkoff.data(); o->a_block = h.ablk.data();
  return MCS_OK;
}

int mcs_optimize_essential_graph_planned_device(mcs_essgraph_plan* pl, int32_t N, const double* d_Scw, const double* d_Snc,
                                                int32_t loop_index, int32_t E, const int32_t* d_edges,
                                                int32_t P, double* d_point_pos, const int32_t* d_point_ref,
                                                const uint8_t* d_point_bad, const mcs_essgraph_options* opts,
                                                const mcs_essgraph_out* out, void* stream) {
  using namespace mcs;
  if (!pl || pl->device < 0) return host::bad_arg("essential graph: no plan, or a host-only plan");
  {
    using host::bad_arg;
    if (!opts || !out || !out->status) return bad_arg("essential graph: null options, out or out->status");
    if (N < 1 || E < 0 || P < 0) return bad_arg("essential graph: bad counts");
    if (!d_Scw || !d_Snc || (E > 0 && !d_edges) || (P > 0 && (!d_point_pos || !d_point_ref || !d_point_bad)))
      return bad_arg("essential graph: null buffer");
    if (loop_index < 0 || loop_index >= N) return bad_arg("essential graph: loop_index outside the keyframes");
    if (opts->iterations < 0 || opts->iterations > MCS_ESSGRAPH_MAX_ITERATIONS)
      return bad_arg("essential graph: iterations outside [0, 64]");
    if (opts->max_trials < 1 || opts->max_trials > MCS_ESSGRAPH_MAX_TRIALS)
      return bad_arg("essential graph: max_trials outside [1, 64]");
    if (E > pl->max_edges || P > pl->max_points) return bad_arg("essential graph: more edges or points than the plan holds");
  }
  MCS_HIP_CHECK(hipSetDevice(pl->device));
  hipStream_t st = (hipStream_t)stream;
  const esg::SparsePlan& h = pl->hp;
  const bool match = N == h.N && loop_index == h.loop;     // else k_sp_check refuses the call; nothing is sized by N then

  esg::Dev d{};
  d.ctl = pl->ctl;
  d.N = N; d.E = E; d.P = P; d.loop = loop_index; d.n = 7 * (N - 1);
  d.T = 1; d.D = 1;
  d.Scw = d_Scw; d.Snc = d_Snc; d.edges_in = d_edges;
  d.S = pl->S; d.Sbak = pl->Sbak; d.C = pl->C; d.err = pl->err; d.J = pl->J;
  d.edges = pl->edges; d.perm = pl->perm; d.ikey = pl->ikey; d.ival = pl->ival; d.skey = pl->skey; d.sval = pl->sval;
  d.A0 = pl->A0; d.b0 = pl->b0; d.A = pl->L; d.b = pl->b0; d.x = pl->x; d.part = pl->part;
  d.point_pos = d_point_pos; d.point_ref = d_point_ref; d.point_bad = d_point_bad;
  const esg::SpView v = pl->dv;
  esg::SpNum m{pl->A0, 0.0, pl->L, pl->LT, pl->D, pl->b0, pl->y, pl->u, pl->xp, pl->x};

  esg::Ctl h0{};
  mcs_ba_options bo{};
  bo.max_iterations = opts->iterations; bo.gain_threshold = opts->gain_threshold;
  bo.terminate_max_iter = opts->terminate_max_iter; bo.max_trials = opts->max_trials; bo.tau = 0.0;
  ba::lm_init(h0.lm, bo);
  h0.lm.done = 1;              // until k_end's start pass has the first chi2
  h0.lambda0 = opts->lambda0;
  auto gb = [](int n) { return dim3((unsigned)((std::max(n, 1) + 255) / 256)); };
  const int nchi = std::max(1, std::min(esg::kChiBlocks, (E + 255) / 256));
  const size_t na = (size_t)h.panel_blocks * 49;
  const unsigned gz = (unsigned)std::max<size_t>(1, std::min<size_t>(2048, (na + 255) / 256));
  auto fail = [&](hipError_t e) { set_hip_error(e, "essential graph", __FILE__, __LINE__); return (int)MCS_ERR_HIP; };

  hipLaunchKernelGGL(esg::k_init, dim3(1), dim3(256), 0, st, h0, pl->ctl);
  hipLaunchKernelGGL(esg::k_check, gb(std::max(E, P)), dim3(256), 0, st, d);
  hipLaunchKernelGGL(esg::k_sp_check, gb(E), dim3(256), 0, st, d, v, (int)h.N, (int)h.loop);
  if (E > 0) {
    hipLaunchKernelGGL(esg::k_edge_keys, gb(E), dim3(256), 0, st, d, pl->ekey_in, pl->eval_in);
    size_t b = pl->tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(pl->tmp, b, pl->ekey_in, pl->ekey_out, pl->eval_in, pl->perm, (size_t)E, 0u, 64u, st);
    if (e != hipSuccess) return fail(e);
  }
  if (match) hipLaunchKernelGGL(esg::k_setup, gb(std::max(N, E)), dim3(256), 0, st, d);
  if (E > 0 && match) {
    size_t b = pl->tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(pl->tmp, b, pl->ikey, pl->skey, pl->ival, pl->sval, 3 * (size_t)E, 0u, 32u, st);
    if (e != hipSuccess) return fail(e);
  }
  hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 1, (double*)nullptr);
  hipLaunchKernelGGL(esg::k_end, dim3(1), dim3(256), 0, st, d, nchi, 1, (int)opts->iterations);
  const int steps = (match && d.n > 0 && E > 0) ? opts->iterations * opts->max_trials : 0;
  const int nl = (int)h.launch_lo.size();
  auto grid_of = [&](int k) {
    return dim3(h.launch_hi[k] - h.launch_lo[k] == 1 ? (unsigned)(h.lvlptr[h.launch_lo[k] + 1] - h.lvlptr[h.launch_lo[k]]) : 1u);
  };
  for (int g = 0; g < steps; g++) {
    hipLaunchKernelGGL(esg::k_linearise, gb(14 * E), dim3(256), 0, st, d);
    hipLaunchKernelGGL(esg::k_sp_zero, dim3(gz), dim3(256), 0, st, d, pl->A0, na);
    hipLaunchKernelGGL(esg::k_sp_assemble, dim3((unsigned)((3 * E + 3) / 4)), dim3(256), 0, st, d, v, pl->A0);
    for (int k = 0; k < nl; k++)
      hipLaunchKernelGGL(esg::k_sp_factor, grid_of(k), dim3(esg::kSpThreads), 0, st, d, v, m, (int)h.launch_lo[k],
                         (int)h.launch_hi[k]);
    for (int k = nl - 1; k >= 0; k--)
      hipLaunchKernelGGL(esg::k_sp_backward, grid_of(k), dim3(esg::kSpThreads), 0, st, d, v, m, (int)h.launch_lo[k],
                         (int)h.launch_hi[k]);
    hipLaunchKernelGGL(esg::k_update, gb(N), dim3(256), 0, st, d);
    hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 0, (double*)nullptr);
    hipLaunchKernelGGL(esg::k_end, dim3(1), dim3(256), 0, st, d, nchi, 0, (int)opts->iterations);
  }
  hipLaunchKernelGGL(esg::k_poses, gb(N), dim3(256), 0, st, d, *out);
  if (P > 0) hipLaunchKernelGGL(esg::k_points, gb(P), dim3(256), 0, st, d);
  if (out->edge_chi2 && E > 0) hipLaunchKernelGGL(esg::k_chi2, dim3(nchi), dim3(256), 0, st, d, 1, out->edge_chi2);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? (int)MCS_OK : fail(e);
}

int mcs_optimize_essential_graph_sparse(int32_t device, int32_t N, const double* Scw, const double* Snc,
                                        int32_t loop_index, int32_t E, const int32_t* edges, int32_t P,
                                        double* point_pos, const int32_t* point_ref, const uint8_t* point_bad,
                                        const mcs_essgraph_options* opts, const mcs_essgraph_out* out) {
  using namespace mcs;
  if (!opts || !out || !out->status) return host::bad_arg("essential graph: null options, out or out->status");
  if (N < 1 || E < 0 || P < 0 || !Scw || !Snc || (E > 0 && !edges) || (P > 0 && (!point_pos || !point_ref || !point_bad)))
    return host::bad_arg("essential graph: bad counts or null buffer");
  mcs_essgraph_plan* pl = nullptr;
  if (int rc = mcs_essgraph_plan_create(device, N, loop_index, edges, E, E, P, nullptr, &pl)) return rc;
  struct Guard { mcs_essgraph_plan* p; ~Guard() { mcs_essgraph_plan_destroy(p); } } guard{pl};
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
  int rc = mcs_optimize_essential_graph_planned_device(pl, N, dScw, dSnc, loop_index, E, dE, P, dpos, dref, dbad, opts, &d,
                                                       nullptr);
  hipError_t se = hipDeviceSynchronize();          // before the plan's storage goes
  if (rc) return rc;
  MCS_HIP_CHECK(se);
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
  if (status) { set_error("essential graph: device error"); return status; }
  return MCS_OK;
}

}  // extern "C"
