// One optimize() call on the device: structure, upload, the host-driven and the device-driven
// Levenberg-Marquardt loops, LocalBA's device-culled tails and the result download.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "ba_ctx.hpp"
#include "ba_kernels.hpp"
#include "ba_lba.hpp"
#include "ba_pairs.hpp"
#include "ba_reduce.hpp"
#include "lm_control.hpp"

namespace {

// One optimize() call split in two so that LocalBA's second round can reuse the first
// round's device state: setup() = initializeOptimization + buildStructure + the problem
// upload; remask() = the same graph with more edges at level 1 (the culled ones: their
// per-edge terms are zeroed once and the active-edge list shrinks, nothing else moves);
// run() = SparseOptimizer::optimize (LM iterations) + the result download.
struct Optimizer {
  mcs_ba_ctx* c;
  const mcs_ba_problem* p;
  bool points_fixed;
  Shard sh;
  bool sharded = false;
  hipStream_t st = nullptr;
  HostStruct& s;
  Dev d;
  int n = 0, T = 1, NE = 0;
  int band = 1;          // tile bandwidth of the reduced camera system (ldlt::Work::band)
  int64_t pmax = 0;      // upper bound of the Schur pairs (device-built lists)
  int items_max = 1;     // upper bound of the k_schur work items
  int32_t* it_nch_dev = nullptr;   // chunks of each item's block (checked by the test hook)
  int nblk = 0;
  XLayout X{1, 0};
  size_t xs_count = 0;   // doubles of the per-trial exchange: bs + the non-zero diagonals of S
  int nl_glob = 0, nae_glob = 0;
  double *d_poses = nullptr, *d_points = nullptr, *d_scalar = nullptr, *d_part = nullptr;
  int* d_flag = nullptr;
  ldlt::Work lw;
  unsigned g_state = 1;
  hipError_t he = hipSuccess;
  // what run_device does after the LM loop
  enum class LbaTail {
    Download,      // the plain download
    Round1,        // cull + compaction, no download
    Round2,        // cull + results
    Round2NoCull,  // results only (empty graph)
  };
  // LocalBA culling on the device (mcs_local_ba_ex with the device-driven LM): set on and extra
  // before setup()
  struct Lba {
    bool on = false;
    const int32_t* extra = nullptr;
    LbaState L{};
    LbaTail tail = LbaTail::Download;
    int32_t res[3] = {0, 0, 0};   // round 1: active edges left, a pose left the system, points left
    uint8_t* inlier_out = nullptr;
    uint8_t* pwrite_out = nullptr;
  } lba;

  Optimizer(mcs_ba_ctx* c_, const mcs_ba_problem* p_, bool pf) : c(c_), p(p_), points_fixed(pf), s(c_->hs) {
    std::memset(&d, 0, sizeof(d));
  }
  double* dz(size_t cnt_) {
    double* q = (double*)c->alloc(std::max<size_t>(1, cnt_) * 8);
    if (!q) he = hipErrorOutOfMemory;
    return q;
  }
  // collective over xchg[off, off+cnt); no-op on one rank.  Stream-ordered shards get it
  // enqueued on st behind the producing kernels; otherwise the stream is drained first and the
  // callback completes it (its host time is the exchange stage).
  int allreduce(int op, size_t off, size_t cnt) {
    if (!sharded || cnt == 0) return MCS_OK;
    if (!sh.ordered) MCS_HIP_CHECK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (sh.fn(sh.user, op, (int64_t)off, (int64_t)cnt, (void*)st) != 0) {
      set_error("BA: allreduce callback failed");
      return MCS_ERR_HIP;
    }
    if (c->timing && !sh.ordered)
      c->acc_ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MCS_OK;
  }
  // all-reduce host scalars through the tail of the exchange buffer
  int allreduce_host(double* v, int cnt, int op, size_t off) {
    if (!sharded) return MCS_OK;
    MCS_HIP_CHECK(hipMemcpyAsync(sh.xchg + off, v, 8 * (size_t)cnt, hipMemcpyHostToDevice, st));
    int rc = allreduce(op, off, cnt);
    if (rc) return rc;
    MCS_HIP_CHECK(hipMemcpyAsync(v, sh.xchg + off, 8 * (size_t)cnt, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipStreamSynchronize(st));
    return MCS_OK;
  }

  // the problem's own arrays (and the trial backups' space) into a packed upload
  void add_problem(Packer& pk, const double* poses, const double* points, double** poses_bk,
                   double** points_bk) {
    pk.add(&d.mc, p->mc, 6 * (size_t)p->n_cams);
    pk.add(&d.cam, p->cam, 17 * (size_t)p->n_cams);
    pk.add(&d.e_pose, p->edge_pose, (size_t)NE);
    pk.add(&d.e_point, p->edge_point, (size_t)NE);
    pk.add(&d.e_cam, p->edge_cam, (size_t)NE);
    pk.add(&d.e_meas, p->edge_meas, 2 * (size_t)NE);
    pk.add(&d.e_info, p->edge_info, (size_t)NE);
    pk.add(&d_poses, poses, 6 * (size_t)p->n_poses);
    pk.add(&d_points, points, 3 * (size_t)p->n_points);
    // the trial backups are written by every trial's push before anything reads them: space only
    pk.add(poses_bk, static_cast<const double*>(nullptr), 6 * (size_t)p->n_poses);
    pk.add(points_bk, static_cast<const double*>(nullptr), 3 * (size_t)p->n_points);
  }

  int setup(const double* poses, const double* points, const uint8_t* edge_level,
            const mcs_ba_shard* shard_in) {
    if (p->n_poses < 0 || p->n_points < 0 || p->n_edges < 0 || p->n_cams < 1) return MCS_ERR_ARG;
    HostClock hc;
    c->host_calls++;
    // ---- structure, pass 1: the index checks, the active edges and their per-pose / per-point
    // counts (+ active point / edge counts), all-reduced over the shards below
    std::vector<double> cnt;
    mcs::HostPool* const pool = c->pool_for(p->n_edges);
    if (!scan_edges(*p, edge_level, points_fixed, s, cnt, pool)) {
      set_error("edge vertex index out of range");
      return MCS_ERR_ARG;
    }
    MCS_HIP_CHECK(hipSetDevice(c->device));
    if (shard_in && shard_in->world > 1) {
      if (!shard_in->xchg || !shard_in->allreduce || shard_in->rank < 0 || shard_in->rank >= shard_in->world ||
          shard_in->xchg_cap < xchg_doubles(p->n_poses)) {
        set_error("invalid mcs_ba_shard (exchange buffer too small or no allreduce callback)");
        return MCS_ERR_ARG;
      }
      sh.rank = shard_in->rank; sh.world = shard_in->world; sh.xchg = shard_in->xchg;
      sh.fn = shard_in->allreduce; sh.user = shard_in->user;
      sh.ordered = shard_in->stream_ordered != 0;
    }
    sharded = sh.world > 1;
    st = c->st;
    c->free_all();
    if (!sharded) {
      sh.xchg = (double*)c->alloc((size_t)xchg_doubles(p->n_poses) * 8);
      if (!sh.xchg) { set_error("BA: out of device memory"); return MCS_ERR_HIP; }
    }
    // ---- threaded (config-E-sized) calls: the problem arrays go up now, their copy
    // overlapping the structure build; the structure arrays follow from the second staging
    // buffer (GlobalBA 6.15 / 6.20 -> 5.86 / 5.47 ms per call, profiles/r06_split_ab.txt).  The
    // second flush relies on this first one's spin_sync (Packer::flush): split implies it ran.
    NE = p->n_edges;
    double *d_poses_bk = nullptr, *d_points_bk = nullptr;
    const bool split = pool != nullptr;
    if (split) {
      Packer pk;
      add_problem(pk, poses, points, &d_poses_bk, &d_points_bk);
      if ((he = pk.flush(c, pool)) != hipSuccess) MCS_HIP_CHECK(he);
    }
    // ---- global pose activity (+ active point / edge counts)
    int rc;
    if ((rc = allreduce_host(cnt.data(), p->n_poses + 2, MCS_REDUCE_SUM, 0))) return rc;
    hc.mark(c->host_ms, 0);
    build_structure(*p, points_fixed, cnt, s, pool);
    hc.mark(c->host_ms, 1);
    nl_glob = (int)cnt[p->n_poses];
    nae_glob = (int)cnt[p->n_poses + 1];
    n = 6 * s.np;
    T = ldlt::tiles_for(std::max(1, n));
    X = XLayout(T, s.np);
    xs_count = X.hdiag - X.bs;
    band = T;
    if (T > 1) {
      // Tiles of S below the widest tile diagonal any rank's points touch are zero on every
      // rank (their blocks have no pairs; the padding rows there are zero too), and LDL^T keeps
      // a banded matrix's L inside the same band: the factorisation runs on diagonals 0 .. w
      // only (ldlt::Work::band), and the sharded exchange stops at diagonal w too.
      std::vector<int> wpart(pool ? pool->size() : 1, 1);   // >= 1: pose blocks straddling a tile boundary
      auto span = [&](int t, int nt) {
        const int q0 = (int)((int64_t)s.nl * t / nt), q1 = (int)((int64_t)s.nl * (t + 1) / nt);
        int w = 1;
        for (int q = q0; q < q1; q++) {
          int lo = INT32_MAX, hi = -1;
          for (int e = s.pt_ptr[q]; e < s.pt_ptr[q + 1]; e++) {
            const int h = s.pt_h[e];
            if (h >= 0) { lo = std::min(lo, h); hi = std::max(hi, h); }
          }
          if (hi >= 0) w = std::max(w, (6 * hi + 5) / ldlt::TB - (6 * lo) / ldlt::TB);
        }
        wpart[t] = w;
      };
      if (pool && s.nl >= 4096) pool->run([&](int t) { span(t, (int)wpart.size()); });
      else span(0, 1);
      double wd = *std::max_element(wpart.begin(), wpart.end());
      if ((rc = allreduce_host(&wd, 1, MCS_REDUCE_MAX, X.sc))) return rc;
      band = ldlt::pipe_band(T, (int)wd + 1);
      if (sharded) xs_count = (size_t)ldlt::TB * T + ldlt::band_tiles((int)wd + 1, T) * ldlt::TB * ldlt::TB;
    }
    // the forced modes factor densely; the exchange above keeps the derived band
    if (c->ldlt_mode != 0) band = T;
    if (c->ldlt_mode == 1 && T >= 2 && !ldlt::pipe_supported(T, T)) {
      set_error("BA: the dense pipelined factorisation (mcs_ba_set_ldlt_mode 1) takes at most 96 tiles");
      return MCS_ERR_UNSUPPORTED;
    }
    const bool pipelined = T >= 2 && c->ldlt_mode != 2 && ldlt::pipe_supported(T, band);
    // mode 2 with the multi-workgroup backward substitution (the pipeline's sync words, no tasks):
    // the same operations in the same order as the pipeline; above 96 tiles the one-workgroup one
    const bool per_step_sync = T >= 2 && c->ldlt_mode == 2 && ldlt::pipe_supported(T, T);
    if (!pipelined && (size_t)T * ldlt::TB * 8 > 96 * 1024) {
      set_error(c->ldlt_mode == 2
                    ? "BA: the per-step factorisation (mcs_ba_set_ldlt_mode 2) takes at most 2048 active poses"
                    : "more than 2048 active poses with a reduced camera system too wide for the banded "
                      "factorisation (its task table exceeds the pipeline's bound)");
      return MCS_ERR_UNSUPPORTED;
    }
    c->shape_n = n; c->shape_T = T; c->shape_band = pipelined ? band : T; c->shape_pipe = pipelined ? 1 : 0;
    {
      Packer pk;
      if (!split) add_problem(pk, poses, points, &d_poses_bk, &d_points_bk);
      // every edge active (LocalBA round 1, GlobalBA): no list, the kernels index edges directly
      if ((int)s.aedge.size() != NE) pk.add(&d.aedge, s.aedge);
      else d.aedge = nullptr;
      pk.add(&d.pose_h, s.pose_h); pk.add(&d.point_h, s.point_h);
      pk.add(&d.hpose_vtx, s.hpose_vtx); pk.add(&d.hpt_vtx, s.hpt_vtx);
      pk.add(&d.pt_ptr, s.pt_ptr); pk.add(&d.pt_edges, s.pt_edges); pk.add(&d.pt_h, s.pt_h);
      pk.add(&d.ps_ptr, s.ps_ptr); pk.add(&d.ps_edges, s.ps_edges);
      pk.add(&d.blk_i, s.blk_i); pk.add(&d.blk_j, s.blk_j);
      if (lba.on && lba.extra) pk.add(&lba.L.extra, lba.extra, (size_t)p->n_points);
      he = pk.flush(c, pool, split);
    }
    d.delta = p->huber_delta;
    d.dsqr = huber_dsqr(p->huber_delta);
    d.poses = d_poses; d.points = d_points; d.poses_bk = d_poses_bk; d.points_bk = d_points_bk;
    d.nae = (int)s.aedge.size();
    d.np = s.np; d.nl = s.nl;
    d.npe = (int)s.pt_edges.size();
    d.err = dz(2 * (size_t)NE); d.w = dz(NE); d.jp = dz(12 * (size_t)NE); d.jl = dz(6 * (size_t)NE);
    d.hpl = dz(18 * (size_t)NE); d.y = dz(18 * (size_t)NE); d.chi = dz(NE); d.rchi = dz(NE);
    // the second linearisation buffer (device-driven runs: speculative linearisation)
    if (!sharded) {
      d.alt_err = dz(2 * (size_t)NE); d.alt_w = dz(NE); d.alt_jp = dz(12 * (size_t)NE);
      d.alt_jl = dz(6 * (size_t)NE); d.alt_hpl = dz(18 * (size_t)NE);
    } else {
      d.alt_err = d.alt_w = d.alt_jp = d.alt_jl = d.alt_hpl = nullptr;
    }
    d.Hpp = dz(36 * (size_t)s.np); d.bp = dz(6 * (size_t)s.np);
    d.Hll = dz(9 * (size_t)s.nl); d.bl = dz(3 * (size_t)s.nl);
    d.Dinv = dz(9 * (size_t)s.nl); d.db = dz(3 * (size_t)s.nl);
    d.S = sh.xchg + X.S; d.bs = sh.xchg + X.bs; d.hdiag = sh.xchg + X.hdiag; d.bpf = sh.xchg + X.bpf;
    d.T = T;
    d.xp = dz((size_t)ldlt::TB * T);
    d.red = dz((size_t)NE + 6 * (size_t)s.np + s.nl + 16);
    // bounds of the device-built pair lists / items: a point with k active edges gives at most
    // k^2 pairs (k (k + 1) / 2 when its edges have distinct poses, as the reference's one
    // observation per keyframe makes them; the C-ABI takes any graph); a block at most
    // 1 + pairs / CH + pose edges / CH chunks
    nblk = s.np * (s.np + 1) / 2;
    pmax = 0;
    for (int l = 0; l < s.nl; l++) {
      const int64_t k = s.pt_ptr[l + 1] - s.pt_ptr[l];
      pmax += k * k;
    }
    if (pmax > INT32_MAX) { set_error("BA: more than 2^31 Schur pairs"); return MCS_ERR_UNSUPPORTED; }
    items_max = (int)std::min<int64_t>(INT32_MAX, 2 * (int64_t)nblk + pmax / kSchurChunk +
                                                       s.ps_ptr[s.np] / kSchurChunk + 1);
    d.schur_part = dz((size_t)items_max * 42);

    lw.L = dz(ldlt::tile_doubles(T));
    lw.Linv = dz((size_t)T * ldlt::TB * ldlt::TB);
    lw.z = dz((size_t)ldlt::TB * T);
    // pipelined factorisation (one launch per solve) for every multi-tile system
    lw.W = nullptr; lw.du = nullptr; lw.sync = nullptr; lw.tasks = nullptr; lw.ntasks = 0; lw.pipe_T = 0;
    lw.band = 0; lw.per_step = false;
    if (per_step_sync) {
      lw.sync = (unsigned*)dz((ldlt::pipe_sync_words(T, T) + 1) / 2);
      lw.pipe_T = T;
      lw.band = T;
      lw.per_step = true;
    }
    if (pipelined) {
      const std::vector<int4>& tq = ldlt::pipe_tasks_host(T, band);
      lw.W = dz(ldlt::tile_doubles(T));
      lw.du = dz((size_t)T * 128);
      lw.sync = (unsigned*)dz((ldlt::pipe_sync_words(T, band) + 1) / 2);
      lw.tasks = (int4*)dz(2 * tq.size());
      if (he == hipSuccess && lw.tasks)
        he = hipMemcpyAsync(lw.tasks, tq.data(), tq.size() * sizeof(int4), hipMemcpyHostToDevice, st);
      lw.ntasks = (int)tq.size();
      lw.pipe_T = T;
      lw.band = band;
    }
    // scalars: [0] chi2 [1] point scale [2] pose scale [3] chi_now; the solve flag in [5] (one
    // 48-byte readback per trial)
    d_scalar = dz(8);
    d_part = dz(kRedPartMax);
    d_flag = reinterpret_cast<int*>(d_scalar + 5);
    if (lba.on) {
      LbaState& L = lba.L;
      const size_t npt = (size_t)std::max(1, p->n_points), ne = (size_t)std::max(1, NE);
      L.obs_left = (int32_t*)c->alloc(4 * npt);
      L.edges_left = (int32_t*)c->alloc(4 * npt);
      L.edges_all = (int32_t*)c->alloc(4 * npt);
      L.bad = (uint8_t*)c->alloc(npt);
      L.pwrite = (uint8_t*)c->alloc(npt);
      L.inlier = (uint8_t*)c->alloc(ne);
      L.level = (uint8_t*)c->alloc(ne);
      L.pose_cnt = (int32_t*)c->alloc(4 * (size_t)std::max(1, s.np));
      L.ctr = (uint32_t*)c->alloc(16);
      L.res = c->pinned_i;   // written by k_lba_count straight into host memory
      L.chi = d.chi;
      L.k2 = p->huber_delta * p->huber_delta;
      if (!L.obs_left || !L.edges_left || !L.edges_all || !L.bad || !L.pwrite || !L.inlier || !L.level ||
          !L.pose_cnt || !L.ctr)
        he = hipErrorOutOfMemory;
      else
        hipLaunchKernelGGL(k_lba_init, dim3(gb(std::max(NE, p->n_points))), dim3(256), 0, st, d, L, NE,
                           p->n_points);
    }
    if (he != hipSuccess) { set_hip_error(he, "BA upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
    d.push_poses = d_poses_bk; d.push_points = d_points_bk;
    d.n_pose_dbl = 6 * p->n_poses; d.n_point_dbl = 3 * p->n_points;
    d.flag = d_flag;
    g_state = gb(std::max(d.n_pose_dbl, d.n_point_dbl));
    const int rp = enqueue_pairs();
    hc.mark(c->host_ms, 2);
    return rp;
  }

  // The Schur pair lists and k_schur items, built on the device (the kernels above), stream
  // ordered after the upload: nothing is read back.
  int enqueue_pairs() {
    const int npe = (int)s.pt_edges.size();
    int32_t* cnt = (int32_t*)c->alloc(4 * (size_t)(npe + 1));
    int32_t* off = (int32_t*)c->alloc(4 * (size_t)(npe + 1));
    uint32_t* k_in = (uint32_t*)c->alloc(4 * (size_t)std::max<int64_t>(1, pmax));
    uint32_t* k_out = (uint32_t*)c->alloc(4 * (size_t)std::max<int64_t>(1, pmax));
    uint2* v_in = (uint2*)c->alloc(8 * (size_t)std::max<int64_t>(1, pmax));
    uint2* v_out = (uint2*)c->alloc(8 * (size_t)std::max<int64_t>(1, pmax));
    int32_t* pr_ptr = (int32_t*)c->alloc(4 * (size_t)(nblk + 1));
    int32_t* nch = (int32_t*)c->alloc(4 * (size_t)(nblk + 1));
    int32_t* nslot = (int32_t*)c->alloc(4 * (size_t)(nblk + 1));
    int32_t* it_off = (int32_t*)c->alloc(4 * (size_t)(nblk + 1));
    int32_t* slot_off = (int32_t*)c->alloc(4 * (size_t)(nblk + 1));
    int32_t* it_blk = (int32_t*)c->alloc(4 * (size_t)items_max);
    int32_t* it_chunk = (int32_t*)c->alloc(4 * (size_t)items_max);
    int32_t* it_slot = (int32_t*)c->alloc(4 * (size_t)items_max);
    int32_t* it_nch = (int32_t*)c->alloc(4 * (size_t)items_max);
    int32_t* nitem = (int32_t*)c->alloc(4);
    if (!cnt || !off || !k_in || !k_out || !v_in || !v_out || !pr_ptr || !nch || !nslot || !it_off ||
        !slot_off || !it_blk || !it_chunk || !it_slot || !it_nch || !nitem) {
      set_error("BA: out of device memory (pair lists)");
      return MCS_ERR_HIP;
    }
    const unsigned bits = nblk > 0 ? 32u - (unsigned)__builtin_clz((unsigned)nblk) : 1u;
    size_t b_scan1 = 0, b_scan2 = 0, b_sort = 0;
    auto plus = rocprim::plus<int32_t>();
    MCS_HIP_CHECK(rocprim::exclusive_scan(nullptr, b_scan1, cnt, off, 0, (size_t)npe + 1, plus, st));
    MCS_HIP_CHECK(rocprim::exclusive_scan(nullptr, b_scan2, nch, it_off, 0, (size_t)nblk + 1, plus, st));
    if (pmax > 0)
      MCS_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, b_sort, k_in, k_out, v_in, v_out, (size_t)pmax, 0u, bits, st));
    const size_t tb = std::max(std::max(b_scan1, b_scan2), b_sort) + 256;
    void* tmp = c->alloc(tb);
    if (!tmp) { set_error("BA: out of device memory (scan storage)"); return MCS_ERR_HIP; }
    size_t b = tb;
    hipLaunchKernelGGL(k_pair_count, dim3(gb(npe + 1)), dim3(256), 0, st, d, cnt);
    MCS_HIP_CHECK(rocprim::exclusive_scan(tmp, b, cnt, off, 0, (size_t)npe + 1, plus, st));
    if (pmax > 0) {
      const unsigned g = std::max(gb(npe), std::min(gb((int)std::min<int64_t>(pmax, INT32_MAX)), 4096u));
      hipLaunchKernelGGL(k_pair_emit, dim3(g), dim3(256), 0, st, d, (const int32_t*)off, k_in, v_in, pmax,
                         (uint32_t)nblk);
      b = tb;
      MCS_HIP_CHECK(rocprim::radix_sort_pairs(tmp, b, k_in, k_out, v_in, v_out, (size_t)pmax, 0u, bits, st));
    }
    hipLaunchKernelGGL(k_block_ptr, dim3(gb(nblk + 1)), dim3(256), 0, st, d, (const uint32_t*)k_out, pmax,
                       nblk, pr_ptr, nch, nslot);
    b = tb;
    MCS_HIP_CHECK(rocprim::exclusive_scan(tmp, b, nch, it_off, 0, (size_t)nblk + 1, plus, st));
    b = tb;
    MCS_HIP_CHECK(rocprim::exclusive_scan(tmp, b, nslot, slot_off, 0, (size_t)nblk + 1, plus, st));
    hipLaunchKernelGGL(k_block_items, dim3(gb(nblk + 1)), dim3(256), 0, st, nblk, (const int32_t*)nch,
                       (const int32_t*)it_off, (const int32_t*)slot_off, it_blk, it_chunk, it_slot, it_nch,
                       nitem);
    MCS_HIP_CHECK(hipGetLastError());
    d.pr_ptr = pr_ptr; d.pr = v_out;
    d.it_blk = it_blk; d.it_chunk = it_chunk; d.it_slot = it_slot;
    d.blk_nch = nch; d.blk_slot0 = slot_off;
    it_nch_dev = it_nch;
    d.nitem = nitem;
    return MCS_OK;
  }

  // More edges at level 1 (a subset of the active ones; unsharded only).  g2o re-runs
  // initializeOptimization: the culled edges leave the graph, and a vertex left without active
  // edges leaves the system.  Here the culled edges' per-edge terms (weight, Jacobians, Hpl,
  // error) are zeroed once and the active-edge list shrinks; every sum they took part in then
  // adds exact zeros, and a point left without edges keeps Hll = 0 (its update is Dinv * 0 = 0,
  // its Schur and model-decrease terms are 0).  Returns 1 (nothing changed on the device) when
  // an active pose would leave the system: the caller then rebuilds from scratch.
  int remask(const uint8_t* edge_level) {
    if (sharded) return 1;
    HostClock hc;
    std::vector<int32_t> keep;
    std::vector<int32_t> culled;
    keep.reserve(s.aedge.size());
    std::vector<int32_t> pose_left(s.np, 0);
    std::vector<char> pt_left(s.nl, 0);
    for (int e : s.aedge) {
      if (edge_level && edge_level[e]) { culled.push_back(e); continue; }
      keep.push_back(e);
      const int h = s.pose_h[p->edge_pose[e]];
      if (h >= 0) pose_left[h]++;
      const int l = s.point_h[p->edge_point[e]];
      if (l >= 0) pt_left[l] = 1;
    }
    for (int h = 0; h < s.np; h++)
      if (pose_left[h] == 0) return 1;
    int nl_left = 0;
    for (int l = 0; l < s.nl; l++) nl_left += pt_left[l];
    if (!culled.empty()) {
      const size_t nb = (keep.size() + culled.size()) * 4 + 512;
      uint8_t* h = c->stage.get(nb);   // the stream is idle: run() ended with a synchronise
      if (!h) { set_error("BA: out of pinned host memory"); return MCS_ERR_HIP; }
      int32_t* dk = (int32_t*)c->alloc(std::max<size_t>(1, keep.size()) * 4);
      int32_t* dc = (int32_t*)c->alloc(culled.size() * 4);
      if (!dk || !dc) { set_error("BA: out of device memory"); return MCS_ERR_HIP; }
      const size_t off_c = ((keep.size() * 4 + 255) & ~(size_t)255);
      std::memcpy(h, keep.data(), keep.size() * 4);
      std::memcpy(h + off_c, culled.data(), culled.size() * 4);
      if (!keep.empty()) MCS_HIP_CHECK(hipMemcpyAsync(dk, h, keep.size() * 4, hipMemcpyHostToDevice, st));
      MCS_HIP_CHECK(hipMemcpyAsync(dc, h + off_c, culled.size() * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_zero_edges, dim3(gb((int)culled.size())), dim3(256), 0, st, d, (const int32_t*)dc,
                         (int)culled.size());
      d.aedge = dk;
      d.nae = (int)keep.size();
    }
    s.aedge.swap(keep);
    nae_glob = d.nae;
    nl_glob = nl_left;
    hc.mark(c->host_ms, 4);
    return MCS_OK;
  }

  // Round 2 of a device-culled LocalBA: round 1's active list with its level-1 edges skipped
  // (no host round trip: the culled edges' terms were zeroed by k_lba_cull)
  void remask_device() {
    d.elevel = lba.L.level;   // round 1's list; its level-1 edges are skipped (terms zeroed)
    nae_glob = lba.res[0];
    nl_glob = lba.res[2];
  }

  // run_device's tail for LocalBA (every LbaTail but Download): chi2 of every edge at the final estimate,
  // the culling pass, and either round 2's counts (round 1: nothing is downloaded; the host
  // reads three counts) or the results (round 2: poses, points, inlier flags, write-back)
  int lba_finish(double* poses, double* points) {
    HostClock hc;
    const LbaState& L = lba.L;
    const bool round1 = lba.tail == LbaTail::Round1;
    if (lba.tail != LbaTail::Round2NoCull) {
      if (int rc = chi2_all_edges()) return rc;
      hipLaunchKernelGGL(k_lba_cull, dim3(gb(s.nl)), dim3(256), 0, st, d, L, round1 ? 1 : 0);
    }
    if (round1) {
      hipLaunchKernelGGL(k_lba_count, dim3(gb(s.nl)), dim3(256), 0, st, d, L);
      MCS_HIP_CHECK(spin_sync(st));
      std::memcpy(lba.res, c->pinned_i, 12);
      hc.mark(c->host_ms, 3);
      MCS_HIP_CHECK(hipGetLastError());
      return MCS_OK;
    }
    const size_t b_po = 48 * (size_t)p->n_poses, b_pt = 24 * (size_t)p->n_points;
    const size_t b_in = (size_t)NE, b_pw = lba.pwrite_out ? (size_t)p->n_points : 0;
    const size_t total = b_po + b_pt + b_in + b_pw + 64;
    if (total > c->stage.cap) MCS_HIP_CHECK(hipStreamSynchronize(st));   // regrow
    uint8_t* hst = c->stage.get(total);
    if (!hst) { set_error("BA: out of pinned host memory"); return MCS_ERR_HIP; }
    // one kernel writes the four results into the pinned staging buffer (host memory the device
    // reaches directly): no readback copies
    const int nmax = (int)std::max<size_t>({b_po / 8 + b_pt / 8, b_in, b_pw, 1});
    hipLaunchKernelGGL(k_lba_out, dim3(gb(nmax)), dim3(256), 0, st, (const double*)d_poses,
                       (int)(b_po / 8), (const double*)d_points, (int)(b_pt / 8), (const uint8_t*)L.inlier,
                       (int)b_in, (const uint8_t*)L.pwrite, (int)b_pw, hst);
    MCS_HIP_CHECK(spin_sync(st));
    if (b_po) std::memcpy(poses, hst, b_po);
    if (b_pt) std::memcpy(points, hst + b_po, b_pt);
    if (b_in && lba.inlier_out) std::memcpy(lba.inlier_out, hst + b_po + b_pt, b_in);
    if (b_pw) std::memcpy(lba.pwrite_out, hst + b_po + b_pt + b_in, b_pw);
    hc.mark(c->host_ms, 3);
    MCS_HIP_CHECK(hipGetLastError());
    return MCS_OK;
  }

  // the round-1 state a host fallback needs (a pose left the system): the estimate, the levels
  // and the per-point culling state
  int lba_fetch(double* poses, double* points, uint8_t* level, uint8_t* inlier, int32_t* obs_left,
                int32_t* edges_left, uint8_t* bad) {
    const LbaState& L = lba.L;
    const size_t npt = (size_t)p->n_points;
    MCS_HIP_CHECK(hipMemcpyAsync(poses, d_poses, 48 * (size_t)p->n_poses, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(points, d_points, 24 * npt, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(level, L.level, (size_t)NE, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(inlier, L.inlier, (size_t)NE, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(obs_left, L.obs_left, 4 * npt, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(edges_left, L.edges_left, 4 * npt, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(bad, L.bad, npt, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipStreamSynchronize(st));
    return MCS_OK;
  }

  // poses and points only (round 1 stopped by the caller's flag)
  int fetch_state(double* poses, double* points) {
    MCS_HIP_CHECK(hipMemcpyAsync(poses, d_poses, 48 * (size_t)p->n_poses, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipMemcpyAsync(points, d_points, 24 * (size_t)p->n_points, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(hipStreamSynchronize(st));
    return MCS_OK;
  }

  // the host-driven loop learns a trial's outcome from k_reduce3's released sequence numbers
  // (one launch for the three sums) instead of a readback copy and a stream synchronisation
  bool sig_path() const { return !sharded && d.nae <= 32768 && s.nl <= 32768 && s.np <= 32768; }

  // the report of a finished run from its control block (run: its own; run_device: the copy
  // k_edges_end left in pinned memory); stop = the stop flag afterwards
  void write_report(mcs_ba_report* rep, const LmCtl& k, int32_t stop) const {
    if (!rep) return;
    rep->n_active_edges = nae_glob;
    rep->n_active_poses = s.np;
    rep->n_active_points = nl_glob;
    rep->chi2_initial = k.chi0;
    rep->chi2_final = k.currentChi;
    rep->iterations = k.it;
    rep->lambda_final = k.lambda_final;
    rep->stop_flag = stop;
  }

  // the LM loop runs on the device (run_device) for these options
  bool device_driven(const mcs_ba_options* o, const mcs_ba_report* rep) const {
    const bool long_trace = rep && rep->trace_chi2 && rep->trace_cap > kLmTraceCap &&
                            o->max_iterations > kLmTraceCap;
    return !sharded && !c->timing && !long_trace;
  }

  int run(const mcs_ba_options* o, double* poses, double* points, double* edge_chi2,
          volatile int32_t* stop_flag, mcs_ba_report* rep) {
    // one GPU and no per-stage timing: the LM control runs on the device (no per-trial
    // host round trip); sharded runs agree on every decision through the host exchange
    // (the device loop records the chi2 trace of its first kLmTraceCap iterations only: a
    // caller asking for a longer trace of a longer run gets the host-driven loop, which fills
    // up to trace_cap like every other path)
    if (device_driven(o, rep))
      return run_device(o, poses, points, edge_chi2, stop_flag, rep);
    auto rec = [&](int k) { if (c->timing) (void)hipEventRecord(c->ev[k], st); };
    auto ms = [&](int a, int b) { float f = 0.f; (void)hipEventElapsedTime(&f, c->ev[a], c->ev[b]); return (double)f; };
    int rc;
    // control state agreed by all ranks: the caller's stop flag is folded into every scalar
    // exchange, so no rank leaves the LM loop alone
    volatile int32_t aux = 0;
    volatile int32_t* stop = stop_flag ? stop_flag : &aux;
    int agreed_stop = 0;
    const size_t sc = X.sc;

    auto chi_now = [&](double* out) -> int {   // robust chi2 of the current estimate (all ranks)
      hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, d, 0);
      reduce_dev<false>(d.rchi, d.nae, d_scalar, d_part, st);
      MCS_HIP_CHECK(hipMemcpyAsync(c->pinned + 3, d_scalar, 8, hipMemcpyDeviceToHost, st));
      MCS_HIP_CHECK(hipStreamSynchronize(st));
      double v[2] = {c->pinned[3], (double)(*stop != 0)};
      int r = allreduce_host(v, 2, MCS_REDUCE_SUM, sc);
      if (r) return r;
      *out = v[0];
      agreed_stop = v[1] > 0;
      return MCS_OK;
    };
    // one LM trial (push, Schur, solve, update, chi2), enqueued on st; lambda in d (by value)
    auto enqueue_trial = [&](bool stop_now) -> int {
      int rc2;
      rec(2);
      // also pushes the state (poses / points -> backups) and resets the solve flag
      hipLaunchKernelGGL(k_point_trial, dim3(std::max(gb(d.npe), g_state)), dim3(256), 0, st, d);
      if (s.np) {
        hipLaunchKernelGGL(k_schur, dim3((unsigned)((items_max + 3) / 4)), dim3(256), 0, st, d);
        hipLaunchKernelGGL(k_schur_fin, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, st, d, nblk);
        // one tile (LocalBA): the padding is applied inside the fused solve, after the exchange
        if (T > 1) MCS_HIP_CHECK(ldlt::pad(d.S, d.bs, n, T, sh.rank == 0 ? 1.0 : 0.0, st));
        rec(3);
        if ((rc2 = allreduce(MCS_REDUCE_SUM, X.bs, xs_count))) return rc2;   // bs | S band
        rec(4);
        if (T == 1) MCS_HIP_CHECK(ldlt::solve_one_tile(d.S, d.bs, d.xp, n, 1.0, d_flag, st));
        else MCS_HIP_CHECK(ldlt::solve(d.S, d.bs, d.xp, T, lw, d_flag, st));
      } else {
        rec(3); rec(4);
      }
      rec(5);
      hipLaunchKernelGGL(k_update, dim3(gb(4 * s.nl + s.np)), dim3(256), 0, st, d);
      hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, d, 0);
      if (sig_path()) {
        Sum3 q{{d.rchi, d.red, d.red + s.nl}, {d.nae, s.nl, s.np}};
        hipLaunchKernelGGL(k_reduce3, dim3(3), dim3(1024), 0, st, q, (const int*)d_flag, c->sig, ++c->sig_seq);
      } else if (sharded) {
        // chi2 and the points' model decrease are partial sums: reduce them straight into the
        // exchange buffer next to the stop flag, all-reduce them there and read back once
        // (pinned[0..2] = the summed {chi2, points' decrease, stop}; pinned[3] = the poses'
        // decrease, replicated; pinned[5] = the solve flag, identical on every rank)
        reduce_dev<false>(d.rchi, d.nae, sh.xchg + X.sc, d_part, st);
        reduce_dev<false>(d.red, s.nl, sh.xchg + X.sc + 1, d_part, st);
        reduce_dev<false>(d.red + s.nl, s.np, d_scalar + 2, d_part, st);
        c->pinned[7] = stop_now ? 1.0 : 0.0;
        MCS_HIP_CHECK(hipMemcpyAsync(sh.xchg + X.sc + 2, c->pinned + 7, 8, hipMemcpyHostToDevice, st));
        if ((rc2 = allreduce(MCS_REDUCE_SUM, X.sc, 3))) return rc2;
        MCS_HIP_CHECK(hipMemcpyAsync(c->pinned, sh.xchg + X.sc, 24, hipMemcpyDeviceToHost, st));
        MCS_HIP_CHECK(hipMemcpyAsync(c->pinned + 3, d_scalar + 2, 8, hipMemcpyDeviceToHost, st));
        MCS_HIP_CHECK(hipMemcpyAsync(c->pinned + 5, d_scalar + 5, 8, hipMemcpyDeviceToHost, st));
      } else {
        reduce_dev<false>(d.red, s.nl, d_scalar + 1, d_part, st);
        reduce_dev<false>(d.red + s.nl, s.np, d_scalar + 2, d_part, st);
        reduce_dev<false>(d.rchi, d.nae, d_scalar, d_part, st);
        MCS_HIP_CHECK(hipMemcpyAsync(c->pinned, d_scalar, 48, hipMemcpyDeviceToHost, st));
      }
      rec(6);
      return MCS_OK;
    };
    // wait for the trial's outcome: spin on the released sequence number (sig_path), checking
    // the stream now and then so a failed launch cannot spin forever; else synchronise the
    // stream after the readback copy.  Fills pinned[0..2] and the solve flag.
    auto wait_trial = [&](int* fl) -> int {
      if (!sig_path()) {
        MCS_HIP_CHECK(hipStreamSynchronize(st));
        std::memcpy(fl, c->pinned + 5, sizeof(*fl));
        return MCS_OK;
      }
      const uint64_t want = c->sig_seq;
      auto arrived = [&]() {
        return __atomic_load_n(&c->sig->seq[0], __ATOMIC_ACQUIRE) == want &&
               __atomic_load_n(&c->sig->seq[1], __ATOMIC_ACQUIRE) == want &&
               __atomic_load_n(&c->sig->seq[2], __ATOMIC_ACQUIRE) == want;
      };
      if (int r = spin_until(st, arrived, [] {}, "BA: trial signal missing after the stream drained", "BA trial"))
        return r;
      c->pinned[0] = c->sig->v[0]; c->pinned[1] = c->sig->v[1]; c->pinned[2] = c->sig->v[2];
      *fl = c->sig->flag;
      if (c->timing) MCS_HIP_CHECK(hipStreamSynchronize(st));   // events complete
      return MCS_OK;
    };
    // the same controller as the device-driven loop (lm_control.hpp), driven from the host:
    // every rank feeds it the same agreed sums, solve flag and stop flag
    LmCtl ctl;
    lm_init(ctl, *o);
    if ((s.np + nl_glob) == 0 || nae_glob == 0) {
      ctl.done = 1;
    } else {
      double chi0 = 0;
      if ((rc = chi_now(&chi0))) return rc;
      lm_start_body(&ctl, chi0);
      ctl.done = (o->max_iterations <= 0 || agreed_stop) ? 1 : 0;
    }
    bool lin_pending = false;
    while (!ctl.done) {
      if (ctl.lin) {
        // ---- OptimizationAlgorithmLevenberg::solve(i)
        // The robust chi2 of the linearisation point equals the chi2 the previous iteration
        // ended with (same kernel, same state: accepted trial or restored backup), so only
        // the first iteration reads anything back (the max diagonal for lambda's init).
        rec(0);
        hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, d, 1);
        hipLaunchKernelGGL(k_build, dim3((unsigned)s.np + (unsigned)((4 * s.nl + kBuildNT - 1) / kBuildNT)), dim3(kBuildNT), 0, st, d);
        rec(1);
        c->n_iter++;
        lin_pending = c->timing;
        if ((rc = allreduce(MCS_REDUCE_SUM, X.hdiag, 12 * (size_t)s.np))) return rc;   // hdiag | bpf
        if (ctl.iter == 0) {
          reduce_dev<true>(d.red, s.nl, d_scalar + 1, d_part, st);
          reduce_dev<true>(d.hdiag, 6 * s.np, d_scalar + 2, d_part, st);
          MCS_HIP_CHECK(hipMemcpyAsync(c->pinned + 1, d_scalar + 1, 16, hipMemcpyDeviceToHost, st));
          MCS_HIP_CHECK(hipStreamSynchronize(st));
          double mx = std::max(c->pinned[1], c->pinned[2]);
          if ((rc = allreduce_host(&mx, 1, MCS_REDUCE_MAX, sc))) return rc;
          lm_lambda0_body(&ctl, mx, mx);
        }
      }
      // lambda reaches the kernels by value (Dev d), no upload; a captured graph of the trial
      // (replayed per trial) measured no faster than these direct launches
      d.lam = ctl.lambda;
      d.lam0 = sh.rank == 0 ? ctl.lambda : 0.0;
      if ((rc = enqueue_trial(*stop != 0))) return rc;
      int fl;   // identical on every rank (same reduced system)
      if ((rc = wait_trial(&fl))) return rc;
      // sharded: chi2, the points' decrease and the stop flag summed on the device by enqueue_trial
      const double tr[3] = {c->pinned[0], c->pinned[1], sharded ? c->pinned[3] : c->pinned[2]};
      agreed_stop = sharded ? c->pinned[2] > 0 : *stop != 0;
      const int i = ctl.iter;
      lm_step(&ctl, tr, (fl & ldlt::kFlagZeroPivot) != 0, (fl & ldlt::kFlagTimeout) != 0, agreed_stop);
      if (ctl.dev_err) {
        set_error("BA: the LDL^T solve's hand-off wait timed out (ldlt kFlagTimeout); result discarded");
        return MCS_ERR_HIP;
      }
      if (c->timing) {
        if (lin_pending) { c->acc_ms[0] += ms(0, 1); lin_pending = false; }
        if (sh.ordered) c->acc_ms[2] += ms(3, 4);
        c->acc_ms[1] += ms(2, 3);
        c->acc_ms[3] += ms(4, 5);
        c->acc_ms[4] += ms(5, 6);
        c->n_trial++;
        c->last_n = n;
      }
      if (ctl.restore) hipLaunchKernelGGL(k_restore, dim3(g_state), dim3(256), 0, st, d);  // pop
      // an iteration ended: this path's trace is not bounded by kLmTraceCap
      if (ctl.iter != i && rep && rep->trace_chi2 && i < rep->trace_cap) rep->trace_chi2[i] = ctl.currentChi;
      if (ctl.stop_out) *stop = 1;   // the terminate action raised the flag
    }
    write_report(rep, ctl, *stop);
    return download(poses, points, edge_chi2);
  }

  // chi2 of every edge (active or not) at the current estimate -> d.chi; a private view: d
  // keeps its active list for a later remask() + run()
  int chi2_all_edges() {
    Dev d2 = d;
    d2.ctl = nullptr;
    d2.aedge = nullptr;
    d2.elevel = nullptr;
    d2.nae = NE;
    d2.err = dz(2 * (size_t)NE);
    d2.rchi = dz(NE);
    if (he != hipSuccess) { set_hip_error(he, "BA chi2", __FILE__, __LINE__); return MCS_ERR_HIP; }
    hipLaunchKernelGGL(k_edges, dim3(gb(NE)), dim3(256), 0, st, d2, 0);
    return MCS_OK;
  }

  // results through the pinned staging buffer (free again: the stream has been drained since
  // the upload), then one host copy each; edge_chi2 (nullable): chi2 of every edge
  int download(double* poses, double* points, double* edge_chi2) {
    HostClock hc;
    if (edge_chi2)
      if (int rc = chi2_all_edges()) return rc;
    const size_t b_po = 48 * (size_t)p->n_poses, b_pt = 24 * (size_t)p->n_points;
    const size_t b_ch = edge_chi2 ? 8 * (size_t)NE : 0;
    if (b_po + b_pt + b_ch + 64 > c->stage.cap) MCS_HIP_CHECK(hipStreamSynchronize(st));   // regrow
    uint8_t* hst = c->stage.get(b_po + b_pt + b_ch + 64);
    if (!hst) { set_error("BA: out of pinned host memory"); return MCS_ERR_HIP; }
    if (b_po) MCS_HIP_CHECK(hipMemcpyAsync(hst, d_poses, b_po, hipMemcpyDeviceToHost, st));
    if (b_pt) MCS_HIP_CHECK(hipMemcpyAsync(hst + b_po, d_points, b_pt, hipMemcpyDeviceToHost, st));
    if (b_ch) MCS_HIP_CHECK(hipMemcpyAsync(hst + b_po + b_pt, d.chi, b_ch, hipMemcpyDeviceToHost, st));
    MCS_HIP_CHECK(spin_sync(st));
    if (b_po) std::memcpy(poses, hst, b_po);
    if (b_pt) std::memcpy(points, hst + b_po, b_pt);
    if (b_ch) std::memcpy(edge_chi2, hst + b_po + b_pt, b_ch);
    hc.mark(c->host_ms, 3);
    MCS_HIP_CHECK(hipGetLastError());
    return MCS_OK;
  }

  // Device-driven SparseOptimizer::optimize: the host enqueues LM steps (restore if the last
  // trial was rejected, linearisation if it ended an iteration, one trial, k_edges_end) up to two
  // ahead of the device and watches the progress word only to stop enqueuing; the decisions
  // are k_edges_end's.  Kernels of steps past the end return at once.
  int run_device(const mcs_ba_options* o, double* poses, double* points, double* edge_chi2,
                 volatile int32_t* stop_flag, mcs_ba_report* rep) {
    volatile int32_t aux = 0;
    volatile int32_t* stop = stop_flag ? stop_flag : &aux;
    LmCtl* dctl = (LmCtl*)c->alloc(sizeof(LmCtl));
    if (!dctl) { set_error("BA: out of device memory"); return MCS_ERR_HIP; }
    LmCtl h0;
    lm_init(h0, *o);
    h0.spec_lin = d.alt_err ? 1 : 0;   // k_edges_end linearises every trial (see k_edges_end)
    const bool empty = (s.np + nl_glob) == 0 || nae_glob == 0;
    h0.done = (empty || o->max_iterations <= 0 || *stop != 0) ? 1 : 0;
    c->lsig->ext_stop = *stop != 0;
    c->lsig->done = 0;   // this run's `done` (the previous run's stream has drained)
    Dev dd = d;
    dd.ctl = dctl;
    // one-tile systems (LocalBA): k_schur adds a split block's chunk slots itself (fused fin)
    // (multi-tile systems keep the k_schur_fin launch: fused, config E measured 7.07 against
    // 6.90 ms per GlobalBA call)
    const bool fuse = T == 1;
    dd.blk_arrive = (fuse && nblk > 0) ? (uint32_t*)c->alloc(4 * (size_t)nblk) : nullptr;
    hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(256), 0, st, h0, dctl, dd.blk_arrive, nblk);
    const int* skip = &dctl->done;
    const unsigned g_upd = gb(4 * s.nl + s.np), g_edg = gb(d.nae);
    dd.part_chi = dz(g_edg);
    dd.part_pt = dz(g_upd);
    dd.part_ps = dz(g_upd);
    if (he != hipSuccess) { set_hip_error(he, "BA partials", __FILE__, __LINE__); return MCS_ERR_HIP; }
    // the starting point's chi2 (activeRobustChi2 before the first iteration): from step 0's
    // linearising pass when the loop will run (the same errors), else a plain evaluation
    const bool lin0 = !empty && !h0.done;
    if (!empty) {
      if (lin0) {
        hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, dd, 1);
      } else {
        Dev d0 = d;
        hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, d0, 0);
      }
      reduce_dev<false>(d.rchi, d.nae, d_scalar, d_part, st);
      hipLaunchKernelGGL(k_lm_start, dim3(1), dim3(64), 0, st, dctl, (const double*)d_scalar);
    }
    auto enqueue_step = [&](int step) -> int {
      // the first step linearises at the start; later steps find the accepted trial's
      // linearisation (k_edges_end) already in place, or keep the iteration's after a reject
      if ((step == 0 && !lin0) || (step > 0 && !h0.spec_lin))
        hipLaunchKernelGGL(k_edges, dim3(gb(d.nae)), dim3(256), 0, st, dd, 1);
      const unsigned g_build = (unsigned)s.np + (unsigned)((4 * s.nl + kBuildNT - 1) / kBuildNT);
      if (step == 0) {   // iteration 0 is always step 0: lambda from the max diagonal
        hipLaunchKernelGGL(k_build, dim3(g_build), dim3(kBuildNT), 0, st, dd);
        reduce_dev<true>(d.red, s.nl, d_scalar + 1, d_part, st);
        reduce_dev<true>(d.hdiag, 6 * s.np, d_scalar + 2, d_part, st);
        hipLaunchKernelGGL(k_lm_lambda0, dim3(1), dim3(64), 0, st, dctl, (const double*)d_scalar);
        hipLaunchKernelGGL(k_point_trial, dim3(std::max(gb(d.npe), g_state)), dim3(256), 0, st, dd);
      } else {
        hipLaunchKernelGGL(k_build_trial, dim3(g_build), dim3(kBuildNT), 0, st, dd);
      }
      if (s.np) {
        hipLaunchKernelGGL(k_schur, dim3((unsigned)((items_max + 3) / 4)), dim3(256), 0, st, dd);
        if (!dd.blk_arrive)
          hipLaunchKernelGGL(k_schur_fin, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, st, dd, nblk);
        if (T == 1) MCS_HIP_CHECK(ldlt::solve_one_tile(d.S, d.bs, d.xp, n, 1.0, d_flag, st, skip));
        else {
          MCS_HIP_CHECK(ldlt::pad(d.S, d.bs, n, T, 1.0, st, skip));
          MCS_HIP_CHECK(ldlt::solve(d.S, d.bs, d.xp, T, lw, d_flag, st, skip));
        }
      }
      LmEnd le{d_scalar, (const int*)d_flag, c->lsig, ++c->lsig_seq, (LmCtl*)c->pinned_ctl};
      hipLaunchKernelGGL(k_update, dim3(gb(4 * s.nl + s.np)), dim3(256), 0, st, dd);
      // the trial's evaluation, then (last workgroup) its three sums from the workgroup
      // partials of k_edges_end / k_update (a fixed order: partials in workgroup order, each a
      // fixed in-workgroup tree), the LM decision and the pop of a rejected trial
      Sum3 q{{dd.part_chi, dd.part_pt, dd.part_ps}, {(int)g_edg, (int)g_upd, (int)g_upd}};
      hipLaunchKernelGGL(k_edges_end, dim3(g_edg), dim3(kEdgeEndNT), 0, st, dd, q, le);
      return hipGetLastError() == hipSuccess ? MCS_OK : MCS_ERR_HIP;
    };
    // progress word of the step whose k_edges_end published sequence `want`
    auto wait_seq = [&](uint64_t want) -> int {
      return spin_until(
          st, [&] { return __atomic_load_n(&c->lsig->seq, __ATOMIC_ACQUIRE) >= want; },
          [&] { c->lsig->ext_stop = *stop != 0; },   // the caller's abort flag reaches k_edges_end
          "BA: LM progress word missing after the stream drained", "BA LM step");
    };
    int rc;
    if (!h0.done) {
      const uint64_t base = c->lsig_seq;
      const int max_steps = o->max_iterations * std::max(1, o->max_trials);
      for (int step = 0; step < max_steps; step++) {
        if (step >= MCS_LM_AHEAD) {   // keep MCS_LM_AHEAD steps in flight
          if ((rc = wait_seq(base + (uint64_t)step - (MCS_LM_AHEAD - 1)))) return rc;
          c->lsig->ext_stop = *stop != 0;
          if (c->lsig->done) break;
        }
        if ((rc = enqueue_step(step))) { set_error("BA: LM step launch failed"); return rc; }
      }
    }
    LmCtl* hc = (LmCtl*)c->pinned_ctl;
    // the step that ended the run wrote the control block to hc (k_edges_end); otherwise (no
    // step ran, or the host stopped at max_steps before seeing `done`) read it back
    const bool ctl_written = !h0.done && __atomic_load_n(&c->lsig->done, __ATOMIC_ACQUIRE) != 0;
    if (!ctl_written) MCS_HIP_CHECK(hipMemcpyAsync(hc, dctl, sizeof(LmCtl), hipMemcpyDeviceToHost, st));
    // per-edge chi2 of every edge at the final estimate, poses, points: the common tail (or
    // LocalBA's device culling)
    const int rtail = lba.tail != LbaTail::Download ? lba_finish(poses, points) : download(poses, points, edge_chi2);
    if (rtail) return rtail;
    if (hc->dev_err) {
      set_error("BA: the LDL^T solve's hand-off wait timed out (ldlt kFlagTimeout); optimisation aborted");
      return MCS_ERR_HIP;
    }
    if (hc->stop_out) *stop = 1;   // the terminate action raised the flag (host-visible)
    write_report(rep, *hc, *stop);   // (an empty graph never ran k_lm_start: chi0 = currentChi = 0)
    if (rep && rep->trace_chi2)
      for (int i = 0; i < std::min(hc->iter, std::min(rep->trace_cap, kLmTraceCap)); i++)
        rep->trace_chi2[i] = hc->trace[i];
    return MCS_OK;
  }
};

int optimize_impl(mcs_ba_ctx* c, const mcs_ba_problem* p, const mcs_ba_options* o, double* poses,
                  double* points, const uint8_t* edge_level, double* edge_chi2,
                  volatile int32_t* stop_flag, mcs_ba_report* rep, const mcs_ba_shard* shard_in,
                  bool points_fixed) {
  if (!c || !p || !o || !poses || !points) return MCS_ERR_ARG;
  Optimizer opt(c, p, points_fixed);
  int rc = opt.setup(poses, points, edge_level, shard_in);
  if (rc) return rc;
  return opt.run(o, poses, points, edge_chi2, stop_flag, rep);
}

}  // namespace
