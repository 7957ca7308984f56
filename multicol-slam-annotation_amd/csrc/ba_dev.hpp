// Device-side state of one BA call: the argument block every kernel takes (Dev), the
// host-coherent progress words of the two LM loops, LocalBA's culling state and the workgroup
// sizes the kernels and their launches share.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lm_control.hpp"

namespace mcs::ba {
// host-coherent progress word of run_device (written by k_edges_end after every step)
struct LmSig { uint64_t seq; int32_t done, iter; int32_t ext_stop, pad_; };

struct Dev {
  LmCtl* ctl;   // device-driven LM (null: host-driven, lambda by value below)
  // device-driven trial sums: per-workgroup partials of the robust chi2 (k_edges), of the
  // points' and the poses' model decrease (k_update); null = the per-element arrays only
  double* part_chi; double* part_pt; double* part_ps;
  // problem
  const double* mc; const double* cam;
  const int32_t* e_pose; const int32_t* e_point; const int32_t* e_cam;
  const double* e_meas; const double* e_info;
  double delta, dsqr;
  // state
  double* poses; double* points; const double* poses_bk; const double* points_bk;
  // active structure
  const int32_t* aedge; int nae;
  const uint8_t* elevel;   // per edge: 1 = level 1 (LocalBA round 2 keeps round 1's list), null = none
  const int32_t* pose_h; const int32_t* point_h;      // hessian index per vertex (-1 inactive)
  const int32_t* hpose_vtx; const int32_t* hpt_vtx;   // vertex id per hessian index
  int np, nl;
  const int32_t* pt_ptr; const int32_t* pt_edges;     // CSR active points -> active edges
  const int32_t* pt_h;                                // pose Hessian index per pt_edges entry
  const int32_t* ps_ptr; const int32_t* ps_edges;     // CSR active poses  -> active edges
  const int32_t* blk_i; const int32_t* blk_j;         // lower pose blocks (i >= j)
  const int32_t* it_blk; const int32_t* it_chunk; const int32_t* it_slot;  // k_schur items
  const int32_t* blk_nch; const int32_t* blk_slot0;  // chunks / first partial slot per block
  double* schur_part;                                 // [slots][42]
  uint32_t* blk_arrive;                               // per block: chunks arrived (fused fin; null: k_schur_fin)
  double lam, lam0;                                   // lambda; lambda on rank 0, 0 elsewhere
  const int32_t* pr_ptr; const uint2* pr;             // edge pairs (e1, e2) per block
  const int32_t* nitem;                               // k_schur items (device-built count)
  int npe;                                            // entries of pt_edges
  // per-edge buffers (indexed by edge id)
  double* err; double* w; double* jp; double* jl; double* hpl; double* y; double* chi; double* rchi;
  // the second linearisation buffer of a device-driven run (null: one buffer): k_edges_end
  // linearises each trial there, and an accepted trial makes it the iteration's (ctl->jbuf)
  double* alt_err; double* alt_w; double* alt_jp; double* alt_jl; double* alt_hpl;
  // system
  double* Hpp; double* bp; double* Hll; double* bl; double* Dinv; double* db;
  double* S; double* bs; double* xp;   // S: lower 64x64 tiles (ldlt.hpp), bs / xp: 64 T
  int T;                               // tiles per side of S
  double* hdiag; double* bpf;          // [6 np] Hpp diagonal and b_p (all-reduced when sharded)
  double* red;                         // reduction scratch
  // trial bookkeeping folded into k_point_trial (each was a 4-5 us copy / fill launch)
  double* push_poses; double* push_points;  // backups (== poses_bk / points_bk)
  int n_pose_dbl, n_point_dbl;              // 6 n_poses, 3 n_points
  int* flag;                                // solve failure flag
};

__device__ __forceinline__ double lam_of(const Dev& d) { return d.ctl ? d.ctl->lambda : d.lam; }
// the linearisation buffer a kernel of a device-driven step reads (spec: the one a trial
// linearises into); host-driven runs have one buffer
__device__ __forceinline__ Dev lin_buf(const Dev& d, bool spec) {
  Dev r = d;
  if (d.ctl && d.alt_err && ((d.ctl->jbuf ^ (spec ? 1 : 0)) & 1)) {
    r.err = d.alt_err; r.w = d.alt_w; r.jp = d.alt_jp; r.jl = d.alt_jl; r.hpl = d.alt_hpl;
  }
  return r;
}
__device__ __forceinline__ double lam0_of(const Dev& d) { return d.ctl ? d.ctl->lambda : d.lam0; }
// a kernel of a device-driven step that is not needed (the loop has ended)
__device__ __forceinline__ bool lm_done(const Dev& d) { return d.ctl && d.ctl->done; }

constexpr int kRedNT = 256;   // reduction workgroup (k_edges_end's LM tail, k_update partials)
#ifndef MCS_BUILD_NT
#define MCS_BUILD_NT 256
#endif
// k_build / k_build_trial workgroup (1024 measured slower: 18.3 vs 12.9 us at config C)
constexpr int kBuildNT = MCS_BUILD_NT;
constexpr int kEdgeEndNT = 512;   // k_edges_end: 256 edges, error and Jacobian waves side by side

// the three closing sums of an LM trial and where their outcome goes (k_reduce3, k_edges_end)
struct Sum3 { const double* v[3]; int n[3]; };
struct TrialSig { double v[3]; int32_t flag, pad; uint64_t seq[3]; };
struct LmEnd { double* sc; const int* flag; LmSig* sig; uint64_t seq; LmCtl* host_ctl; };
#ifndef MCS_LM_AHEAD
#define MCS_LM_AHEAD 2      // LM steps the host keeps enqueued ahead of the device
#endif

// LocalBA's culling state on the device (k_lba_*, ba_lba.hpp)
struct LbaState {
  int32_t* obs_left; int32_t* edges_left; int32_t* edges_all;   // per point vertex
  uint8_t* bad;                                                  // per point vertex
  uint8_t* inlier; uint8_t* level;                               // per edge
  const int32_t* extra;                                          // extra observations (nullable)
  double* chi;                                                   // chi2 of every edge
  double k2;                                                     // thHuber^2
  int32_t* pose_cnt;                                             // active edges per active pose
  uint32_t* ctr;                                                 // {culled edges, points left, arrivals}
  int32_t* res;                                                  // {nae, pose_left, nl_left} (host memory)
  uint8_t* pwrite;                                               // per point vertex (round 2)
};

}  // namespace mcs::ba
