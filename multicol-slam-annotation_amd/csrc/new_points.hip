// CreateNewMapPoints on the device (include/mcs_newpoints.h): the per-match loop of local mapping
// for one (current keyframe KF1, neighbour KF2) pair, and the neighbour loop that chains the
// triangulation search and this loop on one stream.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cLocalMapping::CreateNewMapPoints                    src/cLocalMapping.cpp:224-386
//   triangulate_point                                    src/misc.cpp:26-51
//   cMultiCamSys_::WorldToCamHom_fast                    src/cam_system_omni.cpp:92-112
//   cMultiCamSys_::Set_M_t (MtMc, MtMc_inv)              src/cam_system_omni.cpp:170-183
//   cCamModelGeneral_::WorldToImg                        src/cam_model_omni.cpp:147-163
//   cConverter::invMat                                   src/cConverter.cpp:31-44
//   the order of vMatchedPairs                           src/cORBmatcher.cpp:1140-1152
//   cMapPoint::ComputeDistinctiveDescriptors (N = 2)     src/cMapPoint.cpp:297-390
//   cMapPoint::UpdateNormalAndDepth                      src/cMapPoint.cpp:453-496
// Two launches per neighbour.  k_np_verdict: every block builds the camera-pair table in LDS
// (Get_MtMc, its invMat and relOri = Tcw1inv * Tcw2 for every (c1, c2)), then one thread per KF1
// keypoint runs :277-364 and leaves a verdict, the point and the block's number of survivors.
// k_np_admit: the survivors' output rows in idx1 order (ballot prefix in the wave, wave totals in
// the block, the totals of the earlier blocks) and the admit step (:365-377).  Compiled with
// -ffp-contract=off; cv::Matx products accumulate s = 0; s += a_k * b_k, k ascending.  M_t * M_c, its
// invMat and WorldToImg are frm:: of omni_geom.hpp; the rows on a homogeneous (X, w) stay here.
#include "host_util.hpp"
#include "mappoint_math.hpp"
#include "omni_geom.hpp"
#include "../../include/mcs_newpoints.h"
#include <climits>
#include <cmath>
#include <initializer_list>
#include <vector>

namespace mcs {
namespace npt {

constexpr int kMaxCams = 8;
constexpr int kBlock = 256;
constexpr int kCam = 24;           // doubles per (keyframe, camera): Tcw R 9, t 3, Tcw^-1 R 9, t 3
constexpr int kRel = 12;           // doubles per camera pair: R12 9, t12 3
constexpr double kMaxDist = 25.0;  // maxDIST (src/cLocalMapping.cpp:43)
constexpr double kMaxErr = 4.0;    // :332, :346

struct Kf {
  int n_targets, n_kp_total, C, bytes, L;
  const int32_t* off; const float* kp_xy; const int32_t* kp_oct; const int32_t* kp_cam;
  const uint8_t* desc; const uint8_t* mask; const double* rays;
  const double* m_t; const double* m_c; const double* cam; const double* scale;
};

struct Out {
  int cap;
  int32_t* count; int32_t* kp1; int32_t* kp2; int32_t* nb;
  double* pos; double* normal; double* dmin; double* dmax;
  uint8_t* desc; uint8_t* mask;
};

// Vec3d::dot / a row of a Matx33d * Vec3d product: s = 0; s += a_k * b_k
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  double s = 0.0;
  s = __dadd_rn(s, __dmul_rn(a0, b0));
  s = __dadd_rn(s, __dmul_rn(a1, b1));
  s = __dadd_rn(s, __dmul_rn(a2, b2));
  return s;
}

// a row of a Matx44d * Vec4d product
__device__ __forceinline__ double dot4(double a0, double a1, double a2, double a3, double b0, double b1,
                                       double b2, double b3) {
  return __dadd_rn(dot3(a0, a1, a2, b0, b1, b2), __dmul_rn(a3, b3));
}

// the keypoint range of target t, clamped to the packed arrays
__device__ __forceinline__ void kf_range(const Kf& k, int t, int* o, int* n) {
  *o = min(max(k.off[t], 0), k.n_kp_total);
  *n = min(max(k.off[t + 1] - *o, 0), k.n_kp_total - *o);
}

// The table of one block.  Thread (kf, c): Tcw = M_t * M_c[c] (Get_MtMc) and invMat of it; then
// thread (c1, c2): relOri = Tcw1inv * Tcw2 as the 4 x 4 product (rows 0..2).
__device__ __forceinline__ void build_table(const Kf& k, int i1, int i2, double (*s_cam)[kMaxCams][kCam],
                                            double (*s_rel)[kRel], double* s_ow) {
  const int tid = threadIdx.x, C = k.C;
  if (tid < 2 * C) {
    const int kf = tid / C, c = tid - kf * C;
    double R[9], t[3];
    frm::mtmc44(k.m_t + 16 * (int64_t)(kf ? i2 : i1), k.m_c + 16 * c, R, t);
    double* d = s_cam[kf][c];
#pragma unroll
    for (int j = 0; j < 9; j++) d[j] = R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) d[9 + j] = t[j];
    frm::inv_rt(R, t, d + 12, d + 21);
  } else if (tid >= 64 && tid < 70) {          // GetCameraCenter: the translation of M_t
    const int j = tid - 64, kf = j / 3, r = j - 3 * kf;
    s_ow[j] = k.m_t[16 * (int64_t)(kf ? i2 : i1) + 4 * r + 3];
  }
  __syncthreads();
  if (tid < C * C) {
    const int c1 = tid / C, c2 = tid - c1 * C;
    const double* A = s_cam[0][c1] + 12;       // Tcw1inv
    const double* B = s_cam[1][c2];            // Tcw2
    double* d = s_rel[tid];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++)
        d[3 * i + j] = dot4(A[3 * i], A[3 * i + 1], A[3 * i + 2], A[9 + i], B[j], B[3 + j], B[6 + j], 0.0);
      d[9 + i] = dot4(A[3 * i], A[3 * i + 1], A[3 * i + 2], A[9 + i], B[9], B[10], B[11], 1.0);
    }
  }
  __syncthreads();
}

// WorldToCamHom_fast (src/cam_system_omni.cpp:92-112) with MtMc_inv = Ti (R 9, t 3) on the
// homogeneous point (X, w): false = the text's `zpos` (ptRot(2) <= 0), else the pixel error
// cv::sqrt(ex^2 + ey^2) against the float keypoint widened to double
__device__ __forceinline__ bool reproject(const double* Ti, const double* cam, double X0, double X1, double X2,
                                          double w, float kx, float ky, double* err) {
  const double px = dot4(Ti[0], Ti[1], Ti[2], Ti[9], X0, X1, X2, w);
  const double py = dot4(Ti[3], Ti[4], Ti[5], Ti[10], X0, X1, X2, w);
  const double pz = dot4(Ti[6], Ti[7], Ti[8], Ti[11], X0, X1, X2, w);
  if (pz <= 0.0) return false;
  double u, v;
  frm::world_to_img(cam, px, py, pz, u, v);
  const double ex = __dsub_rn(u, (double)kx), ey = __dsub_rn(v, (double)ky);
  *err = __dsqrt_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)));
  return true;
}

// :287-364 for one match.  T1 / T2: the table rows of (KF1, camIdx1) / (KF2, camIdx2), rel: the
// pair's relOri, ow: Ow1, Ow2.  X = x3D in the world frame (written for every verdict past the
// parallax gate).
__device__ __forceinline__ int verdict(const double* T1, const double* T2, const double* rel,
                                       const double* cam1, const double* cam2, const double* ow,
                                       double a0, double a1, double a2, double b0, double b1, double b2,
                                       float k1x, float k1y, float k2x, float k2y, double cos_thresh,
                                       double* X) {
  // rayRot = Rcw * ray; cosParallax (:299-303)
  const double p0 = dot3(T1[0], T1[1], T1[2], a0, a1, a2), p1 = dot3(T1[3], T1[4], T1[5], a0, a1, a2),
               p2 = dot3(T1[6], T1[7], T1[8], a0, a1, a2);
  const double q0 = dot3(T2[0], T2[1], T2[2], b0, b1, b2), q1 = dot3(T2[3], T2[4], T2[5], b0, b1, b2),
               q2 = dot3(T2[6], T2[7], T2[8], b0, b1, b2);
  const double cosp = __ddiv_rn(dot3(p0, p1, p2, q0, q1, q2),
                                __dmul_rn(mpt::norm3(p0, p1, p2), mpt::norm3(q0, q1, q2)));
  if (cosp < 0.0 || cosp > cos_thresh) return MCS_NP_PARALLAX;     // a NaN passes, as in the text
  // triangulate_point(t12, R12, ray1, ray2) (src/misc.cpp:26-51)
  const double f0 = dot3(rel[0], rel[1], rel[2], b0, b1, b2), f1 = dot3(rel[3], rel[4], rel[5], b0, b1, b2),
               f2 = dot3(rel[6], rel[7], rel[8], b0, b1, b2);
  const double t0 = rel[9], t1 = rel[10], t2 = rel[11];
  const double bb0 = dot3(t0, t1, t2, a0, a1, a2), bb1 = dot3(t0, t1, t2, f0, f1, f2);
  const double A00 = dot3(a0, a1, a2, a0, a1, a2), A10 = dot3(a0, a1, a2, f0, f1, f2);
  const double A01 = -A10, A11 = -dot3(f0, f1, f2, f0, f1, f2);
  // Matx22d::inv(): d = 1 / det, the adjugate times d; a zero matrix when det == 0
  const double det = __dsub_rn(__dmul_rn(A00, A11), __dmul_rn(A01, A10));
  double i00 = 0.0, i01 = 0.0, i10 = 0.0, i11 = 0.0;
  if (det != 0.0) {
    const double d = __ddiv_rn(1.0, det);
    i00 = __dmul_rn(A11, d); i01 = __dmul_rn(-A01, d);
    i10 = __dmul_rn(-A10, d); i11 = __dmul_rn(A00, d);
  }
  const double l0 = __dadd_rn(__dadd_rn(0.0, __dmul_rn(i00, bb0)), __dmul_rn(i01, bb1));
  const double l1 = __dadd_rn(__dadd_rn(0.0, __dmul_rn(i10, bb0)), __dmul_rn(i11, bb1));
  // pt3 = (lambda0 * v1 + (t12 + lambda1 * f2)) / 2.0
  const double c0 = __ddiv_rn(__dadd_rn(__dmul_rn(a0, l0), __dadd_rn(t0, __dmul_rn(f0, l1))), 2.0);
  const double c1 = __ddiv_rn(__dadd_rn(__dmul_rn(a1, l0), __dadd_rn(t1, __dmul_rn(f1, l1))), 2.0);
  const double c2 = __ddiv_rn(__dadd_rn(__dmul_rn(a2, l0), __dadd_rn(t2, __dmul_rn(f2, l1))), 2.0);
  // x3D4 = Tcw1 * (x3D, 1) (:315-317); the fourth row is 0 0 0 1
  const double c[3] = {c0, c1, c2};
  frm::hom_mul(T1, T1 + 9, c, X);
  const double X0 = X[0], X1 = X[1], X2 = X[2];
  const double w = dot4(0.0, 0.0, 0.0, 1.0, c0, c1, c2, 1.0);
  double err;
  if (!reproject(T1 + 12, cam1, X0, X1, X2, w, k1x, k1y, &err)) return MCS_NP_BEHIND1;
  if (err > kMaxErr) return MCS_NP_REPROJ1;
  if (!reproject(T2 + 12, cam2, X0, X1, X2, w, k2x, k2y, &err)) return MCS_NP_BEHIND2;
  if (err > kMaxErr) return MCS_NP_REPROJ2;
  const double d1 = mpt::ref_dist(X0, X1, X2, ow), d2 = mpt::ref_dist(X0, X1, X2, ow + 3);
  if (d1 == 0.0 || d2 == 0.0 || d1 > kMaxDist || d2 > kMaxDist) return MCS_NP_DISTANCE;
  return MCS_NP_CREATED;
}

__global__ __launch_bounds__(kBlock) void k_np_verdict(Kf k, int i1, int i2, int n1,
                                                       const int32_t* __restrict__ matches12, double cos_thresh,
                                                       uint8_t* __restrict__ verd, double* __restrict__ x3d,
                                                       int32_t* __restrict__ bcnt, int32_t* __restrict__ base,
                                                       const int32_t* __restrict__ count) {
  __shared__ double s_cam[2][kMaxCams][kCam];
  __shared__ double s_rel[kMaxCams * kMaxCams][kRel];
  __shared__ double s_ow[6];
  __shared__ int s_w[kBlock / 64];
  build_table(k, i1, i2, s_cam, s_rel, s_ow);
  int o1, n_1, o2, n_2;
  kf_range(k, i1, &o1, &n_1);
  kf_range(k, i2, &o2, &n_2);
  n_1 = min(n_1, n1);
  const int idx1 = blockIdx.x * kBlock + threadIdx.x;
  int code = MCS_NP_NONE;
  if (idx1 < n_1) {
    const int m = matches12[idx1];
    if (m >= 0 && m < n_2) {
      const int64_t g1 = (int64_t)o1 + idx1, g2 = (int64_t)o2 + m;
      const int c1 = k.kp_cam[g1], c2 = k.kp_cam[g2];
      if (c1 >= 0 && c1 < k.C && c2 >= 0 && c2 < k.C) {
        const double* r1 = k.rays + 3 * g1;
        const double* r2 = k.rays + 3 * g2;
        double X[3];
        code = verdict(s_cam[0][c1], s_cam[1][c2], s_rel[c1 * k.C + c2], k.cam + 17 * c1, k.cam + 17 * c2, s_ow,
                       r1[0], r1[1], r1[2], r2[0], r2[1], r2[2], k.kp_xy[2 * g1], k.kp_xy[2 * g1 + 1],
                       k.kp_xy[2 * g2], k.kp_xy[2 * g2 + 1], cos_thresh, X);
        if (code == MCS_NP_CREATED) {
          x3d[3 * (int64_t)idx1] = X[0]; x3d[3 * (int64_t)idx1 + 1] = X[1]; x3d[3 * (int64_t)idx1 + 2] = X[2];
        }
      }
    }
  }
  if (idx1 < n1) verd[idx1] = (uint8_t)code;
  const uint64_t bal = __ballot(code == MCS_NP_CREATED);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) tot += s_w[w];
    bcnt[blockIdx.x] = tot;
    if (blockIdx.x == 0) *base = *count;       // k_np_admit appends from here
  }
}

// The survivors' rows and the admit step.  Block b's first row is *base + the totals of the
// blocks before it; nobody writes *base or bcnt in this launch, and the last block alone writes
// *count, which nobody reads in this launch.
__global__ __launch_bounds__(kBlock) void k_np_admit(Kf k, int i1, int i2, int n1, int neighbour, int kf2_first,
                                                     const int32_t* __restrict__ matches12,
                                                     const uint8_t* __restrict__ verd,
                                                     const double* __restrict__ x3d,
                                                     const int32_t* __restrict__ bcnt,
                                                     const int32_t* __restrict__ base, uint8_t* has1, uint8_t* has2,
                                                     Out o) {
  __shared__ int s_w[kBlock / 64], s_p[kBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int o1, n_1, o2, n_2;
  kf_range(k, i1, &o1, &n_1);
  kf_range(k, i2, &o2, &n_2);
  n_1 = min(n_1, n1);
  int before = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += kBlock) before += bcnt[j];
  before = dev::wave_sum(before);
  const int idx1 = blockIdx.x * kBlock + threadIdx.x;
  const bool keep = idx1 < n_1 && n_2 > 0 && verd[idx1] == MCS_NP_CREATED;
  const uint64_t bal = __ballot(keep);
  if (lane == 0) { s_w[wv] = __popcll(bal); s_p[wv] = before; }
  __syncthreads();
  int pre = 0, tot = 0, first = *base;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) { pre += w < wv ? s_w[w] : 0; tot += s_w[w]; first += s_p[w]; }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *o.count = first + tot;
  if (!keep) return;
  const int m = min(max(matches12[idx1], 0), n_2 - 1);
  has1[idx1] = 1;
  has2[m] = 1;
  const int64_t p = (int64_t)first + pre + __popcll(bal & dev::lanemask_lt());
  if (p < 0 || p >= o.cap) return;
  const int64_t g1 = (int64_t)o1 + idx1, g2 = (int64_t)o2 + m;
  const double X = x3d[3 * (int64_t)idx1], Y = x3d[3 * (int64_t)idx1 + 1], Z = x3d[3 * (int64_t)idx1 + 2];
  o.kp1[p] = idx1; o.kp2[p] = m; o.nb[p] = neighbour;
  o.pos[3 * p] = X; o.pos[3 * p + 1] = Y; o.pos[3 * p + 2] = Z;
  // UpdateNormalAndDepth over {KF1, KF2} in the map's (pointer) order, pRefKF = KF1
  const double* M1 = k.m_t + 16 * (int64_t)i1;
  const double* M2 = k.m_t + 16 * (int64_t)i2;
  const double Ow1[3] = {M1[3], M1[7], M1[11]}, Ow2[3] = {M2[3], M2[7], M2[11]};
  double nx = 0.0, ny = 0.0, nz = 0.0;
  mpt::add_view_dir(X, Y, Z, kf2_first ? Ow2 : Ow1, nx, ny, nz);
  mpt::add_view_dir(X, Y, Z, kf2_first ? Ow1 : Ow2, nx, ny, nz);
  mpt::mean_dir(nx, ny, nz, 2, o.normal + 3 * p);
  const int level = min(max(k.kp_oct[g1], 0), k.L - 1);
  mpt::dist_range(mpt::ref_dist(X, Y, Z, Ow1), k.scale, k.L, level, o.dmin[p], o.dmax[p]);
  // ComputeDistinctiveDescriptors with two observations: BestIdx = 0, the first in map order
  const int64_t src = (kf2_first ? g2 : g1) * k.bytes;
  const int nw = k.bytes >> 2;
  const uint32_t* sd = reinterpret_cast<const uint32_t*>(k.desc + src);
  uint32_t* dd = reinterpret_cast<uint32_t*>(o.desc + p * k.bytes);
  for (int w = 0; w < nw; w++) dd[w] = sd[w];
  if (k.mask && o.mask) {
    const uint32_t* sm = reinterpret_cast<const uint32_t*>(k.mask + src);
    uint32_t* dm = reinterpret_cast<uint32_t*>(o.mask + p * k.bytes);
    for (int w = 0; w < nw; w++) dm[w] = sm[w];
  }
}

using host::bad_arg;

static Kf dev_kf(const mcs_fuse_targets* k) {
  return Kf{k->n_targets, k->n_kp_total, k->n_cams, k->bytes, k->n_levels, k->off, k->kp_xy, k->kp_octave,
            k->kp_cam, k->desc, k->mask, k->rays, k->m_t, k->m_c, k->cam, k->scale};
}

static Out dev_out(const mcs_new_points* o) {
  return Out{o->cap, o->count, o->kp1, o->kp2, o->neighbour, o->pos, o->normal, o->min_dist, o->max_dist,
             o->desc, o->mask};
}

// what both device entries and the host entry require of the set and the outputs
static int check_common(const mcs_fuse_targets* kfs, const mcs_new_points* out) {
  if (!kfs || !out) return bad_arg("new points: null keyframe set / outputs");
  if (kfs->n_cams < 1 || kfs->n_cams > kMaxCams) return bad_arg("new points: 1 to 8 cameras");
  if (int rc = host::check_desc_bytes(kfs->bytes, "new points")) return rc;
  if ((kfs->mask != nullptr) != (out->mask != nullptr))
    return bad_arg("new points: descriptor masks for the keyframes and the outputs, or for neither");
  if (kfs->n_targets < 1 || kfs->n_kp_total < 0 || kfs->n_levels < 1 || out->cap < 0)
    return bad_arg("new points: negative count, empty set or empty pyramid");
  if (!kfs->off || !kfs->m_t || !kfs->m_c || !kfs->cam || !kfs->scale || !out->count)
    return bad_arg("new points: null buffer");
  if (kfs->n_kp_total > 0 && (!kfs->kp_xy || !kfs->kp_octave || !kfs->kp_cam || !kfs->desc || !kfs->rays))
    return bad_arg("new points: null buffer");
  if (out->cap > 0 && (!out->kp1 || !out->kp2 || !out->neighbour || !out->pos || !out->normal || !out->min_dist ||
                       !out->max_dist || !out->desc))
    return bad_arg("new points: null buffer");
  return MCS_OK;
}

}  // namespace npt
}  // namespace mcs

using namespace mcs;

struct mcs_newpts_workspace {
  int device = 0, max_n1 = 0;
  uint8_t* verdict = nullptr;    // [max_n1]
  double* x3d = nullptr;         // [max_n1][3]
  int32_t* bcnt = nullptr;       // [(max_n1 + kBlock - 1) / kBlock]
  int32_t* base = nullptr;       // [1] first output row of the running pair; [1] the matcher's count
  int32_t* matches = nullptr;    // [max_n1]
};

extern "C" {

int mcs_newpts_workspace_create(int32_t device, int32_t max_n1, mcs_newpts_workspace** out) {
  if (!out || max_n1 < 1 || device < 0) return host::bad_arg("new points workspace: need max_n1 >= 1 and a device ordinal >= 0");
  if (int rc = host::open_device(device, "new points workspace")) return rc;
  mcs_newpts_workspace* w = new mcs_newpts_workspace;
  w->device = device;
  w->max_n1 = max_n1;
  const size_t n = (size_t)max_n1;
  hipError_t e = hipMalloc((void**)&w->verdict, n);
  if (e == hipSuccess) e = hipMalloc((void**)&w->x3d, 3 * n * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->bcnt, ((n + npt::kBlock - 1) / npt::kBlock) * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&w->base, 2 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&w->matches, n * sizeof(int32_t));
  if (e != hipSuccess) {
    mcs_newpts_workspace_destroy(w);
    set_hip_error(e, "new points workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_newpts_workspace_destroy(mcs_newpts_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  for (void* p : {(void*)w->verdict, (void*)w->x3d, (void*)w->bcnt, (void*)w->base, (void*)w->matches})
    if (p) (void)hipFree(p);
  delete w;
}

int mcs_new_points_pair_device(mcs_newpts_workspace* ws, const mcs_fuse_targets* kfs, int32_t i1, int32_t i2,
                               int32_t n1, int32_t neighbour, const int32_t* d_matches12, int32_t kf2_first,
                               uint8_t* d_has_mp1, uint8_t* d_has_mp2, uint8_t* d_verdict,
                               const mcs_new_points* out, void* stream) {
  if (int rc = npt::check_common(kfs, out)) return rc;
  if (i1 < 0 || i2 < 0 || i1 >= kfs->n_targets || i2 >= kfs->n_targets || i1 == i2)
    return host::bad_arg("new points: i1 and i2 must be two different keyframes of the set");
  if (!ws) return host::bad_arg("new points: null workspace");
  if (n1 < 0 || n1 > ws->max_n1) return host::bad_arg("new points: n1 above the workspace capacity");
  if (n1 == 0) return MCS_OK;
  if (!d_matches12 || !d_has_mp1 || !d_has_mp2) return host::bad_arg("new points: null buffer");
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  const npt::Kf k = npt::dev_kf(kfs);
  uint8_t* verd = d_verdict ? d_verdict : ws->verdict;
  const dim3 g((unsigned)((n1 + npt::kBlock - 1) / npt::kBlock));
  const double cos_thresh = std::cos(3.0 * 3.14159265358979323846 / 180.0);   // src/cLocalMapping.cpp:39
  hipLaunchKernelGGL(npt::k_np_verdict, g, dim3(npt::kBlock), 0, st, k, i1, i2, n1, d_matches12, cos_thresh, verd,
                     ws->x3d, ws->bcnt, ws->base, out->count);
  hipLaunchKernelGGL(npt::k_np_admit, g, dim3(npt::kBlock), 0, st, k, i1, i2, n1, neighbour, kf2_first ? 1 : 0,
                     d_matches12, verd, ws->x3d, ws->bcnt, ws->base, d_has_mp1, d_has_mp2, npt::dev_out(out));
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_create_new_map_points_device(mcs_newpts_workspace* ws, mcs_tri_workspace* tri,
                                     const mcs_fuse_targets* kfs, const int32_t* h_n_kp, const uint8_t* h_skip,
                                     const uint8_t* h_kf2_first, const double* d_E, uint8_t* d_has_mp,
                                     int32_t th_low, double epi_thresh, int32_t* d_matches12, uint8_t* d_verdict,
                                     const mcs_new_points* out, void* stream) {
  if (int rc = npt::check_common(kfs, out)) return rc;
  if (!ws || !tri || !h_n_kp) return host::bad_arg("new points: null workspace / counts");
  const int T = kfs->n_targets - 1, C = kfs->n_cams;
  int64_t sum = 0;
  for (int t = 0; t <= T; t++) {
    if (h_n_kp[t] < 0) return host::bad_arg("new points: negative keypoint count");
    sum += h_n_kp[t];
  }
  if (sum != kfs->n_kp_total) return host::bad_arg("new points: the keypoint counts must add up to n_kp_total");
  const int n1 = h_n_kp[0];
  if (n1 > ws->max_n1) return host::bad_arg("new points: n1 above the workspace capacity");
  if (T > 0 && (!h_skip || !h_kf2_first || !d_E || (sum > 0 && !d_has_mp))) return host::bad_arg("new points: null buffer");
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  MCS_HIP_CHECK(hipMemsetAsync(out->count, 0, sizeof(int32_t), st));
  const size_t nb = (size_t)kfs->bytes;
  int64_t o2 = n1;
  for (int i = 0; i < T; o2 += h_n_kp[i + 1], i++) {
    int32_t* m12 = d_matches12 ? d_matches12 + (size_t)i * n1 : ws->matches;
    uint8_t* vd = d_verdict ? d_verdict + (size_t)i * n1 : nullptr;
    const int n2 = h_n_kp[i + 1];
    if (h_skip[i] || n1 == 0) {
      if (d_matches12 && n1 > 0) MCS_HIP_CHECK(hipMemsetAsync(m12, 0xFF, 4 * (size_t)n1, st));
      if (vd && n1 > 0) MCS_HIP_CHECK(hipMemsetAsync(vd, 0, (size_t)n1, st));
      continue;
    }
    int rc = mcs_search_for_triangulation_raw_device(
        tri, kfs->desc, kfs->mask, kfs->kp_cam, d_has_mp, kfs->rays, n1, kfs->desc + o2 * nb,
        kfs->mask ? kfs->mask + o2 * nb : nullptr, kfs->kp_cam + o2, d_has_mp + o2, kfs->rays + 3 * o2, n2, C,
        d_E + 9 * (size_t)i * C * C, kfs->bytes, th_low, epi_thresh, m12, ws->base + 1, st);
    if (rc) return rc;
    rc = mcs_new_points_pair_device(ws, kfs, 0, i + 1, n1, i, m12, h_kf2_first[i], d_has_mp, d_has_mp + o2, vd, out,
                                    st);
    if (rc) return rc;
  }
  return MCS_OK;
}

int mcs_create_new_map_points(int32_t device, const mcs_fuse_targets* kfs, const uint8_t* skip,
                              const uint8_t* kf2_first, const double* E, uint8_t* has_mp, int32_t th_low,
                              double epi_thresh, int32_t* matches12, uint8_t* verdict, const mcs_new_points* out) {
  if (int rc = npt::check_common(kfs, out)) return rc;
  if (device < 0) return host::bad_arg("new points: no such device");
  const int T = kfs->n_targets - 1, C = kfs->n_cams;
  const size_t nk = (size_t)kfs->n_kp_total, nb = (size_t)kfs->bytes, cap = (size_t)out->cap;
  if (int rc = host::check_set_offsets(kfs->off, kfs->n_targets, kfs->n_kp_total, 1 << 19, "new points")) return rc;
  if (int rc = host::check_kp_cam(kfs->kp_cam, kfs->n_kp_total, C, "new points")) return rc;
  if (T > 0 && (!skip || !kf2_first || !E || (nk > 0 && !has_mp))) return host::bad_arg("new points: null buffer");
  std::vector<int32_t> n_kp((size_t)T + 1);
  int max_n2 = 1;
  for (int t = 0; t <= T; t++) {
    n_kp[t] = kfs->off[t + 1] - kfs->off[t];
    if (t > 0) max_n2 = std::max(max_n2, n_kp[t]);
  }
  const size_t n1 = (size_t)n_kp[0];
  if (int rc = host::open_device(device, "new points")) return rc;
  host::DevBufs B;
  mcs_fuse_targets d;
  if (int rc = host::upload_kf_set(B, *kfs, host::kKfCam | host::kKfRays, &d)) return rc;
  d.kp_xy = B.up(kfs->kp_xy, 2 * nk);
  d.desc = B.up(kfs->desc, nk * nb);
  d.mask = B.up(kfs->mask, nk * nb);
  d.scale = B.up(kfs->scale, (size_t)kfs->n_levels);
  const double* d_E = B.up(E, 9 * (size_t)T * C * C);
  uint8_t* d_has = B.up(has_mp, nk);
  int32_t* d_m12 = matches12 ? B.alloc<int32_t>((size_t)T * n1) : nullptr;
  uint8_t* d_vd = verdict ? B.alloc<uint8_t>((size_t)T * n1) : nullptr;
  mcs_new_points o = *out;
  o.count = B.alloc<int32_t>(1);
  o.kp1 = B.alloc<int32_t>(cap); o.kp2 = B.alloc<int32_t>(cap); o.neighbour = B.alloc<int32_t>(cap);
  o.pos = B.alloc<double>(3 * cap); o.normal = B.alloc<double>(3 * cap);
  o.min_dist = B.alloc<double>(cap); o.max_dist = B.alloc<double>(cap);
  o.desc = B.alloc<uint8_t>(cap * nb);
  o.mask = out->mask ? B.alloc<uint8_t>(cap * nb) : nullptr;
  if (B.err != hipSuccess) { set_hip_error(B.err, "new points upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  mcs_newpts_workspace* ws = nullptr;
  mcs_tri_workspace* tri = nullptr;
  int rc = mcs_newpts_workspace_create(device, (int32_t)std::max<size_t>(n1, 1), &ws);
  if (!rc) rc = mcs_tri_workspace_create(device, (int32_t)std::max<size_t>(n1, 1), max_n2, &tri);
  if (!rc)
    rc = mcs_create_new_map_points_device(ws, tri, &d, n_kp.data(), skip, kf2_first, d_E, d_has, th_low, epi_thresh,
                                          d_m12, d_vd, &o, nullptr);
  hipError_t e = hipDeviceSynchronize();
  mcs_newpts_workspace_destroy(ws);
  if (tri) mcs_tri_workspace_destroy(tri);
  if (rc) return rc;
  MCS_HIP_CHECK(e);
  int32_t count = 0;
  B.down(&count, o.count, 1);
  const size_t n = std::min<size_t>((size_t)std::max(count, 0), cap);
  B.down(out->kp1, o.kp1, n); B.down(out->kp2, o.kp2, n); B.down(out->neighbour, o.neighbour, n);
  B.down(out->pos, o.pos, 3 * n); B.down(out->normal, o.normal, 3 * n);
  B.down(out->min_dist, o.min_dist, n); B.down(out->max_dist, o.max_dist, n);
  B.down(out->desc, o.desc, n * nb);
  B.down(out->mask, o.mask, n * nb);
  B.down(has_mp, d_has, nk);
  B.down(matches12, d_m12, (size_t)T * n1);
  B.down(verdict, d_vd, (size_t)T * n1);
  if (B.err != hipSuccess) { set_hip_error(B.err, "new points download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  *out->count = count;
  if ((size_t)std::max(count, 0) > cap) {
    set_error("new points: more points created than the outputs hold (count returned)");
    return MCS_ERR_CAPACITY;
  }
  return MCS_OK;
}

}  // extern "C"
