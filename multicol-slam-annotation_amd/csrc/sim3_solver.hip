// cSim3Solver on the device: the constructor, SetRansacParameters and iterate, for ONE current
// keyframe KF1 against a batch of T loop candidates KF2_t, plus the hand-over of the inliers to
// SearchBySim3.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cSim3Solver::cSim3Solver                             src/cSim3Solver.cpp:44-137
//   cSim3Solver::SetRansacParameters                     src/cSim3Solver.cpp:139-165
//   cSim3Solver::iterate / find                          src/cSim3Solver.cpp:167-262
//   cSim3Solver::centroid / computeT                     src/cSim3Solver.cpp:264-371
//   cSim3Solver::CheckInliers                            src/cSim3Solver.cpp:374-415
//   cMultiCamSys_::WorldToCamHom_fast                    src/cam_system_omni.cpp:92-112
//   cCamModelGeneral_::WorldToImg                        src/cam_model_omni.cpp:147-163
//   cConverter::invMat                                   src/cConverter.cpp:31-44
//   vbAlreadyMatched1/2 of SearchBySim3                  src/cORBmatcher.cpp:1758-1774
// A hypothesis depends on no RANSAC state (every iteration samples afresh from mvAllIndices), so
// one call evaluates all its iterations of all candidates in parallel: k_s3s_hyp (Horn's closed
// form per (candidate, iteration)), k_s3s_check (CheckInliers, lanes over correspondences) and
// k_s3s_resolve, which applies the sequential acceptance rule to the counts in iteration order.
// Compiled with -ffp-contract=off; the prepare and check kernels follow the reference's
// expression order (cv::Matx products: s = 0; s += a_k * b_k, k ascending) through frm:: of
// omni_geom.hpp.  cv::eigen and cv::Rodrigues are OpenCV internals: the hypothesis is Horn's
// solution to rounding, not bitwise.
#include "host_util.hpp"
#include "omni_geom.hpp"
#include "sim3_draws.hpp"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <initializer_list>
#include <type_traits>
#include <vector>

namespace mcs {
namespace s3s {

constexpr int kMaxCams = 8;
constexpr int kMaxKp = 1 << 19;
constexpr int kHyp = 34;           // doubles per hypothesis: s, R 9, t 3, sR 9, sRinv 9, tinv 3
constexpr int kHB = 8;             // hypotheses per block of k_s3s_check (two per wave)
constexpr int kChunk = 256;        // correspondences staged per round
constexpr int kPrep = 1024;        // threads of k_s3s_prepare's one block per candidate
constexpr int kRow = 12;           // doubles per staged row: X1 3, X2 3, p1 2, p2 2, maxerr1, maxerr2

struct Set {
  int n_kp_total;
  const int32_t* off; const int32_t* kp_oct; const int32_t* kp_cam;
  const double* m_t; const double* m_c; const double* cam;
};

struct Corr {
  int T, cap, C;
  const double* m_c; const double* cam;
  int32_t* n; int32_t* idx1; double* X1; double* X2; double* p1; double* p2;
  int32_t* cam1; int32_t* cam2; double* maxerr1; double* maxerr2;
};

struct Ransac {
  int32_t* iterations; int32_t* best_inliers; int32_t* max_its; uint64_t* best_words;
  double* s12; double* R12; double* t12; double* T12;
  int32_t* success; int32_t* no_more; int32_t* n_inliers; uint8_t* inlier;
  double* hyp_srt; int32_t* hyp_inl;
};

struct Work { double* hyp; uint64_t* words; int32_t* inl; double* imc; };

// mvnMaxError1 / 2 are std::vector<size_t> (include/cSim3Solver.h:92-93): push_back(9.210 * sigma2)
// truncates toward zero, and CheckInliers compares err < (double)that.  Values outside size_t's
// range (undefined in the text) give 0 or 2^64.
__device__ __forceinline__ double trunc_size_t(double v) {
  if (!(v > 0.0)) return 0.0;
  return v < 18446744073709551616.0 ? floor(v) : 18446744073709551616.0;
}

// ------------------------------------------------------------------------------ the constructor
// One block per candidate (:71-134).  kPrep slots i1 per round (each round is a chain of dependent
// loads, so a round is made wide); the kept ones get consecutive rows in i1 order (the order of
// mvnIndices1) by a ballot prefix inside each wave and a scan over the wave totals.  The rounds
// only place the slot numbers; the rows themselves are computed afterwards, all at once.
__global__ __launch_bounds__(kPrep) void k_s3s_prepare(Set k1, Set k2, const double* __restrict__ pos1,
                                                     const double* __restrict__ pos2,
                                                     const int32_t* __restrict__ matches12,
                                                     const uint8_t* __restrict__ ok1,
                                                     const uint8_t* __restrict__ ok2,
                                                     const int32_t* __restrict__ first1,
                                                     const int32_t* __restrict__ first2,
                                                     const double* __restrict__ sigma2, int L, Corr c) {
  __shared__ int s_w[kPrep / 64];
  __shared__ double s_h[24];     // hom1 = invMat(M_t of KF1), hom2 = invMat(M_t of KF2_t): R 9, t 3 each
  const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n1 = c.cap;
  const int o1 = min(max(k1.off[0], 0), k1.n_kp_total);
  const int n_1 = min(min(max(k1.off[1] - o1, 0), k1.n_kp_total - o1), n1);
  const int o2 = min(max(k2.off[t], 0), k2.n_kp_total);
  const int n_2 = min(max(k2.off[t + 1] - o2, 0), k2.n_kp_total - o2);
  if (threadIdx.x == 0) frm::inv_mat44(k1.m_t, s_h, s_h + 9);
  if (threadIdx.x == 64) frm::inv_mat44(k2.m_t + 16 * (int64_t)t, s_h + 12, s_h + 21);
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < n1; i0 += kPrep) {
    const int i1 = i0 + threadIdx.x;
    bool keep = false;
    if (i1 < n_1) {
      const int m = matches12[(int64_t)t * n1 + i1];
      if (m >= 0 && m < n_2 && ok1[i1] != 0 && ok2[o2 + m] != 0) {
        const int f1 = first1[i1], f2 = first2[o2 + m];
        if (f1 >= 0 && f1 < n_1 && f2 >= 0 && f2 < n_2) {
          const int oc1 = k1.kp_oct[o1 + f1], c1 = k1.kp_cam[o1 + f1];
          const int oc2 = k2.kp_oct[o2 + f2], c2 = k2.kp_cam[o2 + f2];
          keep = oc1 >= 0 && oc1 < L && oc2 >= 0 && oc2 < L && c1 >= 0 && c1 < c.C && c2 >= 0 && c2 < c.C;
        }
      }
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) s_w[wv] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < kPrep / 64; w++) { pre += w < wv ? s_w[w] : 0; tot += s_w[w]; }
    if (keep) c.idx1[(int64_t)t * n1 + base + pre + __popcll(bal & dev::lanemask_lt())] = i1;
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) c.n[t] = base;
  // the rows, all at once: the slot of row j is idx1[j], which passed every test above
  for (int j = threadIdx.x; j < base; j += kPrep) {
    const int64_t r = (int64_t)t * n1 + j;
    const int i1 = min(max(c.idx1[r], 0), max(n_1 - 1, 0));
    const int m = min(max(matches12[(int64_t)t * n1 + i1], 0), max(n_2 - 1, 0));
    const int f1 = min(max(first1[i1], 0), max(n_1 - 1, 0)), f2 = min(max(first2[o2 + m], 0), max(n_2 - 1, 0));
    const int oc1 = min(max(k1.kp_oct[o1 + f1], 0), L - 1), oc2 = min(max(k2.kp_oct[o2 + f2], 0), L - 1);
    const int c1 = min(max(k1.kp_cam[o1 + f1], 0), c.C - 1), c2 = min(max(k2.kp_cam[o2 + f2], 0), c.C - 1);
    const double* P1 = pos1 + 3 * (int64_t)(o1 + i1);
    const double* P2 = pos2 + 3 * (int64_t)(o2 + m);
    const double Xa[3] = {P1[0], P1[1], P1[2]}, Xb[3] = {P2[0], P2[1], P2[2]};
    double R[9], tt[3], u, v, y[3];
    c.maxerr1[r] = trunc_size_t(__dmul_rn(9.210, sigma2[oc1]));
    c.maxerr2[r] = trunc_size_t(__dmul_rn(9.210, sigma2[oc2]));
    frm::mtmc44(k1.m_t, k1.m_c + 16 * c1, R, tt);
    frm::world_to_cam_img(R, tt, k1.cam + 17 * c1, Xa, u, v);
    c.p1[2 * r] = u; c.p1[2 * r + 1] = v;
    frm::rot_add(s_h, Xa, s_h + 9, y);
    c.X1[3 * r] = y[0]; c.X1[3 * r + 1] = y[1]; c.X1[3 * r + 2] = y[2];
    c.cam1[r] = c1;
    frm::mtmc44(k2.m_t + 16 * (int64_t)t, k2.m_c + 16 * c2, R, tt);
    frm::world_to_cam_img(R, tt, k2.cam + 17 * c2, Xb, u, v);
    c.p2[2 * r] = u; c.p2[2 * r + 1] = v;
    frm::rot_add(s_h + 12, Xb, s_h + 21, y);
    c.X2[3 * r] = y[0]; c.X2[3 * r + 1] = y[1]; c.X2[3 * r + 2] = y[2];
    c.cam2[r] = c2;
  }
}

// ------------------------------------------------------------------------------ the RANSAC
// Thread t < T: SetRansacParameters (:139-165) when flags ask for it, and the constructor's zero
// state with MCS_SIM3_INIT.  Threads T + c: invMat(M_c[c]) (:391-392).  Every thread below T * n1
// clears one vbInliers entry (:174).
__global__ __launch_bounds__(256) void k_s3s_params(int T, int C, int n1, int W, int flags, double prob,
                                                    int min_inl, int cap_its, const int32_t* __restrict__ n,
                                                    const double* __restrict__ m_c, double* __restrict__ imc,
                                                    Ransac r) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (int64_t)T * n1) r.inlier[idx] = 0;
  if (idx >= T + C) return;
  if (idx >= T) {
    const int c = (int)idx - T;
    frm::inv_mat44(m_c + 16 * c, imc + 12 * c, imc + 12 * c + 9);
    return;
  }
  if (!flags) return;
  const int t = (int)idx;
  const int N = min(max(n[t], 0), n1);
  int its;
  if (N < min_inl) {
    its = 0;                                   // iterate returns at :177 whatever mRansacMaxIts holds
  } else if (N == min_inl) {
    its = 1;
  } else {
    const double eps = __ddiv_rn((double)min_inl, (double)N);
    const double v = ceil(__ddiv_rn(log(__dsub_rn(1.0, prob)), log(__dsub_rn(1.0, pow(eps, 3.0)))));
    // eps^3 below 2^-53 makes the denominator 0 and v -inf, whose int conversion the text leaves
    // undefined: such an N needs the most iterations, so the cap
    const double lim = (v >= 1.0 && v < (double)cap_its) ? v : (double)cap_its;
    its = lim > 1.0 ? (int)lim : 1;
  }
  r.max_its[t] = its;
  r.iterations[t] = 0;
  if (flags & MCS_SIM3_INIT) {
    r.best_inliers[t] = 0;
    r.s12[t] = 0.0;
    for (int k = 0; k < 9; k++) r.R12[9 * t + k] = 0.0;
    for (int k = 0; k < 3; k++) r.t12[3 * t + k] = 0.0;
    for (int k = 0; k < 16; k++) r.T12[16 * t + k] = 0.0;
    for (int w = 0; w < W; w++) r.best_words[(int64_t)t * W + w] = 0;
  }
}

// one Jacobi rotation of the symmetric 4x4 a that zeroes a[P][Q]; v collects the rotations
template <int P, int Q>
__device__ __forceinline__ void jrot(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  double tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) tn = -tn;
  const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
  a[P][P] -= tn * apq;
  a[Q][Q] += tn * apq;
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (r != P && r != Q) {
      const double arp = a[r][P], arq = a[r][Q];
      a[r][P] = a[P][r] = cs * arp - sn * arq;
      a[r][Q] = a[Q][r] = sn * arp + cs * arq;
    }
    const double vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = cs * vrp - sn * vrq;
    v[r][Q] = sn * vrp + cs * vrq;
  }
}

// computeT (:286-371) on the three correspondences i[0..2] of X1 / X2 -> o[kHyp]
__device__ inline void horn(const double* __restrict__ X1, const double* __restrict__ X2, const int* i,
                            double* o) {
  double P1[3][3], P2[3][3], O1[3], O2[3];   // P(row, point)
  for (int j = 0; j < 3; j++)
    for (int r = 0; r < 3; r++) { P1[r][j] = X1[3 * (int64_t)i[j] + r]; P2[r][j] = X2[3 * (int64_t)i[j] + r]; }
  const double third = 1.0 / 3.0;              // Vec /= 3.0 multiplies by 1. / alpha
  for (int r = 0; r < 3; r++) {
    O1[r] = (((0.0 + P1[r][0]) + P1[r][1]) + P1[r][2]) * third;
    O2[r] = (((0.0 + P2[r][0]) + P2[r][1]) + P2[r][2]) * third;
    for (int j = 0; j < 3; j++) { P1[r][j] -= O1[r]; P2[r][j] -= O2[r]; }
  }
  double M[3][3];                              // M = Pr2 * Pr1.t()
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += P2[r][k] * P1[c][k];
      M[r][c] = s;
    }
  double a[4][4], v[4][4];
  a[0][0] = M[0][0] + M[1][1] + M[2][2];
  a[0][1] = M[1][2] - M[2][1];
  a[0][2] = M[2][0] - M[0][2];
  a[0][3] = M[0][1] - M[1][0];
  a[1][1] = M[0][0] - M[1][1] - M[2][2];
  a[1][2] = M[0][1] + M[1][0];
  a[1][3] = M[2][0] + M[0][2];
  a[2][2] = -M[0][0] + M[1][1] - M[2][2];
  a[2][3] = M[1][2] + M[2][1];
  a[3][3] = -M[0][0] - M[1][1] + M[2][2];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (c < r) a[r][c] = a[c][r];
      v[r][c] = r == c ? 1.0 : 0.0;
    }
  // cyclic Jacobi: sweeps until the off-diagonal part is below 1e-18 of the whole (or 30 sweeps)
  for (int sweep = 0; sweep < 30; sweep++) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
    const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]);
    if (off <= 1e-18 * (off + dia)) break;
    jrot<0, 1>(a, v); jrot<0, 2>(a, v); jrot<0, 3>(a, v);
    jrot<1, 2>(a, v); jrot<1, 3>(a, v); jrot<2, 3>(a, v);
  }
  double q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]}, top = a[0][0];   // the first maximum
#pragma unroll
  for (int c = 1; c < 4; c++)
    if (a[c][c] > top) { top = a[c][c]; q[0] = v[0][c]; q[1] = v[1][c]; q[2] = v[2][c]; q[3] = v[3][c]; }
  const double nv = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double ang = atan2(nv, q[0]);
  const double k2 = 2.0 * ang / nv;            // 0 / 0 = NaN for the identity quaternion, as in the text
  double rv[3] = {q[1] * k2, q[2] * k2, q[3] * k2};
  double* R = o + 1;
  const double theta = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
  if (theta < DBL_EPSILON) {                   // cv::Rodrigues
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  } else {
    const double cs = cos(theta), sn = sin(theta), c1 = 1.0 - cs, it = 1.0 / theta;
    const double x = rv[0] * it, y = rv[1] * it, z = rv[2] * it;
    R[0] = cs + c1 * x * x;      R[1] = c1 * x * y - sn * z;  R[2] = c1 * x * z + sn * y;
    R[3] = c1 * x * y + sn * z;  R[4] = cs + c1 * y * y;      R[5] = c1 * y * z - sn * x;
    R[6] = c1 * x * z - sn * y;  R[7] = c1 * y * z + sn * x;  R[8] = cs + c1 * z * z;
  }
  double nom = 0.0, den = 0.0;                 // P3 = R * Pr2; nom = Pr1.dot(P3); den = sum of P3^2
  for (int r = 0; r < 3; r++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += R[3 * r + k] * P2[k][j];
      nom += P1[r][j] * s;
      den += s * s;
    }
  const double sc = nom / den, inv = 1.0 / sc;
  o[0] = sc;
  double* sR = o + 13;
  double* sRi = o + 22;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      sR[3 * r + c] = __dmul_rn(R[3 * r + c], sc);       // ms12i * mR12i
      sRi[3 * r + c] = __dmul_rn(R[3 * c + r], inv);     // (1.0 / ms12i) * mR12i.t()
    }
  for (int r = 0; r < 3; r++) {                          // mt12i = O1 - ms12i * mR12i * O2
    double s = 0.0;
    for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(sR[3 * r + k], O2[k]));
    o[10 + r] = __dsub_rn(O1[r], s);
  }
  for (int r = 0; r < 3; r++) {                          // tinv = -sRinv * mt12i
    double s = 0.0;
    for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(__dmul_rn(sRi[3 * r + k], -1.0), o[10 + k]));
    o[31 + r] = s;
  }
}

// One thread per (candidate, iteration of this call): iteration it = iterations[t] + k draws
// samples[t][it] (:202-222) and solves (:224).  Iterations at or past max_its get the count -1.
__global__ __launch_bounds__(64) void k_s3s_hyp(Corr c, const int32_t* __restrict__ samples, int n_it,
                                                int cap_its, Ransac r, Work w) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= c.T * n_it) return;
  const int t = gid / n_it, k = gid - t * n_it;
  const int N = min(max(c.n[t], 0), c.cap);
  const int64_t it = (int64_t)r.iterations[t] + k;
  const int64_t h = (int64_t)t * n_it + k;
  if (r.iterations[t] < 0 || it >= r.max_its[t] || it >= cap_its || N < 1) {
    w.inl[h] = -1;
    if (r.hyp_inl) r.hyp_inl[h] = -1;
    return;
  }
  int idx[3];
  for (int j = 0; j < 3; j++) idx[j] = min(max(samples[((int64_t)t * cap_its + it) * 3 + j], 0), N - 1);
  double o[kHyp];
  horn(c.X1 + 3 * (int64_t)t * c.cap, c.X2 + 3 * (int64_t)t * c.cap, idx, o);
  double* dst = w.hyp + kHyp * h;
  for (int j = 0; j < kHyp; j++) dst[j] = o[j];
  w.inl[h] = 0;                                  // evaluated: k_s3s_check puts the count here
  if (r.hyp_srt)
    for (int j = 0; j < 13; j++) r.hyp_srt[13 * h + j] = o[j];
}

// CheckInliers (:374-415).  Block (x, t) takes kHB hypotheses of candidate t, two per wave, and
// walks the candidate's correspondences kChunk at a time: the rows are staged in LDS once per
// block, every wave reads them for its hypotheses, 64 rows per ballot.  NaN fails both `<`.
__global__ __launch_bounds__(256) void k_s3s_check(Corr c, int n_it, Ransac r, Work w, int W) {
  __shared__ double s_row[kRow][kChunk];
  __shared__ int s_cam[2][kChunk];
  __shared__ double s_imc[kMaxCams * 12];
  const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int N = min(max(c.n[t], 0), c.cap);
  const int64_t row0 = (int64_t)t * c.cap;
  for (int j = threadIdx.x; j < 12 * c.C; j += 256) s_imc[j] = w.imc[j];
  int cnt[kHB / 4];
  bool live[kHB / 4];
#pragma unroll
  for (int j = 0; j < kHB / 4; j++) {
    const int k = blockIdx.x * kHB + wv + 4 * j;
    cnt[j] = 0;
    live[j] = k < n_it && w.inl[(int64_t)t * n_it + min(k, n_it - 1)] != -1;
  }
  for (int c0 = 0; c0 < N; c0 += kChunk) {
    __syncthreads();
    {
      const int i = c0 + threadIdx.x;
      if (i < N) {
        const int64_t g = row0 + i;
        for (int j = 0; j < 3; j++) { s_row[j][threadIdx.x] = c.X1[3 * g + j]; s_row[3 + j][threadIdx.x] = c.X2[3 * g + j]; }
        for (int j = 0; j < 2; j++) { s_row[6 + j][threadIdx.x] = c.p1[2 * g + j]; s_row[8 + j][threadIdx.x] = c.p2[2 * g + j]; }
        s_row[10][threadIdx.x] = c.maxerr1[g];
        s_row[11][threadIdx.x] = c.maxerr2[g];
        s_cam[0][threadIdx.x] = c.cam1[g];
        s_cam[1][threadIdx.x] = c.cam2[g];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kHB / 4; j++) {
      if (!live[j]) continue;
      const int k = blockIdx.x * kHB + wv + 4 * j;
      const double* hy = w.hyp + kHyp * ((int64_t)t * n_it + k);
      for (int r0 = 0; r0 < kChunk && c0 + r0 < N; r0 += 64) {
        const int row = r0 + lane;
        bool ok = false;
        if (c0 + row < N) {
          const int ca = s_cam[0][row], cb = s_cam[1][row];
          if (ca >= 0 && ca < c.C && cb >= 0 && cb < c.C) {
            const double Xa[3] = {s_row[0][row], s_row[1][row], s_row[2][row]};
            const double Xb[3] = {s_row[3][row], s_row[4][row], s_row[5][row]};
            double p21[3], p12[3], q1[3], q2[3], u1, v1, u2, v2;
            frm::hom_mul(hy + 13, hy + 10, Xb, p21);            // pt2_in_1 = mT12i * X2
            frm::hom_mul(hy + 22, hy + 31, Xa, p12);            // pt1_in_2 = mT21i * X1
            frm::hom_mul(s_imc + 12 * ca, s_imc + 12 * ca + 9, p21, q1);
            frm::hom_mul(s_imc + 12 * cb, s_imc + 12 * cb + 9, p12, q2);
            frm::world_to_img(c.cam + 17 * ca, q1[0], q1[1], q1[2], u1, v1);
            frm::world_to_img(c.cam + 17 * cb, q2[0], q2[1], q2[2], u2, v2);
            const double d1x = __dsub_rn(s_row[6][row], u1), d1y = __dsub_rn(s_row[7][row], v1);
            const double d2x = __dsub_rn(u2, s_row[8][row]), d2y = __dsub_rn(v2, s_row[9][row]);
            const double e1 = __dadd_rn(__dmul_rn(d1x, d1x), __dmul_rn(d1y, d1y));
            const double e2 = __dadd_rn(__dmul_rn(d2x, d2x), __dmul_rn(d2y, d2y));
            ok = e1 < s_row[10][row] && e2 < s_row[11][row];
          }
        }
        const uint64_t bal = __ballot(ok);
        if (lane == 0) w.words[((int64_t)t * n_it + k) * W + ((c0 + r0) >> 6)] = bal;
        cnt[j] += __popcll(bal);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kHB / 4; j++) {
    const int k = blockIdx.x * kHB + wv + 4 * j;
    if (live[j] && lane == 0) {
      w.inl[(int64_t)t * n_it + k] = cnt[j];
      if (r.hyp_inl) r.hyp_inl[(int64_t)t * n_it + k] = cnt[j];
    }
  }
}

// One wave per candidate: the acceptance rule of :228-253 over the counts in iteration order.
// B_k = max(mnBestInliers at entry, counts before k); iteration k updates the best when
// count_k >= B_k and is a hit when also count_k > min_inliers.
__global__ __launch_bounds__(64) void k_s3s_resolve(Corr c, int n_it, int min_inl, Ransac r, Work w, int W) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const int N = min(max(c.n[t], 0), c.cap);
  const int its0 = max(r.iterations[t], 0), mx = r.max_its[t];
  const int nv = min(max(mx - its0, 0), n_it);
  int carry = r.best_inliers[t], kbest = -1, khit = -1;
  for (int k0 = 0; k0 < nv && khit < 0; k0 += 64) {
    const int k = k0 + lane;
    const int inl = k < nv ? w.inl[(int64_t)t * n_it + k] : -1;
    int inc = inl;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_up(inc, s, 64);
      if (lane >= s) inc = max(inc, o);
    }
    int ex = __shfl_up(inc, 1, 64);
    ex = lane == 0 ? carry : max(carry, ex);
    const bool upd = k < nv && inl >= ex;
    const uint64_t hb = __ballot(upd && inl > min_inl), ub = __ballot(upd);
    if (hb) {
      khit = k0 + __ffsll((unsigned long long)hb) - 1;
      kbest = khit;
    } else if (ub) {
      kbest = k0 + 63 - __clzll((long long)ub);
    }
    carry = max(carry, __shfl(inc, 63, 64));
  }
  int best = 0;
  if (kbest >= 0) {
    const int64_t h = (int64_t)t * n_it + kbest;
    const double* hy = w.hyp + kHyp * h;
    best = w.inl[h];
    if (lane == 0) { r.best_inliers[t] = best; r.s12[t] = hy[0]; }
    if (lane < 9) r.R12[9 * t + lane] = hy[1 + lane];
    if (lane < 3) r.t12[3 * t + lane] = hy[10 + lane];
    if (lane < 16) {                              // Rt2Hom(sR, mt12i)
      const int i = lane >> 2, j = lane & 3;
      r.T12[16 * t + lane] = i == 3 ? (j == 3 ? 1.0 : 0.0) : (j == 3 ? hy[10 + i] : hy[13 + 3 * i + j]);
    }
    for (int x = lane; x < W; x += 64) r.best_words[(int64_t)t * W + x] = 64 * x < N ? w.words[h * W + x] : 0;
  }
  if (khit >= 0) {                                // :239-245; k_s3s_params cleared the row
    const uint64_t* wd = w.words + ((int64_t)t * n_it + khit) * W;
    for (int i = lane; i < N; i += 64)
      if ((wd[i >> 6] >> (i & 63)) & 1) {
        const int j = c.idx1[(int64_t)t * c.cap + i];
        if (j >= 0 && j < c.cap) r.inlier[(int64_t)t * c.cap + j] = 1;
      }
  }
  if (lane == 0) {
    const int its = khit >= 0 ? its0 + khit + 1 : its0 + nv;
    r.iterations[t] = its;
    r.success[t] = khit >= 0;
    r.n_inliers[t] = khit >= 0 ? best : 0;
    r.no_more[t] = khit < 0 && its >= mx;
  }
}

// ------------------------------------------------------------------------------ the hand-over
// vbAlreadyMatched1/2 as SearchBySim3 builds them (cORBmatcher.cpp:1758-1774) from the
// vpMatches12 the call site passes: the inliers' entries alone (cLoopClosing.cpp:354-360).
__global__ __launch_bounds__(256) void k_s3s_active_fill(int T, int n1, int n2, const uint8_t* __restrict__ inlier,
                                                         const uint8_t* __restrict__ good1,
                                                         const uint8_t* __restrict__ good2,
                                                         uint8_t* __restrict__ active1, uint8_t* __restrict__ active2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nd1 = (int64_t)T * n1;
  if (i < nd1) active1[i] = good1[i % n1] != 0 && inlier[i] == 0;
  else if (i < nd1 + n2) active2[i - nd1] = good2[i - nd1] != 0;
}

__global__ __launch_bounds__(256) void k_s3s_active_clear(int n1, int n2, const int32_t* __restrict__ off2,
                                                          const uint8_t* __restrict__ inlier,
                                                          const int32_t* __restrict__ matches12,
                                                          const int32_t* __restrict__ first2,
                                                          uint8_t* __restrict__ active2) {
  const int t = blockIdx.y, i1 = blockIdx.x * blockDim.x + threadIdx.x;
  if (i1 >= n1 || inlier[(int64_t)t * n1 + i1] == 0) return;
  const int o2 = min(max(off2[t], 0), n2);
  const int n_2 = min(max(off2[t + 1] - o2, 0), n2 - o2);
  const int m = matches12[(int64_t)t * n1 + i1];
  if (m < 0 || m >= n_2) return;
  const int f = first2[o2 + m];
  if (f >= 0 && f < n_2) active2[o2 + f] = 0;
}

using host::bad_arg;

static int check_sets(const mcs_fuse_targets* k1, const mcs_fuse_targets* k2) {
  if (!k1 || !k2) return bad_arg("sim3 solver: null keyframe set");
  if (k1->n_targets != 1) return bad_arg("sim3 solver: kf1 must be a set of exactly one keyframe");
  if (k1->n_cams < 1 || k1->n_cams > kMaxCams || k1->n_cams != k2->n_cams || k1->n_levels != k2->n_levels)
    return bad_arg("sim3 solver: 1 to 8 cameras; n_cams and n_levels of kf1 and kf2s must agree (shared rig)");
  if (k2->n_targets < 0 || k1->n_kp_total < 0 || k2->n_kp_total < 0 || k1->n_levels < 1)
    return bad_arg("sim3 solver: negative count or empty pyramid");
  if (k1->n_kp_total >= kMaxKp) return bad_arg("sim3 solver: keypoints per keyframe must be below 2^19");
  return MCS_OK;
}

static bool set_nulls(const mcs_fuse_targets* k) {
  return !k->off || !k->m_t || !k->m_c || !k->cam || (k->n_kp_total > 0 && (!k->kp_octave || !k->kp_cam));
}

static int check_prepare(const mcs_fuse_targets* k1, const mcs_sim3_points* p1, const mcs_fuse_targets* k2,
                         const mcs_sim3_points* p2, const void* m12, const void* ok1, const void* ok2,
                         const void* f1, const void* f2, const void* sigma2, const mcs_sim3_corr* c) {
  int rc = check_sets(k1, k2);
  if (rc) return rc;
  if (!p1 || !p2 || !c) return bad_arg("sim3 solver: null points / correspondences");
  if (p1->n != k1->n_kp_total || p2->n != k2->n_kp_total)
    return bad_arg("sim3 solver: the points must hold one slot per keypoint of their set");
  if (c->n_targets != k2->n_targets || c->cap != k1->n_kp_total || c->n_cams != k1->n_cams)
    return bad_arg("sim3 solver: correspondences need n_targets = T, cap = n1 and n_cams of the rig");
  if (k2->n_targets == 0) return MCS_OK;
  if (set_nulls(k1) || set_nulls(k2) || !sigma2 || !c->n) return bad_arg("sim3 solver: null buffer");
  if (k1->n_kp_total > 0 &&
      (!p1->pos || !m12 || !ok1 || !f1 || !c->idx1 || !c->X1 || !c->X2 || !c->p1 || !c->p2 || !c->cam1 ||
       !c->cam2 || !c->maxerr1 || !c->maxerr2))
    return bad_arg("sim3 solver: null buffer");
  if (k2->n_kp_total > 0 && (!p2->pos || !ok2 || !f2)) return bad_arg("sim3 solver: null buffer");
  return MCS_OK;
}

static int check_iterate(const mcs_sim3_corr* c, const void* samples, int n_it, double prob, int min_inl,
                         int cap_its, int flags, const mcs_sim3_ransac* r, bool host) {
  if (!c || !r) return bad_arg("sim3 solver: null correspondences / state");
  if (c->n_targets < 0 || c->cap < 0 || c->cap >= kMaxKp || c->n_cams < 1 || c->n_cams > kMaxCams)
    return bad_arg("sim3 solver: bad correspondence set");
  if (n_it < 1 || cap_its < 1 || n_it > cap_its) return bad_arg("sim3 solver: 1 <= n_iterations <= max_its_cap");
  if (min_inl < 1) return bad_arg("sim3 solver: min_inliers must be at least 1");
  if (!(prob > 0.0 && prob < 1.0)) return bad_arg("sim3 solver: probability must lie inside (0, 1)");
  if (flags & ~(MCS_SIM3_INIT | MCS_SIM3_SET_PARAMS)) return bad_arg("sim3 solver: unknown flag");
  if ((int64_t)c->n_targets * cap_its >= INT_MAX / 4 || (int64_t)c->n_targets * std::max(c->cap, 1) >= INT_MAX / 2)
    return bad_arg("sim3 solver: batch too large for one launch");
  if (c->n_targets == 0) return MCS_OK;
  if (!samples || !r->iterations || !r->best_inliers || !r->max_its || !r->s12 || !r->R12 || !r->t12 ||
      !r->T12 || !r->success || !r->no_more || !r->n_inliers)
    return bad_arg("sim3 solver: null buffer");
  if (!host && (!c->m_c || !c->cam || !c->n)) return bad_arg("sim3 solver: null buffer");
  if (c->cap > 0 && (!r->best_words || !r->inlier)) return bad_arg("sim3 solver: null buffer");
  if (!host && c->cap > 0 &&
      (!c->idx1 || !c->X1 || !c->X2 || !c->p1 || !c->p2 || !c->cam1 || !c->cam2 || !c->maxerr1 || !c->maxerr2))
    return bad_arg("sim3 solver: null buffer");
  return MCS_OK;
}

static Set dev_set(const mcs_fuse_targets* k) {
  return Set{k->n_kp_total, k->off, k->kp_octave, k->kp_cam, k->m_t, k->m_c, k->cam};
}

static Corr dev_corr(const mcs_sim3_corr* c) {
  return Corr{c->n_targets, c->cap, c->n_cams, c->m_c, c->cam, c->n, c->idx1, c->X1, c->X2, c->p1, c->p2,
              c->cam1, c->cam2, c->maxerr1, c->maxerr2};
}

static Ransac dev_ransac(const mcs_sim3_ransac* r) {
  return Ransac{r->iterations, r->best_inliers, r->max_its, r->best_words, r->s12, r->R12, r->t12, r->T12,
                r->success, r->no_more, r->n_inliers, r->inlier, r->hyp_srt, r->hyp_inl};
}

}  // namespace s3s
}  // namespace mcs

using namespace mcs;

struct mcs_sim3_solver_workspace {
  int device = 0, max_targets = 0, max_kp = 0, max_its = 0;
  double* hyp = nullptr;       // [max_targets][max_its][kHyp]
  uint64_t* words = nullptr;   // [max_targets][max_its][(max_kp + 63) / 64]
  int32_t* inl = nullptr;      // [max_targets][max_its]
  double* imc = nullptr;       // [8][12]
};

extern "C" {

int mcs_sim3_draw_samples(int32_t n, const int32_t* draws, int32_t n_its, int32_t* samples) {
  if (n_its < 0 || (n_its > 0 && (!draws || !samples))) return host::bad_arg("sim3 draws: null buffer or negative count");
  if (sim3_draw_samples(n, draws, n_its, samples)) return host::bad_arg("sim3 draws: n >= 3 and every draw inside [0, n)");
  return MCS_OK;
}

int mcs_sim3_solver_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp, int32_t max_its_cap,
                                     mcs_sim3_solver_workspace** out) {
  if (!out || max_targets < 1 || max_kp < 1 || max_kp >= s3s::kMaxKp || max_its_cap < 1 ||
      (int64_t)max_targets * max_its_cap >= INT_MAX / 4 || (int64_t)max_targets * max_kp >= INT_MAX / 2) {
    set_error("sim3 solver workspace: bad argument");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "sim3 solver workspace")) return rc;
  mcs_sim3_solver_workspace* w = new mcs_sim3_solver_workspace;
  w->device = device;
  w->max_targets = max_targets;
  w->max_kp = max_kp;
  w->max_its = max_its_cap;
  const size_t nh = (size_t)max_targets * max_its_cap, W = ((size_t)max_kp + 63) / 64;
  hipError_t e = hipMalloc((void**)&w->hyp, nh * s3s::kHyp * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->words, nh * W * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc((void**)&w->inl, nh * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&w->imc, 12 * s3s::kMaxCams * sizeof(double));
  if (e != hipSuccess) {
    mcs_sim3_solver_workspace_destroy(w);
    set_hip_error(e, "sim3 solver workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_sim3_solver_workspace_destroy(mcs_sim3_solver_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->hyp) (void)hipFree(w->hyp);
  if (w->words) (void)hipFree(w->words);
  if (w->inl) (void)hipFree(w->inl);
  if (w->imc) (void)hipFree(w->imc);
  delete w;
}

int mcs_sim3_solver_prepare_device(const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                                   const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2,
                                   const int32_t* d_matches12, const uint8_t* d_ok1, const uint8_t* d_ok2,
                                   const int32_t* d_first1, const int32_t* d_first2, const double* d_sigma2,
                                   const mcs_sim3_corr* corr, void* stream) {
  int rc = s3s::check_prepare(kf1, pts1, kf2s, pts2, d_matches12, d_ok1, d_ok2, d_first1, d_first2, d_sigma2, corr);
  if (rc) return rc;
  const int T = kf2s->n_targets;
  if (T == 0) return MCS_OK;
  hipLaunchKernelGGL(s3s::k_s3s_prepare, dim3(T), dim3(s3s::kPrep), 0, (hipStream_t)stream, s3s::dev_set(kf1),
                     s3s::dev_set(kf2s), pts1->pos, pts2->pos, d_matches12, d_ok1, d_ok2, d_first1, d_first2,
                     d_sigma2, kf1->n_levels, s3s::dev_corr(corr));
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_sim3_solver_iterate_device(mcs_sim3_solver_workspace* ws, const mcs_sim3_corr* corr,
                                   const int32_t* d_samples, int32_t n_iterations, double prob,
                                   int32_t min_inliers, int32_t max_its_cap, int32_t flags,
                                   const mcs_sim3_ransac* ransac, void* stream) {
  int rc = s3s::check_iterate(corr, d_samples, n_iterations, prob, min_inliers, max_its_cap, flags, ransac, false);
  if (rc) return rc;
  const int T = corr->n_targets, n1 = corr->cap, C = corr->n_cams;
  if (T == 0) return MCS_OK;
  if (ws && (T > ws->max_targets || n1 > ws->max_kp || n_iterations > ws->max_its)) {
    set_error("sim3 solver: more candidates, keypoints or iterations than the workspace holds");
    return MCS_ERR_ARG;
  }
  mcs_sim3_solver_workspace* tmp = nullptr;
  if (!ws) {
    int dev = 0;
    MCS_HIP_CHECK(hipGetDevice(&dev));
    rc = mcs_sim3_solver_workspace_create(dev, T, std::max(n1, 1), n_iterations, &tmp);
    if (rc) return rc;
    ws = tmp;
  } else {
    MCS_HIP_CHECK(hipSetDevice(ws->device));
  }
  hipStream_t st = (hipStream_t)stream;
  const int W = (n1 + 63) / 64;
  const s3s::Corr c = s3s::dev_corr(corr);
  const s3s::Ransac r = s3s::dev_ransac(ransac);
  const s3s::Work w{ws->hyp, ws->words, ws->inl, ws->imc};
  const int64_t np = std::max<int64_t>(T + C, (int64_t)T * n1);
  hipLaunchKernelGGL(s3s::k_s3s_params, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, T, C, n1, W, flags,
                     prob, min_inliers, max_its_cap, corr->n, corr->m_c, ws->imc, r);
  hipLaunchKernelGGL(s3s::k_s3s_hyp, dim3((T * n_iterations + 63) / 64), dim3(64), 0, st, c, d_samples,
                     n_iterations, max_its_cap, r, w);
  hipLaunchKernelGGL(s3s::k_s3s_check, dim3((n_iterations + s3s::kHB - 1) / s3s::kHB, T), dim3(256), 0, st, c,
                     n_iterations, r, w, W);
  hipLaunchKernelGGL(s3s::k_s3s_resolve, dim3(T), dim3(64), 0, st, c, n_iterations, min_inliers, r, w, W);
  hipError_t e = hipGetLastError();
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    mcs_sim3_solver_workspace_destroy(tmp);
  }
  MCS_HIP_CHECK(e);
  return MCS_OK;
}

int mcs_sim3_solver_active_device(const mcs_fuse_targets* kf1, const mcs_fuse_targets* kf2s,
                                  const uint8_t* d_inlier, const uint8_t* d_good1, const uint8_t* d_good2,
                                  const int32_t* d_matches12, const int32_t* d_first2, uint8_t* d_active1,
                                  uint8_t* d_active2, void* stream) {
  if (!kf1 || !kf2s) return host::bad_arg("sim3 solver: null keyframe set");
  if (kf1->n_targets != 1 || kf2s->n_targets < 0 || kf1->n_kp_total < 0 || kf2s->n_kp_total < 0)
    return host::bad_arg("sim3 solver: kf1 must be a set of exactly one keyframe; no negative counts");
  const int T = kf2s->n_targets, n1 = kf1->n_kp_total, n2 = kf2s->n_kp_total;
  if ((int64_t)T * n1 + n2 >= (int64_t)INT_MAX) return host::bad_arg("sim3 solver: batch too large for one launch");
  if (T == 0) return MCS_OK;
  if (!kf2s->off || (n1 > 0 && (!d_inlier || !d_good1 || !d_matches12 || !d_active1)) ||
      (n2 > 0 && (!d_good2 || !d_active2 || (n1 > 0 && !d_first2))))
    return host::bad_arg("sim3 solver: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nt = (int64_t)T * n1 + n2;
  if (nt > 0)
    hipLaunchKernelGGL(s3s::k_s3s_active_fill, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, T, n1, n2,
                       d_inlier, d_good1, d_good2, d_active1, d_active2);
  if (n1 > 0 && n2 > 0)
    hipLaunchKernelGGL(s3s::k_s3s_active_clear, dim3((n1 + 255) / 256, T), dim3(256), 0, st, n1, n2, kf2s->off,
                       d_inlier, d_matches12, d_first2, d_active2);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_sim3_solver(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                    const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2, const int32_t* matches12,
                    const uint8_t* ok1, const uint8_t* ok2, const int32_t* first1, const int32_t* first2,
                    const double* sigma2, const int32_t* samples, int32_t n_iterations, double prob,
                    int32_t min_inliers, int32_t max_its_cap, int32_t flags, const mcs_sim3_corr* corr,
                    const mcs_sim3_ransac* ransac, const uint8_t* good1, const uint8_t* good2,
                    uint8_t* active1, uint8_t* active2) {
  int rc = s3s::check_sets(kf1, kf2s);
  if (rc) return rc;
  mcs_sim3_corr hc{};                      // the caller's (nullable) output pointers
  if (corr) hc = *corr;
  hc.n_targets = kf2s->n_targets; hc.cap = kf1->n_kp_total; hc.n_cams = kf1->n_cams;
  mcs_sim3_corr full = hc;                 // what check_prepare sees: every output present
  int32_t dummy_i = 0; double dummy_d = 0.0;
  full.n = &dummy_i; full.idx1 = full.cam1 = full.cam2 = &dummy_i;
  full.X1 = full.X2 = full.p1 = full.p2 = full.maxerr1 = full.maxerr2 = &dummy_d;
  if ((rc = s3s::check_prepare(kf1, pts1, kf2s, pts2, matches12, ok1, ok2, first1, first2, sigma2, &full))) return rc;
  if ((rc = s3s::check_iterate(&full, samples, n_iterations, prob, min_inliers, max_its_cap, flags, ransac, true)))
    return rc;
  const int T = kf2s->n_targets;
  const size_t n1 = (size_t)kf1->n_kp_total, n2 = (size_t)kf2s->n_kp_total;
  if ((active1 || active2) && ((n1 > 0 && (!good1 || !active1)) || (n2 > 0 && (!good2 || !active2))))
    return host::bad_arg("sim3 solver: the hand-over needs good1, good2, active1 and active2");
  if (T == 0) return MCS_OK;
  for (const mcs_fuse_targets* k : {kf1, kf2s})
    if ((rc = host::check_set_offsets(k->off, k->n_targets, k->n_kp_total, 0, "sim3 solver"))) return rc;
  if ((rc = host::open_device(device, "sim3 solver"))) return rc;
  host::DevBufs B;
  auto upload = [&](const mcs_fuse_targets* k, const mcs_sim3_points* p, mcs_fuse_targets* d, mcs_sim3_points* dp) {
    *dp = *p;
    dp->pos = B.up(p->pos, 3 * (size_t)k->n_kp_total);
    dp->dist = nullptr; dp->desc = dp->mask = nullptr;
    return host::upload_kf_set(B, *k, host::kKfCam, d);   // no search: neither grids nor descriptors
  };
  mcs_fuse_targets d1, d2;
  mcs_sim3_points dp1, dp2;
  if ((rc = upload(kf1, pts1, &d1, &dp1)) || (rc = upload(kf2s, pts2, &d2, &dp2))) return rc;
  const size_t nr = (size_t)T * n1, W = (n1 + 63) / 64, nh = (size_t)T * n_iterations;
  const int32_t* d_m12 = B.up(matches12, nr);
  const uint8_t* d_ok1 = B.up(ok1, n1);
  const uint8_t* d_ok2 = B.up(ok2, n2);
  const int32_t* d_f1 = B.up(first1, n1);
  const int32_t* d_f2 = B.up(first2, n2);
  const double* d_sig = B.up(sigma2, (size_t)kf1->n_levels);
  const int32_t* d_smp = B.up(samples, 3 * (size_t)T * max_its_cap);
  mcs_sim3_corr dc = hc;
  dc.m_c = d1.m_c; dc.cam = d1.cam;
  dc.n = B.alloc<int32_t>(T); dc.idx1 = B.alloc<int32_t>(nr); dc.cam1 = B.alloc<int32_t>(nr); dc.cam2 = B.alloc<int32_t>(nr);
  dc.X1 = B.alloc<double>(3 * nr); dc.X2 = B.alloc<double>(3 * nr); dc.p1 = B.alloc<double>(2 * nr);
  dc.p2 = B.alloc<double>(2 * nr); dc.maxerr1 = B.alloc<double>(nr); dc.maxerr2 = B.alloc<double>(nr);
  mcs_sim3_ransac dr = *ransac;
  const bool init = (flags & MCS_SIM3_INIT) != 0;          // then the state is written, never read
  auto state = [&](auto* h, size_t n) { return init ? B.alloc<std::remove_pointer_t<decltype(h)>>(n) : B.up(h, n); };
  dr.iterations = state(ransac->iterations, T); dr.best_inliers = state(ransac->best_inliers, T);
  dr.max_its = state(ransac->max_its, T); dr.best_words = state(ransac->best_words, T * W);
  dr.s12 = state(ransac->s12, T); dr.R12 = state(ransac->R12, 9 * (size_t)T); dr.t12 = state(ransac->t12, 3 * (size_t)T);
  dr.T12 = state(ransac->T12, 16 * (size_t)T);
  dr.success = B.alloc<int32_t>(T); dr.no_more = B.alloc<int32_t>(T); dr.n_inliers = B.alloc<int32_t>(T);
  dr.inlier = B.alloc<uint8_t>(nr);
  dr.hyp_srt = ransac->hyp_srt ? B.alloc<double>(13 * nh) : nullptr;
  dr.hyp_inl = ransac->hyp_inl ? B.alloc<int32_t>(nh) : nullptr;
  const bool hand = active1 || active2;
  const uint8_t* d_g1 = hand ? B.up(good1, n1) : nullptr;
  const uint8_t* d_g2 = hand ? B.up(good2, n2) : nullptr;
  uint8_t* d_a1 = hand ? B.alloc<uint8_t>(nr) : nullptr;
  uint8_t* d_a2 = hand ? B.alloc<uint8_t>(n2) : nullptr;
  if (B.err == hipSuccess && dr.hyp_srt) B.err = hipMemset(dr.hyp_srt, 0, 13 * nh * sizeof(double));
  if (B.err != hipSuccess) { set_hip_error(B.err, "sim3 solver upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if ((rc = mcs_sim3_solver_prepare_device(&d1, &dp1, &d2, &dp2, d_m12, d_ok1, d_ok2, d_f1, d_f2, d_sig, &dc, nullptr)))
    return rc;
  if ((rc = mcs_sim3_solver_iterate_device(nullptr, &dc, d_smp, n_iterations, prob, min_inliers, max_its_cap, flags,
                                           &dr, nullptr)))
    return rc;
  if (hand && (rc = mcs_sim3_solver_active_device(&d1, &d2, dr.inlier, d_g1, d_g2, d_m12, d_f2, d_a1, d_a2, nullptr)))
    return rc;
  MCS_HIP_CHECK(hipDeviceSynchronize());
  B.down(hc.n, dc.n, (size_t)T);
  B.down(hc.idx1, dc.idx1, nr);
  B.down(hc.cam1, dc.cam1, nr);
  B.down(hc.cam2, dc.cam2, nr);
  B.down(hc.X1, dc.X1, 3 * nr);
  B.down(hc.X2, dc.X2, 3 * nr);
  B.down(hc.p1, dc.p1, 2 * nr);
  B.down(hc.p2, dc.p2, 2 * nr);
  B.down(hc.maxerr1, dc.maxerr1, nr);
  B.down(hc.maxerr2, dc.maxerr2, nr);
  B.down(ransac->iterations, dr.iterations, (size_t)T);
  B.down(ransac->best_inliers, dr.best_inliers, (size_t)T);
  B.down(ransac->max_its, dr.max_its, (size_t)T);
  B.down(ransac->best_words, dr.best_words, T * W);
  B.down(ransac->s12, dr.s12, (size_t)T);
  B.down(ransac->R12, dr.R12, 9 * (size_t)T);
  B.down(ransac->t12, dr.t12, 3 * (size_t)T);
  B.down(ransac->T12, dr.T12, 16 * (size_t)T);
  B.down(ransac->success, dr.success, (size_t)T);
  B.down(ransac->no_more, dr.no_more, (size_t)T);
  B.down(ransac->n_inliers, dr.n_inliers, (size_t)T);
  B.down(ransac->inlier, dr.inlier, nr);
  B.down(ransac->hyp_srt, dr.hyp_srt, 13 * nh);
  B.down(ransac->hyp_inl, dr.hyp_inl, nh);
  B.down(active1, d_a1, nr);
  B.down(active2, d_a2, n2);
  if (B.err != hipSuccess) { set_hip_error(B.err, "sim3 solver download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
