// The per-match loop of cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:272-382) for one
// neighbour as plain single-thread C++: what a caller runs on the host between two device searches
// when the library has no device entry for it.  Written from the description in
// include/mcs_newpoints.h (cv::Matx products accumulate s = 0; s += a_k * b_k; the 2 x 2 inverse is
// d = 1 / det, adjugate * d).  Built as a shared object by tools/bench_new_points.py, which times it
// and requires its points to equal the device's; tests/test_newpoints_ref.py holds it to the NumPy
// restatement.  It is a baseline, not part of the library.
//   g++ -O3 -std=c++17 -ffp-contract=off -shared -fPIC newpoints_cpu.cpp -o libnewpoints_cpu.so
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

inline double dot3(const double* a, const double* b) {
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += a[k] * b[k];
  return s;
}

inline double norm3(const double* a) { return std::sqrt(dot3(a, a)); }

// rows 0..2 of A * B for row-major 4 x 4 matrices
void mul44(const double* A, const double* B, double* O) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += A[4 * i + k] * B[4 * k + j];
      O[4 * i + j] = s;
    }
}

void inv_mat(const double* M, double* O) {   // cConverter::invMat
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
      O[4 * i + k] = M[4 * k + i];
      s += -M[4 * k + i] * M[4 * k + 3];
    }
    O[4 * i + 3] = s;
  }
  O[12] = O[13] = O[14] = 0.0;
  O[15] = 1.0;
}

void mul4v(const double* A, const double* x, double* y) {
  for (int i = 0; i < 4; i++) {
    double s = 0.0;
    for (int k = 0; k < 4; k++) s += A[4 * i + k] * x[k];
    y[i] = s;
  }
}

void world_to_img(const double* cam, double x, double y, double z, double* u, double* v) {
  double norm = std::sqrt(x * x + y * y);
  if (norm == 0.0) norm = 1e-14;
  const double theta = std::atan(-z / norm);
  double rho = 0.0;
  for (int i = 11; i >= 0; i--) rho = rho * theta + cam[5 + i];
  const double uu = x / norm * rho, vv = y / norm * rho;
  *u = uu * cam[0] + vv * cam[1] + cam[3];
  *v = uu * cam[2] + vv + cam[4];
}

struct CamPair { double T[16], Ti[16]; };

}  // namespace

extern "C" int newpoints_cpu_pair(int n_cams, int bytes, int n_levels, const double* m_c, const double* cam,
                                  const double* scale, int n1, const float* xy1, const int32_t* oct1,
                                  const int32_t* cam1, const uint8_t* desc1, const uint8_t* mask1, const double* rays1,
                                  const double* m_t1, int n2, const float* xy2, const int32_t* cam2,
                                  const uint8_t* desc2, const uint8_t* mask2, const double* rays2, const double* m_t2,
                                  const int32_t* matches12, int kf2_first, int neighbour, uint8_t* has1, uint8_t* has2,
                                  uint8_t* verdict, int cap, int32_t* count, int32_t* kp1, int32_t* kp2, int32_t* nbr,
                                  double* pos, double* normal, double* dmin, double* dmax, uint8_t* odesc,
                                  uint8_t* omask) {
  if (n_cams < 1 || n_cams > 8) return -1;
  const double cos_thresh = std::cos(3.0 * 3.14159265358979323846 / 180.0);
  CamPair K1[8], K2[8];
  double rel[8][8][16];
  for (int c = 0; c < n_cams; c++) {
    mul44(m_t1, m_c + 16 * c, K1[c].T);
    inv_mat(K1[c].T, K1[c].Ti);
    mul44(m_t2, m_c + 16 * c, K2[c].T);
    inv_mat(K2[c].T, K2[c].Ti);
  }
  for (int a = 0; a < n_cams; a++)
    for (int b = 0; b < n_cams; b++) mul44(K1[a].Ti, K2[b].T, rel[a][b]);
  const double Ow1[3] = {m_t1[3], m_t1[7], m_t1[11]}, Ow2[3] = {m_t2[3], m_t2[7], m_t2[11]};
  for (int i1 = 0; i1 < n1; i1++) {
    if (verdict) verdict[i1] = 0;
    const int m = matches12[i1];
    if (m < 0 || m >= n2) continue;
    const int c1 = cam1[i1], c2 = cam2[m];
    if (c1 < 0 || c1 >= n_cams || c2 < 0 || c2 >= n_cams) continue;
    const double* T1 = K1[c1].T;
    const double* T2 = K2[c2].T;
    const double* r1 = rays1 + 3 * (size_t)i1;
    const double* r2 = rays2 + 3 * (size_t)m;
    int code = 1;
    double X4[4] = {0, 0, 0, 0};
    do {
      double p[3], q[3];
      for (int i = 0; i < 3; i++) { p[i] = dot3(T1 + 4 * i, r1); q[i] = dot3(T2 + 4 * i, r2); }
      const double cosp = dot3(p, q) / (norm3(p) * norm3(q));
      if (cosp < 0 || cosp > cos_thresh) { code = 2; break; }
      const double* R = rel[c1][c2];
      const double t12[3] = {R[3], R[7], R[11]};
      double f2[3];
      for (int i = 0; i < 3; i++) f2[i] = dot3(R + 4 * i, r2);
      const double b0 = dot3(t12, r1), b1 = dot3(t12, f2);
      const double A00 = dot3(r1, r1), A10 = dot3(r1, f2), A01 = -A10, A11 = -dot3(f2, f2);
      const double det = A00 * A11 - A01 * A10;
      double i00 = 0, i01 = 0, i10 = 0, i11 = 0;
      if (det != 0) {
        const double d = 1.0 / det;
        i00 = A11 * d; i01 = -A01 * d; i10 = -A10 * d; i11 = A00 * d;
      }
      const double l0 = 0.0 + i00 * b0 + i01 * b1, l1 = 0.0 + i10 * b0 + i11 * b1;
      double x3[4];
      for (int i = 0; i < 3; i++) x3[i] = ((r1[i] * l0) + (t12[i] + f2[i] * l1)) / 2.0;
      x3[3] = 1.0;
      mul4v(T1, x3, X4);
      double pr[4], u, v;
      mul4v(K1[c1].Ti, X4, pr);
      if (pr[2] <= 0.0) { code = 3; break; }
      world_to_img(cam + 17 * c1, pr[0], pr[1], pr[2], &u, &v);
      double ex = u - (double)xy1[2 * (size_t)i1], ey = v - (double)xy1[2 * (size_t)i1 + 1];
      if (std::sqrt(ex * ex + ey * ey) > 4.0) { code = 4; break; }
      mul4v(K2[c2].Ti, X4, pr);
      if (pr[2] <= 0.0) { code = 5; break; }
      world_to_img(cam + 17 * c2, pr[0], pr[1], pr[2], &u, &v);
      ex = u - (double)xy2[2 * (size_t)m];
      ey = v - (double)xy2[2 * (size_t)m + 1];
      if (std::sqrt(ex * ex + ey * ey) > 4.0) { code = 6; break; }
      const double n1v[3] = {X4[0] - Ow1[0], X4[1] - Ow1[1], X4[2] - Ow1[2]};
      const double n2v[3] = {X4[0] - Ow2[0], X4[1] - Ow2[1], X4[2] - Ow2[2]};
      const double d1 = norm3(n1v), d2 = norm3(n2v);
      if (d1 == 0 || d2 == 0 || d1 > 25.0 || d2 > 25.0) { code = 7; break; }
    } while (false);
    if (verdict) verdict[i1] = (uint8_t)code;
    if (code != 1) continue;
    has1[i1] = 1;
    has2[m] = 1;
    const int pnt = (*count)++;
    if (pnt >= cap) continue;
    kp1[pnt] = i1; kp2[pnt] = m; nbr[pnt] = neighbour;
    double nrm[3] = {0, 0, 0};
    for (int o = 0; o < 2; o++) {
      const double* O = (o == 0) == (kf2_first != 0) ? Ow2 : Ow1;
      const double ni[3] = {X4[0] - O[0], X4[1] - O[1], X4[2] - O[2]};
      const double ia = 1.0 / norm3(ni);
      for (int i = 0; i < 3; i++) nrm[i] = nrm[i] + ni[i] * ia;
    }
    const double PC[3] = {X4[0] - Ow1[0], X4[1] - Ow1[1], X4[2] - Ow1[2]};
    const double dist = norm3(PC);
    int level = oct1[i1];
    level = level < 0 ? 0 : level >= n_levels ? n_levels - 1 : level;
    const double sf = scale[level];
    for (int i = 0; i < 3; i++) { pos[3 * (size_t)pnt + i] = X4[i]; normal[3 * (size_t)pnt + i] = nrm[i] * (1.0 / 2); }
    dmin[pnt] = (1.0 / sf) * dist / sf;
    dmax[pnt] = sf * dist * scale[n_levels - 1 - level];
    const uint8_t* sd = kf2_first ? desc2 + (size_t)m * bytes : desc1 + (size_t)i1 * bytes;
    std::memcpy(odesc + (size_t)pnt * bytes, sd, (size_t)bytes);
    if (omask && mask1 && mask2)
      std::memcpy(omask + (size_t)pnt * bytes, kf2_first ? mask2 + (size_t)m * bytes : mask1 + (size_t)i1 * bytes,
                  (size_t)bytes);
  }
  return 0;
}
