// The numeric core of the block-sparse LDL^T over a plan (essential_graph_plan.hpp): what one
// workgroup does for one supernode, written once for the device kernels
// (essential_graph_sparse.hpp) and the host program tests/cpp/essgraph_sparse_host.cpp.
//
// An executor X says who runs it: X.tid of X.nt workers, X.sync() a barrier over them that also
// orders their memory accesses, X.raise(bits) ORs into the solve's flag word.  On the host one
// worker runs everything and sync() does nothing; on the device the workers are the lanes of one
// workgroup.  Between two barriers every entry has one owner, and an owner adds its contributions
// in the plan's order (sources ascending, then the supernode's own columns ascending), so the
// result does not depend on the number of workers: the host and the device give the same bits.
//
//   sn_factor   left-looking: the panel minus the sources' L D L^T, then the dense LDL^T of the
//               panel column by column; D per scalar row; the right-hand side rides along as one
//               more column, so y = L^-1 b (own rows), the update u = L_below y the ancestors
//               subtract, and z = D^-1 y come out of the same pass.  A zero pivot raises
//               kFlagZeroPivot and leaves zeros in its column.
//   sn_backward x = z - L_below^T x(ancestors), then the back substitution with the own triangle;
//               x leaves in keyframe order.
//
// No HIP include.  Needs -ffp-contract=off.
#pragma once
#include "essential_graph_plan.hpp"

namespace mcs {
namespace esg {

constexpr int kSpFlagZeroPivot = 1;      // ldlt::kFlagZeroPivot

// The numbers of a plan.  A0: the assembled panels; L: the panels of the trial (sn_factor copies
// its own from A0, adds lambda to the diagonal and leaves L in place); LT: per supernode its rows
// below the own ones once more, transposed (column c at c (M - W)), so that a target's update reads
// along rows;
// D [B n] by permuted row; b [B n] in keyframe order; y [B n] by permuted row (y, then z);
// u [B rows] by position in the row lists; xp [B n] by permuted row; x [B n] in keyframe order.
struct SpNum {
  const double* A0; double lambda; double* L; double* LT; double* D; const double* b; double* y; double* u; double* xp; double* x;
};

template <int B, class X>
MCS_LM_FN void sn_factor(const SpView& v, const SpNum& m, int t, X& ex) {
  const int c0 = v.col0[t], ns = v.col0[t + 1] - c0, r0 = v.rowptr[t], nr = v.rowptr[t + 1] - r0;
  const int W = B * ns, M = B * nr;
  double* P = m.L + (size_t)B * B * v.blkoff[t];
  double* D = m.D + (size_t)B * c0;
  double* y = m.y + (size_t)B * c0;
  double* u = m.u + (size_t)B * r0;          // rows [W, M) are used
  const double* P0 = m.A0 + (size_t)B * B * v.blkoff[t];
  for (int idx = ex.tid; idx < M * W; idx += ex.nt) {
    const int r = idx / W, q = idx % W;
    if (r >= q) P[idx] = r == q ? P0[idx] + m.lambda : P0[idx];
  }
  for (int q = ex.tid; q < M; q += ex.nt) {
    if (q < W) y[q] = m.b[B * v.iperm[c0 + q / B] + q % B];
    else u[q] = 0.0;
  }
  ex.sync();
  for (int k = v.srcptr[t]; k < v.srcptr[t + 1]; k++) {
    const int s = v.src_s[k], p0 = v.src_p0[k], p1 = v.src_p1[k];
    const int32_t* map = v.relmap + v.src_map[k];
    const int sc0 = v.col0[s], nss = v.col0[s + 1] - sc0, Ws = B * nss, sr0 = v.rowptr[s], nrs = v.rowptr[s + 1] - sr0;
    const int Mb = B * (nrs - nss);                 // the source's rows below its own, transposed in LT
    const double* Xt = m.LT + (size_t)B * B * v.blkoff[s] + B * (p0 - nss);
    const double* Ds = m.D + (size_t)B * sc0;
    const double* us = m.u + (size_t)B * sr0;
    const int R = B * (nrs - p0), C = B * (p1 - p0);
    for (int idx = ex.tid; idx < R * C; idx += ex.nt) {
      const int ri = idx / C, cj = idx % C;
      if (ri < cj) continue;
      double sum = 0.0;
      for (int c = 0; c < Ws; c++) sum += Xt[(size_t)c * Mb + ri] * Ds[c] * Xt[(size_t)c * Mb + cj];
      P[(size_t)(B * map[ri / B] + ri % B) * W + (B * map[cj / B] + cj % B)] -= sum;
    }
    for (int idx = ex.tid; idx < C; idx += ex.nt) y[B * map[idx / B] + idx % B] -= us[B * p0 + idx];
    ex.sync();
  }
  // the panel's own LDL^T, a block column at a time; every entry sees its subtractions in the
  // order of the scalar columns
  for (int jb = 0; jb < ns; jb++) {
    const int q0 = B * jb;
    if (ex.tid == 0) {                               // the diagonal block and its part of y, in registers
      double T[B][B], yy[B];
      for (int i = 0; i < B; i++) {
        yy[i] = y[q0 + i];
        for (int j = 0; j <= i; j++) T[i][j] = P[(size_t)(q0 + i) * W + q0 + j];
      }
      for (int c = 0; c < B; c++) {
        const double d = T[c][c];
        if (d == 0.0) ex.raise(kSpFlagZeroPivot);
        for (int i = c + 1; i < B; i++) T[i][c] = d == 0.0 ? 0.0 : T[i][c] / d;
        for (int i = c + 1; i < B; i++) {
          for (int j = c + 1; j <= i; j++) T[i][j] -= T[i][c] * d * T[j][c];
          yy[i] -= T[i][c] * yy[c];
        }
        D[q0 + c] = d;
      }
      for (int i = 0; i < B; i++) {
        y[q0 + i] = yy[i];
        for (int j = 0; j <= i; j++) P[(size_t)(q0 + i) * W + q0 + j] = T[i][j];
      }
    }
    ex.sync();
    for (int r = q0 + B + ex.tid; r < M; r += ex.nt) {      // the rows below the block
      double* row = P + (size_t)r * W + q0;
      double val[B];
      for (int c = 0; c < B; c++) val[c] = row[c];
      for (int c = 0; c < B; c++) {
        const double d = D[q0 + c];
        const double l = d == 0.0 ? 0.0 : val[c] / d;
        val[c] = l;
        for (int c2 = c + 1; c2 < B; c2++) val[c2] -= l * d * P[(size_t)(q0 + c2) * W + q0 + c];
      }
      for (int c = 0; c < B; c++) row[c] = val[c];
    }
    ex.sync();
    const int r1 = q0 + B, R = M - r1, C = W - r1 + 1;      // the last column of the rectangle is the right-hand side
    for (int idx = ex.tid; idx < R * C; idx += ex.nt) {
      const int r = r1 + idx / C, q = r1 + idx % C;
      const double* lr = P + (size_t)r * W + q0;
      if (q == W) {
        double acc = r < W ? y[r] : u[r];
        if (r < W) { for (int c = 0; c < B; c++) acc -= lr[c] * y[q0 + c]; y[r] = acc; }
        else { for (int c = 0; c < B; c++) acc += lr[c] * y[q0 + c]; u[r] = acc; }
      } else if (r >= q) {
        const double* lq = P + (size_t)q * W + q0;
        double acc = P[(size_t)r * W + q];
        for (int c = 0; c < B; c++) acc -= lr[c] * D[q0 + c] * lq[c];
        P[(size_t)r * W + q] = acc;
      }
    }
    ex.sync();
  }
  {                                                  // the rows below, transposed, for the targets' updates
    const int Mb = M - W;
    double* Xt = m.LT + (size_t)B * B * v.blkoff[t];
    for (int idx = ex.tid; idx < Mb * W; idx += ex.nt) Xt[(size_t)(idx % W) * Mb + idx / W] = P[(size_t)W * W + idx];
  }
  for (int q = ex.tid; q < W; q += ex.nt) y[q] = D[q] == 0.0 ? 0.0 : y[q] / D[q];
  ex.sync();
}

template <int B, class X>
MCS_LM_FN void sn_backward(const SpView& v, const SpNum& m, int t, X& ex) {
  const int c0 = v.col0[t], ns = v.col0[t + 1] - c0, r0 = v.rowptr[t], nr = v.rowptr[t + 1] - r0;
  const int W = B * ns, M = B * nr;
  const double* P = m.L + (size_t)B * B * v.blkoff[t];
  const double* z = m.y + (size_t)B * c0;
  double* w = m.xp + (size_t)B * c0;
  const int32_t* rows = v.rows + r0;
  for (int q = ex.tid; q < W; q += ex.nt) {
    double acc = z[q];
    for (int r = W; r < M; r++) acc -= P[(size_t)r * W + q] * m.xp[B * rows[r / B] + r % B];
    w[q] = acc;
  }
  ex.sync();
  for (int p = W - 1; p > 0; p--) {
    const double xv = w[p];
    for (int q = ex.tid; q < p; q += ex.nt) w[q] -= P[(size_t)p * W + q] * xv;
    ex.sync();
  }
  for (int q = ex.tid; q < W; q += ex.nt) m.x[B * v.iperm[c0 + q / B] + q % B] = w[q];
  ex.sync();
}

struct HostExec {
  int tid = 0, nt = 1;
  int* flag;
  void sync() {}
  void raise(int bits) { *flag |= bits; }
};

}  // namespace esg
}  // namespace mcs
