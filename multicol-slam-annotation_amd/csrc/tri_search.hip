// SearchForTriangulationRaw on the device: the descriptor radius search of one keyframe pair,
// the epipolar verdicts and the ordered vbMatched2 pass.
//
// Reference: SearchForTriangulationRaw          src/cORBmatcher.cpp:968-1156
//            DescriptorDistance64 / ...Masked   src/cORBmatcher.cpp:2443-2477
//            CheckDistEpipolarLine              src/misc.cpp:54-70 (frm::epi_check of omni_geom.hpp:
//            one definition for the host entry of epipolar.cpp and the kernels here)
#include "host_util.hpp"
#include "omni_geom.hpp"
#include "ham_dist.hpp"
#include <map>
#include <mutex>
#include "../../include/mcs_matcher.h"
#include "ldlt.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <new>

namespace mcs {

// ---- SearchForTriangulationRaw on the device (src/cORBmatcher.cpp:1016-1089)
// The reference walks KF1's keypoints in index order; for each it sorts the (dist, idx2) list of
// unmatched same-camera KF2 keypoints with dist <= TH_LOW, takes best = the first list entry,
// and accepts the first entry with dist <= cvRound(2 best) that passes CheckDistEpipolarLine,
// marking it in vbMatched2.  With keys (dist << 20 | idx2) the sorted order is key order.  The
// only state between queries is vbMatched2, and KF2 keypoint i2 can only be taken by a query
// that lists it AND passes the epipolar check with it.  Kernels (stream-ordered):
//   k_tri_radius  (query tiles x train segments): each (query, segment) thread appends its
//                 candidate keys to its own kTriSub slots (no returning atomics in the loop),
//                 counts how many queries list each KF2 keypoint, flags slot overflow
//   k_tri_pass    (one thread per query and segment): the epipolar verdict of every stored
//                 candidate into bit 30, and how many queries pass with each KF2 keypoint
//   k_tri_private (one thread per query): a query none of whose candidates another query could
//                 take, and none of whose passing candidates another query lists, decides alone
//                 (its outcome neither depends on nor changes anyone's vbMatched2 view); the
//                 others are marked -2 and flagged for the ordered pass.  After any overflow the
//                 pass counts are incomplete, so every query goes to the ordered pass.
//   two exclusive scans (rocPRIM) give each flagged query its place and key offset
//   k_tri_gather  (one wave per flagged query): its keys sorted into one flat array, flagged
//                 queries in index order
//   k_tri_seq     (one wave per camera): the flagged queries in index order against an LDS
//                 vbMatched2 bitmap, streaming the flat keys through two LDS windows with the
//                 next window prefetched; per query a ballot finds the first unmatched key
//                 (best) and a second the first unmatched passing key with dist <= 2 best.  A
//                 query whose candidates overflowed a slot rescans KF2 on the fly (exact, rare).
constexpr int kTriSeg = 16;                 // train segments of k_tri_radius (grid.y)
constexpr int kTriSub = 96;                 // candidate slots per (query, segment)
constexpr int kTriCap = kTriSeg * kTriSub;  // per query
constexpr int kTriWin = 1024;    // keys per k_tri_seq LDS window (16 per lane)
constexpr uint32_t kTriPass = 1u << 30, kTriKey = kTriPass - 1;

template <int W, bool MASKED>
__global__ __launch_bounds__(kHamThreads) void k_tri_radius(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ MA, const int32_t* __restrict__ camA,
    const uint8_t* __restrict__ hasA, int na, const uint8_t* __restrict__ B,
    const uint8_t* __restrict__ MB, const int32_t* __restrict__ camB,
    const uint8_t* __restrict__ hasB, int nb, int ncams, int th, uint32_t* __restrict__ cand,
    int32_t* __restrict__ cnt, int32_t* __restrict__ ref_all, int32_t* __restrict__ overflow) {
  __shared__ uint4 tile[kHamTile * (W / 4)];
  __shared__ uint4 mtile[MASKED ? kHamTile * (W / 4) : 1];
  __shared__ int tcam[kHamTile];
  const int qi = blockIdx.x * kHamThreads + threadIdx.x;
  const int seg = blockIdx.y;
  uint32_t q[W], qm[W];
  int qc = -1;
#pragma unroll
  for (int w = 0; w < W; w++) { q[w] = 0; qm[w] = 0; }
  if (qi < na) {
    qc = camA[qi];
    if (hasA[qi] || qc < 0 || qc >= ncams) qc = -1;   // inactive: no candidates
  }
  if (qc >= 0) {
    load_desc_row<W>(q, A + (int64_t)qi * W * 4);
    if (MASKED) load_desc_row<W>(qm, MA + (int64_t)qi * W * 4);
  }
  uint32_t* const out = cand + ((int64_t)(qi < na ? qi : 0) * kTriSeg + seg) * kTriSub;
  int n = 0;
  const int per = ((nb + kTriSeg - 1) / kTriSeg + kHamTile - 1) / kHamTile * kHamTile;
  const int tb = seg * per, te = min(nb, tb + per);
  for (int t0 = tb; t0 < te; t0 += kHamTile) {
    const int nt_tile = min(kHamTile, te - t0);
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(B + (int64_t)t0 * W * 4);
    for (int i = threadIdx.x; i < nt_tile * (W / 4); i += kHamThreads) tile[i] = src[i];
    if (MASKED) {
      const uint4* msrc = reinterpret_cast<const uint4*>(MB + (int64_t)t0 * W * 4);
      for (int i = threadIdx.x; i < nt_tile * (W / 4); i += kHamThreads) mtile[i] = msrc[i];
    }
    for (int i = threadIdx.x; i < nt_tile; i += kHamThreads)
      tcam[i] = hasB[t0 + i] ? -2 : camB[t0 + i];
    __syncthreads();
    if (qc < 0) continue;
    for (int j = 0; j < nt_tile; j++) {
      if (tcam[j] != qc) continue;
      const int d = MASKED ? ham_dist_masked_v<W>(q, qm, &tile[j * (W / 4)], &mtile[j * (W / 4)])
                           : ham_dist_v<W>(q, &tile[j * (W / 4)]);
      if (d <= th) {
        const int i2 = t0 + j;
        if (n < kTriSub) out[n] = ((uint32_t)d << 20) | (uint32_t)i2;
        n++;
        atomicAdd(ref_all + i2, 1);
      }
    }
  }
  if (qi < na) {
    cnt[(int64_t)qi * kTriSeg + seg] = n;
    if (n > kTriSub) atomicOr(overflow, 1);
  }
}

__global__ __launch_bounds__(256) void k_tri_pass(const int32_t* __restrict__ camA,
                                                  const double* __restrict__ raysA, int na,
                                                  const double* __restrict__ raysB, int ncams,
                                                  const double* __restrict__ E, double thresh,
                                                  uint32_t* __restrict__ cand,
                                                  const int32_t* __restrict__ cnt,
                                                  int32_t* __restrict__ ref_pass) {
  const int gt = blockIdx.x * 256 + threadIdx.x;
  if (gt >= na * kTriSeg) return;
  const int n = min(cnt[gt], kTriSub);
  if (n == 0) return;
  const int qi = gt / kTriSeg, qc = camA[qi];
  double r1[3], Em[9];
  for (int k = 0; k < 3; k++) r1[k] = raysA[3 * (int64_t)qi + k];
  // same camera only (:1040-1041): E[cam1][cam2] with cam2 == cam1
  for (int k = 0; k < 9; k++) Em[k] = E[9 * ((int64_t)qc * ncams + qc) + k];
  uint32_t* const ks = cand + (int64_t)gt * kTriSub;
  for (int i = 0; i < n; i++) {
    const uint32_t key = ks[i];
    const int i2 = (int)(key & 0xFFFFFu);
    if (frm::epi_check(r1, raysB + 3 * (int64_t)i2, Em, thresh)) {
      ks[i] = key | kTriPass;
      atomicAdd(ref_pass + i2, 1);
    }
  }
}

__global__ __launch_bounds__(256) void k_tri_private(const uint32_t* __restrict__ cand,
                                                     const int32_t* __restrict__ cnt_in,
                                                     const int32_t* __restrict__ ref_all,
                                                     const int32_t* __restrict__ ref_pass,
                                                     const int32_t* __restrict__ overflow, int na,
                                                     int32_t* __restrict__ m12,
                                                     int32_t* __restrict__ n_matches,
                                                     int32_t* __restrict__ flag,
                                                     int32_t* __restrict__ len) {
  const int qi = blockIdx.x * 256 + threadIdx.x;
  int won = 0;
  if (qi < na) {
    int c = 0;
    bool over = false;
    for (int sg = 0; sg < kTriSeg; sg++) {
      const int n = cnt_in[(int64_t)qi * kTriSeg + sg];
      over = over || n > kTriSub;
      c += n;
    }
    over = over || c > kTriWin;   // k_tri_seq keeps a query's keys inside two LDS windows
    int r = -1, fl = 0, ln = 0;
    if (over) {
      r = -2; fl = 1;   // ln = 0: k_tri_seq rescans
    } else if (c > 0) {
      bool alone = *overflow == 0;
      uint32_t best = 0xFFFFFFFFu;
      for (int sg = 0; sg < kTriSeg; sg++) {
        const uint32_t* k = cand + ((int64_t)qi * kTriSeg + sg) * kTriSub;
        const int n = cnt_in[(int64_t)qi * kTriSeg + sg];
        for (int i = 0; i < n; i++) {
          const uint32_t key = k[i];
          const int i2 = (int)(key & 0xFFFFFu), own = (key & kTriPass) ? 1 : 0;
          best = min(best, key & kTriKey);
          if (own && ref_all[i2] > 1) alone = false;       // it could take a key another lists
          if (ref_pass[i2] - own > 0) alone = false;      // another could take one of its keys
        }
      }
      if (!alone) {
        r = -2; fl = 1; ln = c;
      } else {
        const uint32_t th = 2u * (best >> 20);   // cvRound(2 * bestDist), integer distance
        uint32_t win = 0xFFFFFFFFu;
        for (int sg = 0; sg < kTriSeg; sg++) {
          const uint32_t* k = cand + ((int64_t)qi * kTriSeg + sg) * kTriSub;
          const int n = cnt_in[(int64_t)qi * kTriSeg + sg];
          for (int i = 0; i < n; i++) {
            const uint32_t key = k[i];
            if ((key & kTriPass) && ((key & kTriKey) >> 20) <= th) win = min(win, key & kTriKey);
          }
        }
        if (win != 0xFFFFFFFFu) { r = (int)(win & 0xFFFFFu); won = 1; }
      }
    }
    m12[qi] = r;
    flag[qi] = fl;
    len[qi] = ln;
  } else if (qi == na) {   // the scans' total slot
    flag[qi] = 0;
    len[qi] = 0;
  }
  const int s = dev::wave_sum(won);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(n_matches, s);
}

// one wave per flagged query: its keys (the segments' lists), ascending by (dist, idx2), to
// flat[koff[q] ...); the entry (q, offset, count, camera) at its place pos[q] of the ordered list
__global__ __launch_bounds__(256) void k_tri_gather(const uint32_t* __restrict__ cand,
                                                    const int32_t* __restrict__ cnt_in,
                                                    const int32_t* __restrict__ cam,
                                                    const int32_t* __restrict__ flag,
                                                    const int32_t* __restrict__ len,
                                                    const int32_t* __restrict__ pos,
                                                    const int32_t* __restrict__ koff, int na,
                                                    uint32_t* __restrict__ flat,
                                                    int4* __restrict__ entries) {
  __shared__ uint32_t sk[4][kTriCap];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + wv;
  if (q >= na || !flag[q]) return;
  const int c = len[q], o = koff[q];
  if (lane == 0) entries[pos[q]] = make_int4(q, o, c, cam[q]);
  int at = 0;
  for (int sg = 0; sg < kTriSeg && c > 0; sg++) {
    const int n = cnt_in[(int64_t)q * kTriSeg + sg];
    const uint32_t* src = cand + ((int64_t)q * kTriSeg + sg) * kTriSub;
    for (int i = lane; i < n; i += 64) sk[wv][at + i] = src[i];
    at += n;
  }
  dev::wave_sync();
  for (int i = lane; i < c; i += 64) {   // rank by counting (keys are distinct: idx2 differs)
    const uint32_t key = sk[wv][i], kk = key & kTriKey;
    int rank = 0;
    for (int j = 0; j < c; j++) rank += (sk[wv][j] & kTriKey) < kk;
    flat[o + rank] = key;
  }
}

__device__ __forceinline__ int first_lane(uint64_t m) { return (int)__builtin_ctzll(m); }

// One wave per camera (a query's candidates are KF2 keypoints of its own camera, so cameras
// never share vbMatched2 bits): the wave walks the ordered flagged list, takes its camera's
// entries, and streams their keys through two LDS windows of its own.
template <int W, bool MASKED>
__global__ __launch_bounds__(512) void k_tri_seq(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ MA, const int32_t* __restrict__ camA,
    const double* __restrict__ raysA, const uint8_t* __restrict__ B,
    const uint8_t* __restrict__ MB, const int32_t* __restrict__ camB,
    const uint8_t* __restrict__ hasB, const double* __restrict__ raysB, int na, int nb, int ncams,
    const double* __restrict__ E, int th_low, double thresh, const uint32_t* __restrict__ flat,
    const int4* __restrict__ entries, const int32_t* __restrict__ pos,
    int32_t* __restrict__ m12, int32_t* __restrict__ n_matches) {
  extern __shared__ uint32_t smem[];
  const int cam = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint32_t* const matched2 = smem;                                 // vbMatched2 bitmap, nb bits
  const int nwords = (nb + 31) >> 5;
  uint32_t* const win = smem + ((nwords + 3) & ~3) + cam * 2 * kTriWin;   // this wave's windows
  for (int i = threadIdx.x; i < nwords; i += blockDim.x) matched2[i] = 0u;
  __syncthreads();
  if (cam >= ncams) return;
  const int ns = pos[na];                         // flagged queries
  auto is_matched = [&](uint32_t i2) { return (matched2[i2 >> 5] >> (i2 & 31)) & 1u; };
  constexpr int R = kTriWin / 64;
  uint32_t pre[R];
  auto load_win = [&](int wj, uint32_t (&v)[R]) {
#pragma unroll
    for (int k = 0; k < R; k++) v[k] = flat[(int64_t)wj * kTriWin + 64 * k + lane];
  };
  auto store_win = [&](int wj, const uint32_t (&v)[R]) {
#pragma unroll
    for (int k = 0; k < R; k++) win[(wj & 1) * kTriWin + 64 * k + lane] = v[k];
  };
  // windows cw, cw + 1 are in LDS (slots cw & 1, (cw + 1) & 1), window cw + 2 in flight; the
  // flat array is padded by three windows (workspace), so whole-window loads stay inside it
  int cw = -8;
  auto ensure = [&](int o) {
    const int w0 = o / kTriWin;
    if (w0 == cw) return;
    if (w0 == cw + 1) {
      store_win(cw + 2, pre);
      cw++;
    } else {
      uint32_t v0[R], v1[R];
      load_win(w0, v0);
      load_win(w0 + 1, v1);
      store_win(w0, v0);
      store_win(w0 + 1, v1);
      cw = w0;
    }
    load_win(cw + 2, pre);
    dev::wave_sync();
  };
  auto key_at = [&](int g) { return win[((g / kTriWin) & 1) * kTriWin + (g % kTriWin)]; };
  int nm = 0;
  int4 ent = lane < ns ? entries[lane] : make_int4(0, 0, 0, -1);
  for (int base = 0; base < ns; base += 64) {
    const int4 cur = ent;
    if (base + 64 + lane < ns) ent = entries[base + 64 + lane];   // next chunk's entries
    uint64_t todo = __ballot(base + lane < ns && cur.w == cam);
    while (todo) {
      const int i = first_lane(todo);
      todo &= todo - 1;
      const int q = __builtin_amdgcn_readlane(cur.x, i);
      const int o = __builtin_amdgcn_readlane(cur.y, i);
      const int c = __builtin_amdgcn_readlane(cur.z, i);
      // Two short queries at once, one per 32-lane half, from one key read and one vbMatched2
      // read: the second decides on the first's state plus the first's winner (its bit is
      // cleared from the second's unmatched keys before its own best is taken), which is the
      // sequential order.  Both must lie in the two resident windows.
      if (todo && c > 0 && c <= 32) {
        const int j = first_lane(todo);
        const int c2 = __builtin_amdgcn_readlane(cur.z, j);
        const int o2 = __builtin_amdgcn_readlane(cur.y, j);
        if (c2 > 0 && c2 <= 32 && o2 + c2 - o <= kTriWin) {
          todo &= todo - 1;
          const int q2 = __builtin_amdgcn_readlane(cur.x, j);
          ensure(o);
          const bool hi = lane >= 32;
          const int li = lane & 31;
          const bool valid = li < (hi ? c2 : c);
          const uint32_t key = valid ? key_at((hi ? o2 : o) + li) : 0u;
          const uint32_t kid = key & 0xFFFFFu;
          const bool unm = valid && !is_matched(kid);
          const uint64_t bu = __ballot(unm);
          uint32_t w1 = 0xFFFFFFFFu, w2 = 0xFFFFFFFFu;
          const uint64_t b1 = bu & 0xFFFFFFFFull;
          if (b1) {
            const uint32_t best = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(b1)) & kTriKey;
            const uint32_t th = 2u * (best >> 20);
            const uint64_t bo = __ballot(!hi && unm && (key & kTriPass) && ((key & kTriKey) >> 20) <= th);
            if (bo) w1 = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(bo)) & kTriKey;
          }
          const uint32_t r1k = w1 != 0xFFFFFFFFu ? (w1 & 0xFFFFFu) : 0xFFFFFFFFu;
          const bool unm2 = hi && unm && kid != r1k;
          const uint64_t b2 = __ballot(unm2);
          if (b2) {
            const uint32_t best = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(b2)) & kTriKey;
            const uint32_t th = 2u * (best >> 20);
            const uint64_t bo = __ballot(unm2 && (key & kTriPass) && ((key & kTriKey) >> 20) <= th);
            if (bo) w2 = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(bo)) & kTriKey;
          }
          const int r1 = w1 != 0xFFFFFFFFu ? (int)(w1 & 0xFFFFFu) : -1;
          const int r2 = w2 != 0xFFFFFFFFu ? (int)(w2 & 0xFFFFFu) : -1;
          if (lane == 0) {
            m12[q] = r1;
            m12[q2] = r2;
            if (r1 >= 0) atomicOr(&matched2[r1 >> 5], 1u << (r1 & 31));
            if (r2 >= 0) atomicOr(&matched2[r2 >> 5], 1u << (r2 & 31));
          }
          nm += (r1 >= 0) + (r2 >= 0);
          continue;
        }
      }
      uint32_t wkey = 0xFFFFFFFFu;
      if (c > 0) {
        ensure(o);
        if (c <= 64) {   // one round: best and winner from the same reads
          const bool valid = lane < c;
          const uint32_t key = valid ? key_at(o + lane) : 0u;
          const bool unm = valid && !is_matched(key & 0xFFFFFu);
          const uint64_t bu = __ballot(unm);
          if (bu) {
            const uint32_t best = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(bu)) & kTriKey;
            const uint32_t th = 2u * (best >> 20);
            const uint64_t bo = __ballot(unm && (key & kTriPass) && ((key & kTriKey) >> 20) <= th);
            if (bo) wkey = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(bo)) & kTriKey;
          }
        } else {
          int rb = -1;
          uint32_t best = 0;
          for (int r = 0; r * 64 < c; r++) {
            const bool valid = r * 64 + lane < c;
            const uint32_t key = valid ? key_at(o + r * 64 + lane) : 0u;
            const uint64_t b = __ballot(valid && !is_matched(key & 0xFFFFFu));
            if (b) { best = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(b)) & kTriKey; rb = r; break; }
          }
          if (rb >= 0) {
            const uint32_t th = 2u * (best >> 20);
            for (int r = rb; r * 64 < c; r++) {
              const bool valid = r * 64 + lane < c;
              const uint32_t key = valid ? key_at(o + r * 64 + lane) : 0xFFFFFFFFu;
              const uint32_t d = (key & kTriKey) >> 20;
              const uint64_t b = __ballot(valid && (key & kTriPass) && d <= th && !is_matched(key & 0xFFFFFu));
              if (b) { wkey = (uint32_t)__builtin_amdgcn_readlane((int)key, first_lane(b)) & kTriKey; break; }
              // keys ascend: once a round's last key is past the threshold, no later key qualifies
              if ((((uint32_t)__builtin_amdgcn_readlane((int)key, 63) & kTriKey) >> 20) > th) break;
            }
          }
        }
      } else {
        // more candidates than a slot holds: rescan KF2 for this query (same filters)
        const int qc = camA[q];
        uint32_t qd[W], qmk[W];
        load_desc_row<W>(qd, A + (int64_t)q * W * 4);
        if (MASKED) load_desc_row<W>(qmk, MA + (int64_t)q * W * 4);
        else
          for (int w = 0; w < W; w++) qmk[w] = 0;
        auto dist_to = [&](int i2) {
          uint32_t t[W], tm[W];
          load_desc_row<W>(t, B + (int64_t)i2 * W * 4);
          int d = 0;
          if (MASKED) {
            load_desc_row<W>(tm, MB + (int64_t)i2 * W * 4);
            for (int w = 0; w < W; w++) {
              const uint32_t x = qd[w] ^ t[w];
              d += __popc(x & qmk[w]) + __popc(x & tm[w]);
            }
            d /= 2;
          } else {
            for (int w = 0; w < W; w++) d += __popc(qd[w] ^ t[w]);
          }
          return d;
        };
        uint32_t lbest = 0xFFFFFFFFu;
        for (int i2 = lane; i2 < nb; i2 += 64) {
          if (camB[i2] != qc || hasB[i2] || is_matched((uint32_t)i2)) continue;
          const int d = dist_to(i2);
          if (d <= th_low) lbest = min(lbest, ((uint32_t)d << 20) | (uint32_t)i2);
        }
        const uint32_t best = wave_min_u32(lbest);
        if (best != 0xFFFFFFFFu) {
          const int th = 2 * (int)(best >> 20);
          double r1[3], Em[9];
          for (int k = 0; k < 3; k++) r1[k] = raysA[3 * (int64_t)q + k];
          for (int k = 0; k < 9; k++) Em[k] = E[9 * ((int64_t)qc * ncams + qc) + k];
          uint32_t lw = 0xFFFFFFFFu;
          for (int i2 = lane; i2 < nb; i2 += 64) {
            if (camB[i2] != qc || hasB[i2] || is_matched((uint32_t)i2)) continue;
            const int d = dist_to(i2);
            if (d <= th_low && d <= th && frm::epi_check(r1, raysB + 3 * (int64_t)i2, Em, thresh))
              lw = min(lw, ((uint32_t)d << 20) | (uint32_t)i2);
          }
          wkey = wave_min_u32(lw);
        }
      }
      const int r = wkey != 0xFFFFFFFFu ? (int)(wkey & 0xFFFFFu) : -1;
      if (lane == 0) {
        m12[q] = r;
        // LDS atomics of one wave execute in order with its later LDS reads
        if (r >= 0) atomicOr(&matched2[r >> 5], 1u << (r & 31));
      }
      nm += r >= 0;
    }
  }
  if (lane == 0 && nm) atomicAdd(n_matches, nm);
}

}  // namespace mcs

// Workspace of the device search (sized at creation; reused call after call on one stream).
struct mcs_tri_workspace {
  int device = 0, max_n1 = 0, max_n2 = 0;
  uint32_t* cand = nullptr;     // [max_n1][kTriCap] candidate keys
  uint32_t* flat = nullptr;     // [max_n1 * kTriCap + 3 kTriWin] sorted keys of flagged queries
  int4* entries = nullptr;      // [max_n1] (query, key offset, count)
  int32_t* cnt = nullptr;       // [max_n1][kTriSeg]
  int32_t* overflow = nullptr;  // [1] a (query, segment) overflowed its slots
  int32_t* flag = nullptr;      // [max_n1 + 1]
  int32_t* len = nullptr;       // [max_n1 + 1]
  int32_t* pos = nullptr;       // [max_n1 + 1]
  int32_t* koff = nullptr;      // [max_n1 + 1]
  int32_t* ref_all = nullptr;   // [max_n2]
  int32_t* ref_pass = nullptr;  // [max_n2]
  void* scan_tmp = nullptr; size_t scan_bytes = 0;
};

namespace mcs {

static size_t tri_lds_bytes(int n2, int ncams) {
  return (size_t)ncams * 2 * kTriWin * 4 + (size_t)(((n2 + 31) / 32 + 3) & ~3) * 4;
}

// Device pipeline on device buffers (stream-ordered; no host synchronisation).
static hipError_t tri_run(mcs_tri_workspace* ws, const uint8_t* dA, const uint8_t* dmA, const int32_t* dcA,
                          const uint8_t* dhA, const double* drA, int n1, const uint8_t* dB, const uint8_t* dmB,
                          const int32_t* dcB, const uint8_t* dhB, const double* drB, int n2, int ncams,
                          const double* dE, int bytes, int th_low, double thresh, int32_t* m12,
                          int32_t* nmatch, hipStream_t st) {
  hipError_t e = hipMemsetAsync(nmatch, 0, sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(ws->overflow, 0, sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(ws->ref_all, 0, sizeof(int32_t) * (size_t)n2, st);
  if (e == hipSuccess) e = hipMemsetAsync(ws->ref_pass, 0, sizeof(int32_t) * (size_t)n2, st);
  if (e != hipSuccess) return e;
  const bool masked = dmA != nullptr;
  const dim3 g((n1 + kHamThreads - 1) / kHamThreads, kTriSeg);
#define MCS_TRI_RADIUS(WW, MM)                                                                   \
  hipLaunchKernelGGL((k_tri_radius<WW, MM>), g, dim3(kHamThreads), 0, st, dA, dmA, dcA, dhA, n1, dB,  \
                     dmB, dcB, dhB, n2, ncams, th_low, ws->cand, ws->cnt, ws->ref_all, ws->overflow)
  if (bytes == 16) { if (masked) MCS_TRI_RADIUS(4, true); else MCS_TRI_RADIUS(4, false); }
  else if (bytes == 32) { if (masked) MCS_TRI_RADIUS(8, true); else MCS_TRI_RADIUS(8, false); }
  else { if (masked) MCS_TRI_RADIUS(16, true); else MCS_TRI_RADIUS(16, false); }
#undef MCS_TRI_RADIUS
  hipLaunchKernelGGL(k_tri_pass, dim3((n1 * kTriSeg + 255) / 256), dim3(256), 0, st, dcA, drA, n1, drB, ncams, dE,
                     thresh, ws->cand, ws->cnt, ws->ref_pass);
  hipLaunchKernelGGL(k_tri_private, dim3((n1 + 1 + 255) / 256), dim3(256), 0, st, ws->cand, ws->cnt, ws->ref_all,
                     ws->ref_pass, ws->overflow, n1, m12, nmatch, ws->flag, ws->len);
  auto plus = rocprim::plus<int32_t>();
  size_t b1 = ws->scan_bytes;
  if ((e = rocprim::exclusive_scan(ws->scan_tmp, b1, ws->flag, ws->pos, 0, (size_t)n1 + 1, plus, st)) != hipSuccess)
    return e;
  b1 = ws->scan_bytes;
  if ((e = rocprim::exclusive_scan(ws->scan_tmp, b1, ws->len, ws->koff, 0, (size_t)n1 + 1, plus, st)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_tri_gather, dim3((n1 + 3) / 4), dim3(256), 0, st, ws->cand, ws->cnt, dcA, ws->flag, ws->len, ws->pos,
                     ws->koff, n1, ws->flat, ws->entries);
  const int lds = (int)tri_lds_bytes(n2, ncams);
  if (ncams > 8 || lds > 160 * 1024) return hipErrorInvalidValue;   // entry points check first
  const void* fn = nullptr;
#define MCS_TRI_SEQ_FN(WW, MM) fn = (const void*)&k_tri_seq<WW, MM>
  if (bytes == 16) { if (masked) MCS_TRI_SEQ_FN(4, true); else MCS_TRI_SEQ_FN(4, false); }
  else if (bytes == 32) { if (masked) MCS_TRI_SEQ_FN(8, true); else MCS_TRI_SEQ_FN(8, false); }
  else { if (masked) MCS_TRI_SEQ_FN(16, true); else MCS_TRI_SEQ_FN(16, false); }
#undef MCS_TRI_SEQ_FN
  if (lds > 64 * 1024 && (e = ldlt::set_lds_limit(fn, lds)) != hipSuccess) return e;
#define MCS_TRI_SEQ(WW, MM)                                                                       \
  hipLaunchKernelGGL((k_tri_seq<WW, MM>), dim3(1), dim3(64 * ncams), lds, st, dA, dmA, dcA, drA, dB, dmB, dcB, \
                     dhB, drB, n1, n2, ncams, dE, th_low, thresh, ws->flat, ws->entries, ws->pos, m12, \
                     nmatch)
  if (bytes == 16) { if (masked) MCS_TRI_SEQ(4, true); else MCS_TRI_SEQ(4, false); }
  else if (bytes == 32) { if (masked) MCS_TRI_SEQ(8, true); else MCS_TRI_SEQ(8, false); }
  else { if (masked) MCS_TRI_SEQ(16, true); else MCS_TRI_SEQ(16, false); }
#undef MCS_TRI_SEQ
  return hipGetLastError();
}

static int search_for_triangulation(const uint8_t* desc1, const uint8_t* mask1,
                                    const int32_t* cam1, const uint8_t* has_mp1,
                                    const double* rays1, int32_t n1, const uint8_t* desc2,
                                    const uint8_t* mask2, const int32_t* cam2,
                                    const uint8_t* has_mp2, const double* rays2, int32_t n2,
                                    int32_t ncams, const double* E, int32_t bytes, int32_t th_low,
                                    double epi_thresh, int32_t* matches12, int32_t* n_matches) {
  int rc = host::check_desc_bytes(bytes, "matcher");
  if (rc) return rc;
  if (!n_matches || (n1 > 0 && !matches12)) return MCS_ERR_ARG;
  *n_matches = 0;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  if (n1 <= 0 || n2 <= 0) return MCS_OK;
  // candidates are packed (dist << 20 | idx2): train index must fit 20 bits
  if (n2 >= (1 << 19)) { set_error("triangulation: at most 2^19 - 1 keypoints in KF2"); return MCS_ERR_ARG; }
  if (!desc1 || !desc2 || !cam1 || !cam2 || !has_mp1 || !has_mp2 || !rays1 || !rays2 || !E ||
      ncams <= 0)
    return MCS_ERR_ARG;
  if (ncams > 8) { set_error("triangulation: at most 8 cameras (one ordered-pass wave each)"); return MCS_ERR_UNSUPPORTED; }
  const bool masked = mask1 != nullptr;
  if (masked != (mask2 != nullptr)) { set_error("triangulation: masks for both keyframes or none"); return MCS_ERR_ARG; }
  for (int i = 0; i < n1; i++)
    if (cam1[i] < 0 || cam1[i] >= ncams) { set_error("triangulation: cam1 out of range"); return MCS_ERR_ARG; }
  for (int i = 0; i < n2; i++)
    if (cam2[i] < 0 || cam2[i] >= ncams) { set_error("triangulation: cam2 out of range"); return MCS_ERR_ARG; }
  int ndev = 0;
  if ((rc = host::have_device(&ndev))) return rc;
  // host entry: upload, run the device search, download (one synchronisation)
  host::DevBufs B;
  const size_t s1 = (size_t)n1, s2 = (size_t)n2;
  const uint8_t* dA = B.up(desc1, s1 * bytes);
  const uint8_t* dB = B.up(desc2, s2 * bytes);
  const uint8_t* dmA = B.up(mask1, s1 * bytes);
  const uint8_t* dmB = B.up(mask2, s2 * bytes);
  const uint8_t* dhA = B.up(has_mp1, s1);
  const uint8_t* dhB = B.up(has_mp2, s2);
  const int32_t* dcA = B.up(cam1, s1);
  const int32_t* dcB = B.up(cam2, s2);
  const double* drA = B.up(rays1, 3 * s1);
  const double* drB = B.up(rays2, 3 * s2);
  const double* dE = B.up(E, 9 * (size_t)ncams * ncams);
  int32_t* dm12 = B.alloc<int32_t>(s1);
  int32_t* dn = B.alloc<int32_t>(1);
  hipError_t& e = B.err;
  int dev = 0;
  if (e == hipSuccess) e = hipGetDevice(&dev);
  {
    // one workspace per device, kept for the process and grown on demand (a call holds the
    // lock for its whole run: calls on one device share the buffers)
    static std::mutex mu;
    static std::map<int, mcs_tri_workspace*> cache;
    std::lock_guard<std::mutex> g(mu);
    mcs_tri_workspace*& ws = cache[dev];
    if (e == hipSuccess && (!ws || ws->max_n1 < n1 || ws->max_n2 < n2)) {
      const int32_t g1 = ws ? std::max(ws->max_n1, n1) : n1, g2 = ws ? std::max(ws->max_n2, n2) : n2;
      if (ws) { mcs_tri_workspace_destroy(ws); ws = nullptr; }
      if ((rc = mcs_tri_workspace_create(dev, g1, g2, &ws)) != MCS_OK) { ws = nullptr; e = hipErrorOutOfMemory; }
    }
    if (e == hipSuccess)
      e = tri_run(ws, dA, dmA, dcA, dhA, drA, n1, dB, dmB, dcB, dhB, drB, n2, ncams, dE, bytes, th_low,
                  epi_thresh, dm12, dn, nullptr);
    B.down(matches12, dm12, s1);
    B.down(n_matches, dn, 1);
  }
  if (e != hipSuccess) {
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    *n_matches = 0;
    set_hip_error(e, "triangulation search", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  return MCS_OK;
}

}  // namespace mcs

using namespace mcs;

extern "C" {

int mcs_search_for_triangulation_raw(const uint8_t* desc1, const int32_t* cam1,
                                     const uint8_t* has_mp1, const double* rays1, int32_t n1,
                                     const uint8_t* desc2, const int32_t* cam2,
                                     const uint8_t* has_mp2, const double* rays2, int32_t n2,
                                     int32_t ncams, const double* E, int32_t bytes,
                                     int32_t th_low, double epi_thresh, int32_t* matches12,
                                     int32_t* n_matches) {
  return search_for_triangulation(desc1, nullptr, cam1, has_mp1, rays1, n1, desc2, nullptr, cam2,
                                  has_mp2, rays2, n2, ncams, E, bytes, th_low, epi_thresh,
                                  matches12, n_matches);
}

int mcs_search_for_triangulation_raw_masked(const uint8_t* desc1, const uint8_t* mask1,
                                            const int32_t* cam1, const uint8_t* has_mp1,
                                            const double* rays1, int32_t n1,
                                            const uint8_t* desc2, const uint8_t* mask2,
                                            const int32_t* cam2, const uint8_t* has_mp2,
                                            const double* rays2, int32_t n2, int32_t ncams,
                                            const double* E, int32_t bytes, int32_t th_low,
                                            double epi_thresh, int32_t* matches12,
                                            int32_t* n_matches) {
  if (!mask1 || !mask2) { set_error("triangulation: masked entry needs both masks"); return MCS_ERR_ARG; }
  return search_for_triangulation(desc1, mask1, cam1, has_mp1, rays1, n1, desc2, mask2, cam2,
                                  has_mp2, rays2, n2, ncams, E, bytes, th_low, epi_thresh,
                                  matches12, n_matches);
}

int mcs_tri_workspace_create(int32_t device, int32_t max_n1, int32_t max_n2, mcs_tri_workspace** out) {
  if (!out || max_n1 < 1 || max_n2 < 1 || max_n2 >= (1 << 19)) {
    set_error("tri workspace: need max_n1 >= 1 and 1 <= max_n2 < 2^19");
    return MCS_ERR_ARG;
  }
  *out = nullptr;
  if (int rc = host::open_device(device, "tri workspace")) return rc;
  auto* w = new (std::nothrow) mcs_tri_workspace();
  if (!w) return MCS_ERR_ARG;
  w->device = device; w->max_n1 = max_n1; w->max_n2 = max_n2;
  const size_t n1 = (size_t)max_n1, n2 = (size_t)max_n2;
  hipError_t e = hipMalloc((void**)&w->cand, 4 * n1 * kTriCap);
  if (e == hipSuccess) e = hipMalloc((void**)&w->flat, 4 * (n1 * kTriCap + 3 * kTriWin));
  if (e == hipSuccess) e = hipMalloc((void**)&w->entries, sizeof(int4) * n1);
  if (e == hipSuccess) e = hipMalloc((void**)&w->cnt, 4 * n1 * kTriSeg);
  if (e == hipSuccess) e = hipMalloc((void**)&w->overflow, 4);
  if (e == hipSuccess) e = hipMalloc((void**)&w->flag, 4 * (n1 + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->len, 4 * (n1 + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->pos, 4 * (n1 + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->koff, 4 * (n1 + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->ref_all, 4 * n2);
  if (e == hipSuccess) e = hipMalloc((void**)&w->ref_pass, 4 * n2);
  if (e == hipSuccess)
    e = rocprim::exclusive_scan(nullptr, w->scan_bytes, w->flag, w->pos, 0, n1 + 1, rocprim::plus<int32_t>(),
                                (hipStream_t)0);
  if (e == hipSuccess) e = hipMalloc(&w->scan_tmp, std::max<size_t>(16, w->scan_bytes));
  if (e != hipSuccess) {
    mcs_tri_workspace_destroy(w);
    set_hip_error(e, "tri workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_tri_workspace_destroy(mcs_tri_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  void* bufs[] = {w->cand, w->flat, w->entries, w->cnt, w->overflow, w->flag, w->len, w->pos, w->koff, w->ref_all,
                  w->ref_pass, w->scan_tmp};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  delete w;
}

int mcs_search_for_triangulation_raw_device(mcs_tri_workspace* ws, const uint8_t* d_desc1,
                                            const uint8_t* d_mask1, const int32_t* d_cam1,
                                            const uint8_t* d_has_mp1, const double* d_rays1,
                                            int32_t n1, const uint8_t* d_desc2,
                                            const uint8_t* d_mask2, const int32_t* d_cam2,
                                            const uint8_t* d_has_mp2, const double* d_rays2,
                                            int32_t n2, int32_t ncams, const double* d_E,
                                            int32_t bytes, int32_t th_low, double epi_thresh,
                                            int32_t* d_matches12, int32_t* d_n_matches,
                                            void* stream) {
  int rc = host::check_desc_bytes(bytes, "matcher");
  if (rc) return rc;
  if (!ws || !d_n_matches || n1 < 0 || n2 < 0 || ncams <= 0) { set_error("triangulation: bad arguments"); return MCS_ERR_ARG; }
  if (n1 > ws->max_n1 || n2 > ws->max_n2) { set_error("triangulation: n1 / n2 above the workspace capacity"); return MCS_ERR_CAPACITY; }
  if (ncams > 8) { set_error("triangulation: at most 8 cameras (one ordered-pass wave each)"); return MCS_ERR_UNSUPPORTED; }
  if ((d_mask1 != nullptr) != (d_mask2 != nullptr)) { set_error("triangulation: masks for both keyframes or none"); return MCS_ERR_ARG; }
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  if (n1 == 0 || n2 == 0) {
    if (n1 > 0) MCS_HIP_CHECK(hipMemsetAsync(d_matches12, 0xFF, 4 * (size_t)n1, st));   // -1
    MCS_HIP_CHECK(hipMemsetAsync(d_n_matches, 0, 4, st));
    return MCS_OK;
  }
  if (!d_desc1 || !d_desc2 || !d_cam1 || !d_cam2 || !d_has_mp1 || !d_has_mp2 || !d_rays1 ||
      !d_rays2 || !d_E || !d_matches12) {
    set_error("triangulation: null device buffer");
    return MCS_ERR_ARG;
  }
  const hipError_t e = tri_run(ws, d_desc1, d_mask1, d_cam1, d_has_mp1, d_rays1, n1, d_desc2, d_mask2, d_cam2,
                               d_has_mp2, d_rays2, n2, ncams, d_E, bytes, th_low, epi_thresh, d_matches12,
                               d_n_matches, st);
  if (e != hipSuccess) { set_hip_error(e, "triangulation search", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
