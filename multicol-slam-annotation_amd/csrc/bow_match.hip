// SearchByBoW on gfx950: relocalisation (keyframe -> frame, by vocabulary node) and loop
// detection (keyframe -> keyframe, brute force), one frame against a batch of candidates.
//
// Reference: SearchByBoW(cMultiKeyFrame*, cMultiFrame&, ...)      src/cORBmatcher.cpp:179-323
//            SearchByBoW(cMultiKeyFrame*, cMultiKeyFrame*, ...)   src/cORBmatcher.cpp:885-966
//            ComputeThreeMaxima                                   src/cORBmatcher.cpp:2399-2441
//            TemplatedVocabulary::transform (FeatureVector part)  TemplatedVocabulary.h:1126-1196
#include "host_util.hpp"
#include "ham_dist.hpp"
#include "../../include/mcs_matcher.h"
#include "../../include/mcs_vocab.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cmath>
#include <new>
#include <vector>

namespace mcs {

constexpr uint32_t kNone = 0xFFFFFFFFu;       // "no candidate" key / INT_MAX distance
constexpr int kIdxBits = 20;                  // keys are (dist << 20 | position): dist <= 512
constexpr uint32_t kIdxMask = (1u << kIdxBits) - 1;
constexpr int kBowMaxKp = 1 << 19;            // keypoints per set (positions fit kIdxBits)
constexpr int kHisto = 30;                    // cORBmatcher::HISTO_LENGTH (:44)

// One frame of a packed set.  Offsets, node counts and CSR ranges come from device memory the
// caller filled: everything is clamped into the set, so a malformed set reads no byte outside
// the buffers the header describes.
struct FrameView {
  int n, fv_n;
  const uint8_t* desc; const uint8_t* mask; const float* angle; const uint8_t* has_mp;
  const uint32_t* fv_node; const int32_t* fv_ptr; const uint32_t* fv_feat;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ FrameView frame_view(const mcs_bow_set& s, int k, int bytes, bool fv) {
  FrameView v;
  const int o0 = clampi(s.off[k], 0, s.n_kp_total), o1 = clampi(s.off[k + 1], o0, s.n_kp_total);
  v.n = o1 - o0;
  v.desc = s.desc + (int64_t)o0 * bytes;
  v.mask = s.mask ? s.mask + (int64_t)o0 * bytes : nullptr;
  v.angle = s.angle ? s.angle + o0 : nullptr;
  v.has_mp = s.has_mp ? s.has_mp + o0 : nullptr;
  v.fv_n = 0; v.fv_node = nullptr; v.fv_ptr = nullptr; v.fv_feat = nullptr;
  if (fv) {
    v.fv_node = s.fv_node + o0;
    v.fv_ptr = s.fv_ptr + o0 + k;
    v.fv_feat = s.fv_feat + o0;
    v.fv_n = clampi(s.fv_n[k], 0, v.n);
  }
  return v;
}

template <int W, bool MASKED>
__device__ __forceinline__ int dist_rr(const uint32_t (&a)[W], const uint32_t (&am)[W],
                                       const uint32_t (&b)[W], const uint32_t (&bm)[W]) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < W; w++) {
    const uint32_t x = a[w] ^ b[w];
    if (MASKED) d += __popc(x & am[w]) + __popc(x & bm[w]);   // :2466-2474
    else d += __popc(x);
  }
  return MASKED ? (d >> 1) : d;                               // :2477
}

// Running best key / second-best distance of one lane (:252-261 restated on keys: strict <
// with ascending positions is "smallest (dist, position) key", the second-best counts
// multiplicity).
__device__ __forceinline__ void top2_update(uint32_t key, uint32_t& k1, uint32_t& d2) {
  if (key < k1) {
    if (k1 != kNone) d2 = min(d2, k1 >> kIdxBits);
    k1 = key;
  } else {
    d2 = min(d2, key >> kIdxBits);
  }
}

// The wave's best key and the second-best distance over every entry but the best one.
__device__ __forceinline__ uint32_t top2_reduce(uint32_t k1, uint32_t d2, int* best2) {
  const uint32_t best = wave_min_u32(k1);
  const uint32_t mine = (k1 == best) ? d2 : (k1 == kNone ? kNone : (k1 >> kIdxBits));
  const uint32_t sec = wave_min_u32(mine);
  *best2 = sec == kNone ? INT_MAX : (int)sec;
  return best;
}

// :274-279.  rot * factor is a float product rounded half to even by cvRound; the factor is
// 1.0f / HISTO_LENGTH (so only bins 0..12 fill).  Angles are cv::KeyPoint angles in [0, 360);
// anything else would index outside rotHist in the reference and is clamped here.
__device__ __forceinline__ int ori_bin(float a_kf, float a_f) {
  float rot = a_kf - a_f;
  if (rot < 0.0f) rot += 360.0f;
  const float factor = 1.0f / (float)kHisto;
  int bin = __float2int_rn(rot * factor);
  if (bin == kHisto) bin = 0;
  return clampi(bin, 0, kHisto - 1);
}

// ---- overload A: one wave per (candidate keyframe, F node)
// The greedy dependency of :203-300 lives inside one vocabulary node (a keypoint belongs to
// one node), so nodes and candidates run in parallel and one wave walks a node's KF keypoints
// in list order.  Lanes own the node's F entries (entry e -> lane e % 64; the first kBowRegs
// entries of a lane stay in VGPRs, longer nodes re-read theirs); "not yet assigned in this call"
// (:237) is the match row itself, read and written only by the entry's owner lane.
constexpr int kBowRegs = 2;

template <int W, bool MASKED>
__global__ __launch_bounds__(256) void k_bow_node(mcs_bow_set f, mcs_bow_set kfs, int th_low,
                                                  double nnratio, int check_ori, int32_t* match_f,
                                                  int32_t* n_matches, int32_t* hist) {
  const int lane = dev::lane_id();
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), k = blockIdx.y;
  const FrameView F = frame_view(f, 0, W * 4, true);
  if (j >= F.fv_n) return;
  const FrameView K = frame_view(kfs, k, W * 4, true);
  const uint32_t node = F.fv_node[j];
  int lo = 0, hi = K.fv_n;                       // the node's entry in the keyframe (:292-299)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (K.fv_node[mid] < node) lo = mid + 1; else hi = mid;
  }
  if (lo >= K.fv_n || K.fv_node[lo] != node) return;
  const int fb = clampi(F.fv_ptr[j], 0, F.n), fe = clampi(F.fv_ptr[j + 1], fb, F.n);
  const int kb = clampi(K.fv_ptr[lo], 0, K.n), ke = clampi(K.fv_ptr[lo + 1], kb, K.n);
  const int nf = fe - fb;
  int32_t* const mrow = match_f + (int64_t)k * f.n_kp_total;

  uint32_t cd[kBowRegs][W], cm[kBowRegs][W];
  int cf[kBowRegs];
#pragma unroll
  for (int c = 0; c < kBowRegs; c++) {
    cf[c] = -1;
#pragma unroll
    for (int w = 0; w < W; w++) { cd[c][w] = 0; cm[c][w] = 0; }
    const int e = lane + 64 * c;
    if (e < nf) {
      const uint32_t fi = F.fv_feat[fb + e];
      if (fi < (uint32_t)F.n) {
        cf[c] = (int)fi;
        load_desc_row<W>(cd[c], F.desc + (int64_t)fi * W * 4);
        if (MASKED) load_desc_row<W>(cm[c], F.mask + (int64_t)fi * W * 4);
      }
    }
  }
  int cnt = 0;
  for (int iq = kb; iq < ke; iq++) {
    const uint32_t kidx = K.fv_feat[iq];
    if (kidx >= (uint32_t)K.n || !K.has_mp[kidx]) continue;      // :214-220
    uint32_t q[W], qm[W];
    load_desc_row<W>(q, K.desc + (int64_t)kidx * W * 4);
    if (MASKED) load_desc_row<W>(qm, K.mask + (int64_t)kidx * W * 4);
    else {
#pragma unroll
      for (int w = 0; w < W; w++) qm[w] = 0;
    }
    uint32_t k1 = kNone, d2 = kNone;
#pragma unroll
    for (int c = 0; c < kBowRegs; c++)
      if (cf[c] >= 0) {
        const uint32_t d = (uint32_t)dist_rr<W, MASKED>(q, qm, cd[c], cm[c]);
        top2_update((d << kIdxBits) | (uint32_t)(lane + 64 * c), k1, d2);
      }
    for (int e = lane + 64 * kBowRegs; e < nf; e += 64) {
      const uint32_t fi = F.fv_feat[fb + e];
      if (fi >= (uint32_t)F.n || mrow[fi] >= 0) continue;        // :237
      uint32_t t[W], tm[W];
      load_desc_row<W>(t, F.desc + (int64_t)fi * W * 4);
      if (MASKED) load_desc_row<W>(tm, F.mask + (int64_t)fi * W * 4);
      else {
#pragma unroll
        for (int w = 0; w < W; w++) tm[w] = 0;
      }
      const uint32_t d = (uint32_t)dist_rr<W, MASKED>(q, qm, t, tm);
      top2_update((d << kIdxBits) | (uint32_t)e, k1, d2);
    }
    int best2;
    const uint32_t best = top2_reduce(k1, d2, &best2);
    if (best == kNone) continue;
    const int bd = (int)(best >> kIdxBits);
    if (bd <= th_low && (double)bd < nnratio * (double)best2) {   // :264-266
      const uint32_t pos = best & kIdxMask;
      const uint32_t fi = F.fv_feat[fb + pos];
      if (k1 == best) {
        mrow[fi] = (int32_t)kidx;                                 // :268
#pragma unroll
        for (int c = 0; c < kBowRegs; c++)
          if (pos == (uint32_t)(lane + 64 * c)) cf[c] = -1;
      }
      if (check_ori && lane == 0)                                 // :272-282, counts only
        atomicAdd(hist + k * kHisto + ori_bin(K.angle[kidx], F.angle[fi]), 1);
      cnt++;
    }
  }
  if (lane == 0 && cnt) atomicAdd(n_matches + k, cnt);
}

// ComputeThreeMaxima (:2399-2441) over one keyframe's bin counts: strict >, the 0.1f rule.
__global__ void k_bow_maxima(const int32_t* __restrict__ hist, int32_t* __restrict__ keep, int n_kf) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_kf) return;
  int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
  for (int i = 0; i < kHisto; i++) {
    const int s = hist[k * kHisto + i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
  keep[3 * k] = ind1; keep[3 * k + 1] = ind2; keep[3 * k + 2] = ind3;
}

// :311-320: matches whose bin was not kept are removed (after the walk: they did block later
// keyframe keypoints).  The bin is recomputed from the same two angles.
__global__ __launch_bounds__(256) void k_bow_prune(mcs_bow_set f, mcs_bow_set kfs, int bytes,
                                                   const int32_t* __restrict__ keep,
                                                   int32_t* match_f, int32_t* n_matches) {
  const int k = blockIdx.y;
  const FrameView F = frame_view(f, 0, bytes, false);
  const int fi = blockIdx.x * 256 + threadIdx.x;
  if (fi >= F.n) return;
  const FrameView K = frame_view(kfs, k, bytes, false);
  int32_t* const mrow = match_f + (int64_t)k * f.n_kp_total;
  const int m = mrow[fi];
  if (m < 0 || m >= K.n) return;
  const int bin = ori_bin(K.angle[m], F.angle[fi]);
  if (bin == keep[3 * k] || bin == keep[3 * k + 1] || bin == keep[3 * k + 2]) return;
  mrow[fi] = -1;
  atomicSub(n_matches + k, 1);
}

// ---- overload B: parallel candidate pass + one ordered pass per candidate keyframe
// The order dependency (vbMatched2, :924 / :958) is global, so as for SearchForTriangulationRaw
// a parallel pass lists per query the KF2 keypoints that can matter and one wave per candidate
// then walks KF1 in index order against an LDS vbMatched2 bitmap.  What can matter: a query is
// accepted only with best <= th_low - 1, and then its second-best decides only when
// nnratio * second <= best, i.e. second <= (th_low - 1) / nnratio.  With every KF2 keypoint of
// dist <= bound = floor((th_low - 1) / nnratio) + 1 listed (the + 1 keeps the rounding of the
// division on the safe side), fewer than two free entries in the list mean the true second-best
// lies above the bound and the ratio test passes.  A (query, segment) that overflows its slots
// sends the query to an exact rescan of KF2 in the ordered pass.
constexpr int kBowSeg = 8;                    // KF2 segments of the candidate pass (grid.y)
constexpr int kBowSub = 16;                   // slots per (query, segment)
constexpr int kBowCap = kBowSeg * kBowSub;    // per query: two slots per lane of the ordered pass
constexpr int kBowTile = 256;

template <int W, bool MASKED>
__global__ __launch_bounds__(256) void k_bowkf_cand(mcs_bow_set a, mcs_bow_set b, int bound,
                                                    uint32_t* __restrict__ cand,
                                                    int32_t* __restrict__ cnt) {
  __shared__ uint4 tile[kBowTile * (W / 4)];
  __shared__ uint4 mtile[MASKED ? kBowTile * (W / 4) : 1];
  __shared__ uint8_t thas[kBowTile];
  const int k = blockIdx.z, seg = blockIdx.y;
  const int qi = blockIdx.x * 256 + threadIdx.x;
  const FrameView A = frame_view(a, 0, W * 4, false), B = frame_view(b, k, W * 4, false);
  const bool active = qi < A.n && A.has_mp[qi];                 // :903-907
  uint32_t q[W], qm[W];
#pragma unroll
  for (int w = 0; w < W; w++) { q[w] = 0; qm[w] = 0; }
  if (active) {
    load_desc_row<W>(q, A.desc + (int64_t)qi * W * 4);
    if (MASKED) load_desc_row<W>(qm, A.mask + (int64_t)qi * W * 4);
  }
  const int64_t row = (int64_t)k * a.n_kp_total + (qi < A.n ? qi : 0);
  uint32_t* const out = cand + (row * kBowSeg + seg) * kBowSub;
  int n = 0;
  const int per = ((B.n + kBowSeg - 1) / kBowSeg + kBowTile - 1) / kBowTile * kBowTile;
  const int tb = min(B.n, seg * per), te = min(B.n, tb + per);
  for (int t0 = tb; t0 < te; t0 += kBowTile) {
    const int nt = min(kBowTile, te - t0);
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(B.desc + (int64_t)t0 * W * 4);
    for (int i = threadIdx.x; i < nt * (W / 4); i += 256) tile[i] = src[i];
    if (MASKED) {
      const uint4* msrc = reinterpret_cast<const uint4*>(B.mask + (int64_t)t0 * W * 4);
      for (int i = threadIdx.x; i < nt * (W / 4); i += 256) mtile[i] = msrc[i];
    }
    for (int i = threadIdx.x; i < nt; i += 256) thas[i] = B.has_mp[t0 + i];
    __syncthreads();
    if (!active) continue;
    for (int jj = 0; jj < nt; jj++) {
      if (!thas[jj]) continue;                                  // :924-927
      const int d = MASKED ? ham_dist_masked_v<W>(q, qm, &tile[jj * (W / 4)], &mtile[jj * (W / 4)])
                           : ham_dist_v<W>(q, &tile[jj * (W / 4)]);
      if (d <= bound) {
        if (n < kBowSub) out[n] = ((uint32_t)d << kIdxBits) | (uint32_t)(t0 + jj);
        n++;
      }
    }
  }
  if (qi < A.n) cnt[row * kBowSeg + seg] = n;
}

template <int W, bool MASKED>
__global__ __launch_bounds__(64) void k_bowkf_seq(mcs_bow_set a, mcs_bow_set b, int th_low,
                                                  double nnratio, const uint32_t* __restrict__ cand,
                                                  const int32_t* __restrict__ cnt,
                                                  int32_t* __restrict__ matches12,
                                                  int32_t* __restrict__ n_matches) {
  extern __shared__ uint32_t taken[];                           // vbMatched2 (:897)
  const int k = blockIdx.x, lane = dev::lane_id();
  const FrameView A = frame_view(a, 0, W * 4, false), B = frame_view(b, k, W * 4, false);
  for (int i = lane; i < (B.n + 31) / 32; i += 64) taken[i] = 0;
  dev::wave_sync();
  const int64_t row0 = (int64_t)k * a.n_kp_total;
  int32_t* const mrow = matches12 + row0;
  int nm = 0;
  // the next query's flag and slot counts are requested one query ahead
  int has_next = A.n > 0 ? A.has_mp[0] : 0;
  int cl_next = (A.n > 0 && lane < kBowSeg) ? cnt[row0 * kBowSeg + lane] : 0;
  for (int i1 = 0; i1 < A.n; i1++) {
    const int has = has_next, cl = cl_next;
    if (i1 + 1 < A.n) {
      has_next = A.has_mp[i1 + 1];
      cl_next = lane < kBowSeg ? cnt[(row0 + i1 + 1) * kBowSeg + lane] : 0;
    }
    int res = -1;
    if (has) {
      const bool over = __ballot(cl > kBowSub) != 0;
      const bool any = __ballot(cl > 0) != 0;
      uint32_t k1 = kNone, d2 = kNone;
      if (over) {                                               // exact rescan (:920-950)
        uint32_t q[W], qm[W];
        load_desc_row<W>(q, A.desc + (int64_t)i1 * W * 4);
        if (MASKED) load_desc_row<W>(qm, A.mask + (int64_t)i1 * W * 4);
        else {
#pragma unroll
          for (int w = 0; w < W; w++) qm[w] = 0;
        }
        for (int i2 = lane; i2 < B.n; i2 += 64) {
          if (!B.has_mp[i2] || ((taken[i2 >> 5] >> (i2 & 31)) & 1)) continue;
          uint32_t t[W], tm[W];
          load_desc_row<W>(t, B.desc + (int64_t)i2 * W * 4);
          if (MASKED) load_desc_row<W>(tm, B.mask + (int64_t)i2 * W * 4);
          else {
#pragma unroll
            for (int w = 0; w < W; w++) tm[w] = 0;
          }
          const uint32_t d = (uint32_t)dist_rr<W, MASKED>(q, qm, t, tm);
          top2_update((d << kIdxBits) | (uint32_t)i2, k1, d2);
        }
      } else if (any) {
        const uint32_t* keys = cand + (row0 + i1) * kBowCap;
#pragma unroll
        for (int s = 0; s < kBowCap / 64; s++) {
          const int slot = lane + 64 * s;
          const int cs = __shfl(cl, slot / kBowSub, 64);
          if (slot % kBowSub < cs) {
            const uint32_t key = keys[slot];
            const uint32_t i2 = key & kIdxMask;
            if (!((taken[i2 >> 5] >> (i2 & 31)) & 1)) top2_update(key, k1, d2);
          }
        }
      }
      if (over || any) {
        int best2;
        const uint32_t best = top2_reduce(k1, d2, &best2);
        const int bd = (int)(best >> kIdxBits);
        if (best != kNone && bd < th_low && (double)bd < nnratio * (double)best2) {   // :952-955
          const uint32_t i2 = best & kIdxMask;
          if (lane == 0) taken[i2 >> 5] |= 1u << (i2 & 31);      // :958
          dev::wave_sync();
          res = (int)i2;
          nm++;
        }
      }
    }
    if (lane == 0) mrow[i1] = res;
  }
  if (lane == 0) n_matches[k] = nm;
}

// ---- device FeatureVector: (node, weight) per descriptor -> CSR by ascending node
__global__ void k_fv_keys(const uint32_t* __restrict__ node, const double* __restrict__ weight, int n,
                          uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = weight[i] > 0.0 ? node[i] : kNone;   // stopped words sort behind every node and drop
  val[i] = (uint32_t)i;
}

// ---- device BowVector: (word, weight) per descriptor -> ascending unique words with values.
// The words go through the FeatureVector's sort / flag / scan / emit (word in place of node:
// seg[j] .. seg[j+1] are the descriptors of word j in feature order); the values follow
// mcs_vocab_transform's evaluation order to the bit.
// addWeight (TF_IDF / TF): the first weight, then one `+= w` per further occurrence, in feature
// order -- not count * w.  addIfNotExist (IDF / BINARY): the first weight.
__global__ void k_bow_values(const int32_t* __restrict__ seg, const uint32_t* __restrict__ feat,
                             const double* __restrict__ weight, const int32_t* __restrict__ bow_n, int n,
                             int tf, double* __restrict__ value) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(*bow_n, n)) return;
  const int b = max(seg[j], 0), e = min(seg[j + 1], n);
  if (b >= e) { value[j] = 0.0; return; }
  double v = weight[feat[b]];
  if (tf)
    for (int i = b + 1; i < e; i++) v += weight[feat[i]];
  value[j] = v;
}

// BowVector::normalize (BowVector.cpp:66-86) / the TF division of transform (:1166-1172).  The
// norm is the serial sum in ascending word order that std::map iteration gives the reference: ONE
// lane adds the values one after the other, from LDS chunks the block stages.  This is deliberate:
// a tree reduction would be faster and would change the last bits of every value.
constexpr int kBowNormChunk = 2048;
__global__ __launch_bounds__(256) void k_bow_normalize(const int32_t* __restrict__ bow_n, int n, int mode,
                                                      double* __restrict__ value) {
  __shared__ double s_v[kBowNormChunk];
  __shared__ double s_norm;
  const int m = min(max(*bow_n, 0), n);
  if (mode == 0 || m == 0) return;
  if (mode == 3) {   // TF weighting without a normalising scoring: v /= size
    const double nd = (double)m;
    for (int i = threadIdx.x; i < m; i += 256) value[i] /= nd;
    return;
  }
  double norm = 0.0;
  for (int c = 0; c < m; c += kBowNormChunk) {
    const int len = min(kBowNormChunk, m - c);
    for (int i = threadIdx.x; i < len; i += 256) s_v[i] = value[c + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      if (mode == 1) for (int i = 0; i < len; i++) norm += fabs(s_v[i]);
      else for (int i = 0; i < len; i++) norm += s_v[i] * s_v[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) s_norm = mode == 2 ? sqrt(norm) : norm;
  __syncthreads();
  const double nrm = s_norm;
  if (nrm > 0.0)
    for (int i = threadIdx.x; i < m; i += 256) value[i] /= nrm;
}

__global__ void k_fv_flag(const uint32_t* __restrict__ key, int n, int32_t* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  flag[i] = (i < n && key[i] != kNone && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
}

__global__ void k_fv_emit(const uint32_t* __restrict__ key, const int32_t* __restrict__ flag,
                          const int32_t* __restrict__ pos, int n, uint32_t* __restrict__ fv_node,
                          int32_t* __restrict__ fv_ptr, int32_t* __restrict__ fv_n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i < n) {
    if (flag[i]) { fv_node[pos[i]] = key[i]; fv_ptr[pos[i]] = i; }
    // the last kept feature closes the last node
    if (key[i] != kNone && (i == n - 1 || key[i + 1] == kNone)) fv_ptr[pos[n]] = i + 1;
  } else {
    *fv_n = pos[n];
    if (n == 0 || key[0] == kNone) fv_ptr[0] = 0;
  }
}

}  // namespace mcs

struct mcs_bow_workspace {
  int device = 0, max_kp = 0, max_cand = 0;
  int32_t* hist = nullptr;      // [max_cand][30]
  int32_t* keep = nullptr;      // [max_cand][3]
  uint32_t* cand = nullptr;     // [max_cand][max_kp][kBowCap]
  int32_t* cnt = nullptr;       // [max_cand][max_kp][kBowSeg]
  uint32_t* key_in = nullptr;   // [max_kp] each
  uint32_t* key_out = nullptr;
  uint32_t* val_in = nullptr;
  uint32_t* val_out = nullptr;  // [max_kp]      the BowVector's sorted descriptor indices
  int32_t* seg = nullptr;       // [max_kp + 1]  and its word segments
  int32_t* flag = nullptr;      // [max_kp + 1]
  int32_t* pos = nullptr;       // [max_kp + 1]
  void* tmp = nullptr; size_t tmp_bytes = 0;
};

static int bow_ws_create(int32_t device, int32_t max_kp, int32_t max_candidates, bool with_b,
                         mcs_bow_workspace** out);

namespace mcs {

// What can be checked without reading a set's arrays (device and host entries alike).
static int bow_check_shape(const mcs_bow_set* s, const char* what, bool one_frame, bool need_has,
                           bool need_angle, bool need_fv) {
  static thread_local char msg[160];
  const char* err = nullptr;
  if (!s) err = "null set";
  else if (s->n_frames < 0 || s->n_kp_total < 0) err = "negative size";
  else if (one_frame && s->n_frames != 1) err = "must hold exactly one frame";
  else if (s->n_kp_total >= kBowMaxKp) err = "at most 2^19 - 1 keypoints";
  else if (s->n_frames > 0 && !s->off) err = "null offsets";
  else if (s->n_kp_total > 0 && !s->desc) err = "null descriptors";
  else if (s->n_kp_total > 0 && need_has && !s->has_mp) err = "null has_mp";
  else if (s->n_kp_total > 0 && need_angle && !s->angle) err = "check_orientation needs angles";
  else if (s->n_frames > 0 && need_fv && !s->fv_n) err = "null fv_n";
  else if (s->n_kp_total > 0 && need_fv && (!s->fv_node || !s->fv_ptr || !s->fv_feat)) err = "null FeatureVector";
  if (!err) return MCS_OK;
  snprintf(msg, sizeof msg, "SearchByBoW: %s: %s", what, err);
  set_error(msg);
  return MCS_ERR_ARG;
}

// The contents of a host set: offsets, and (overload A) the FeatureVector of every frame.
static int bow_check_host(const mcs_bow_set* s, const char* what, bool need_fv) {
  static thread_local char msg[200];
  auto fail = [&](const char* err, int k) {
    snprintf(msg, sizeof msg, "SearchByBoW: %s frame %d: %s", what, k, err);
    set_error(msg);
    return MCS_ERR_ARG;
  };
  if (s->n_frames == 0) return s->n_kp_total == 0 ? MCS_OK : fail("keypoints without a frame", 0);
  if (s->off[0] != 0) return fail("off[0] must be 0", 0);
  for (int k = 0; k < s->n_frames; k++)
    if (s->off[k + 1] < s->off[k]) return fail("offsets must not decrease", k);
  if (s->off[s->n_frames] != s->n_kp_total) return fail("off[n_frames] must equal n_kp_total", s->n_frames);
  if (!need_fv) return MCS_OK;
  for (int k = 0; k < s->n_frames; k++) {
    const int o = s->off[k], n = s->off[k + 1] - o, m = s->fv_n[k];
    if (m < 0 || m > n) return fail("fv_n outside [0, n_kp]", k);
    if (m == 0) continue;
    const uint32_t* node = s->fv_node + o;
    const int32_t* ptr = s->fv_ptr + o + k;
    const uint32_t* feat = s->fv_feat + o;
    if (ptr[0] < 0 || ptr[m] > n) return fail("fv_ptr outside [0, n_kp]", k);
    for (int j = 0; j < m; j++) {
      if (j > 0 && node[j] <= node[j - 1]) return fail("FeatureVector nodes must be strictly ascending", k);
      if (ptr[j + 1] < ptr[j]) return fail("fv_ptr must not decrease", k);
    }
    for (int i = ptr[0]; i < ptr[m]; i++)
      if (feat[i] >= (uint32_t)n) return fail("feature index >= n_kp", k);
  }
  return MCS_OK;
}

#define MCS_BOW_DISPATCH(bytes, masked, LAUNCH)                         \
  do {                                                                  \
    if ((bytes) == 16) { if (masked) LAUNCH(4, true); else LAUNCH(4, false); }        \
    else if ((bytes) == 32) { if (masked) LAUNCH(8, true); else LAUNCH(8, false); }   \
    else { if (masked) LAUNCH(16, true); else LAUNCH(16, false); }                    \
  } while (0)

static hipError_t bow_run_a(mcs_bow_workspace* ws, const mcs_bow_set& f, const mcs_bow_set& kfs, int bytes,
                            int th_low, double nnratio, int check_ori, int32_t* match_f, int32_t* n_matches,
                            hipStream_t st) {
  const int n_f = f.n_kp_total, n_kf = kfs.n_frames;
  hipError_t e = hipMemsetAsync(n_matches, 0, 4 * (size_t)n_kf, st);
  if (e == hipSuccess && n_f > 0) e = hipMemsetAsync(match_f, 0xFF, 4 * (size_t)n_kf * n_f, st);   // -1
  if (e != hipSuccess || n_f == 0 || kfs.n_kp_total == 0) return e;
  if (check_ori && (e = hipMemsetAsync(ws->hist, 0, 4 * (size_t)n_kf * kHisto, st)) != hipSuccess) return e;
  const bool masked = f.mask != nullptr;
  // F has at most n_f nodes (its count is device data): waves past the last node leave at once
  const dim3 g((n_f + 3) / 4, n_kf);
#define MCS_BOW_NODE(WW, MM)                                                                        \
  hipLaunchKernelGGL((k_bow_node<WW, MM>), g, dim3(256), 0, st, f, kfs, th_low, nnratio, check_ori, \
                     match_f, n_matches, ws->hist)
  MCS_BOW_DISPATCH(bytes, masked, MCS_BOW_NODE);
#undef MCS_BOW_NODE
  if (check_ori) {
    hipLaunchKernelGGL(k_bow_maxima, dim3((n_kf + 63) / 64), dim3(64), 0, st, ws->hist, ws->keep, n_kf);
    hipLaunchKernelGGL(k_bow_prune, dim3((n_f + 255) / 256, n_kf), dim3(256), 0, st, f, kfs, bytes, ws->keep,
                       match_f, n_matches);
  }
  return hipGetLastError();
}

static hipError_t bow_run_b(mcs_bow_workspace* ws, const mcs_bow_set& a, const mcs_bow_set& b, int bytes,
                            int th_low, double nnratio, int32_t* m12, int32_t* n_matches, hipStream_t st) {
  const int n1 = a.n_kp_total, n_kf = b.n_frames;
  hipError_t e = hipMemsetAsync(n_matches, 0, 4 * (size_t)n_kf, st);
  if (e == hipSuccess && n1 > 0) e = hipMemsetAsync(m12, 0xFF, 4 * (size_t)n_kf * n1, st);   // -1
  if (e != hipSuccess || n1 == 0 || b.n_kp_total == 0) return e;
  // no match is possible with best >= th_low, nor with nnratio <= 0 (best >= 0): bound -1
  int bound = -1;
  if (th_low > 0 && nnratio > 0.0) {
    const double q = (double)(th_low - 1) / nnratio;
    const int far = 8 * bytes;
    bound = std::min(far, std::max(th_low - 1, q < (double)far ? (int)std::floor(q) + 1 : far));
  }
  const bool masked = a.mask != nullptr;
  const dim3 g((n1 + 255) / 256, kBowSeg, n_kf);
#define MCS_BOW_CAND(WW, MM) \
  hipLaunchKernelGGL((k_bowkf_cand<WW, MM>), g, dim3(256), 0, st, a, b, bound, ws->cand, ws->cnt)
  MCS_BOW_DISPATCH(bytes, masked, MCS_BOW_CAND);
#undef MCS_BOW_CAND
  const size_t lds = 4 * (size_t)((b.n_kp_total + 31) / 32);   // <= 64 KiB (n_kp_total < 2^19)
#define MCS_BOW_SEQ(WW, MM)                                                                        \
  hipLaunchKernelGGL((k_bowkf_seq<WW, MM>), dim3(n_kf), dim3(64), lds, st, a, b, th_low, nnratio,  \
                     ws->cand, ws->cnt, m12, n_matches)
  MCS_BOW_DISPATCH(bytes, masked, MCS_BOW_SEQ);
#undef MCS_BOW_SEQ
  return hipGetLastError();
}

// Device copy of a host set (the arrays a run reads).
static void bow_upload(host::DevBufs& B, const mcs_bow_set& h, int bytes, bool with_fv, bool with_angle,
                       bool with_has, mcs_bow_set* d) {
  *d = h;
  const size_t n = (size_t)h.n_kp_total, nf = (size_t)h.n_frames;
  d->off = B.up(h.off, nf + 1);
  d->desc = B.up(h.desc, n * bytes);
  d->mask = B.up(h.mask, n * bytes);
  d->angle = with_angle ? B.up(h.angle, n) : nullptr;
  d->has_mp = with_has ? B.up(h.has_mp, n) : nullptr;
  d->fv_node = with_fv ? B.up(h.fv_node, n) : nullptr;
  d->fv_ptr = with_fv ? B.up(h.fv_ptr, n + nf) : nullptr;
  d->fv_feat = with_fv ? B.up(h.fv_feat, n) : nullptr;
  d->fv_n = with_fv ? B.up(h.fv_n, nf) : nullptr;
}

// Shared body of the two host entries: upload, run on a workspace of the call's size, download.
static int bow_host_run(bool overload_b, int device, const mcs_bow_set* one, const mcs_bow_set* many, int bytes,
                        int th_low, double nnratio, int check_ori, int32_t* out, int32_t* n_matches) {
  const int n_one = one->n_kp_total, n_kf = many->n_frames;
  auto reset = [&] {
    for (int64_t i = 0; i < (int64_t)n_kf * n_one; i++) out[i] = -1;
    for (int k = 0; k < n_kf; k++) n_matches[k] = 0;
  };
  reset();
  if (n_kf == 0 || n_one == 0 || many->n_kp_total == 0) return MCS_OK;
  mcs_bow_workspace* ws = nullptr;
  int max_kp = n_one;
  for (int k = 0; k < n_kf; k++) max_kp = std::max(max_kp, many->off[k + 1] - many->off[k]);
  int rc = bow_ws_create(device, max_kp, n_kf, overload_b, &ws);   // opens the device
  if (rc != MCS_OK) return rc;
  host::DevBufs B;
  mcs_bow_set d_one, d_many;
  bow_upload(B, *one, bytes, !overload_b, check_ori != 0, overload_b, &d_one);
  bow_upload(B, *many, bytes, !overload_b, check_ori != 0, true, &d_many);
  int32_t* d_out = B.alloc<int32_t>((size_t)n_kf * n_one);
  int32_t* d_n = B.alloc<int32_t>((size_t)n_kf);
  if (B.err == hipSuccess)
    B.err = overload_b ? bow_run_b(ws, d_one, d_many, bytes, th_low, nnratio, d_out, d_n, nullptr)
                       : bow_run_a(ws, d_one, d_many, bytes, th_low, nnratio, check_ori, d_out, d_n, nullptr);
  B.down(out, d_out, (size_t)n_kf * n_one);
  B.down(n_matches, d_n, (size_t)n_kf);
  mcs_bow_workspace_destroy(ws);
  if (B.err != hipSuccess) {
    reset();
    set_hip_error(B.err, "SearchByBoW", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  return MCS_OK;
}

// Argument checks common to the four search entries.
static int bow_check_call(const mcs_bow_set* one, const mcs_bow_set* many, int bytes, bool overload_b,
                          int check_ori, const void* out, const void* n_matches) {
  int rc = host::check_desc_bytes(bytes, "SearchByBoW");
  if (rc) return rc;
  const char* n1 = overload_b ? "kf1" : "f";
  const char* n2 = overload_b ? "kf2s" : "kfs";
  if ((rc = bow_check_shape(one, n1, true, overload_b, check_ori != 0, !overload_b)) != MCS_OK) return rc;
  if ((rc = bow_check_shape(many, n2, false, true, check_ori != 0, !overload_b)) != MCS_OK) return rc;
  if ((one->mask != nullptr) != (many->mask != nullptr) && one->n_kp_total > 0 && many->n_kp_total > 0) {
    set_error("SearchByBoW: masks for both sides or none");
    return MCS_ERR_ARG;
  }
  if ((many->n_frames > 0 && !n_matches) || (many->n_frames > 0 && one->n_kp_total > 0 && !out)) {
    set_error("SearchByBoW: null output");
    return MCS_ERR_ARG;
  }
  return MCS_OK;
}

static int bow_check_ws(const mcs_bow_workspace* ws, const mcs_bow_set* one, const mcs_bow_set* many) {
  if (!ws) { set_error("SearchByBoW: null workspace"); return MCS_ERR_ARG; }
  if (one->n_kp_total > ws->max_kp || many->n_frames > ws->max_cand ||
      (int64_t)many->n_kp_total > (int64_t)ws->max_kp * ws->max_cand) {
    set_error("SearchByBoW: sizes above the workspace (max_kp / max_candidates)");
    return MCS_ERR_ARG;
  }
  return MCS_OK;
}

}  // namespace mcs

using namespace mcs;

// with_b = false leaves out overload B's candidate slots (the host entry of overload A)
static int bow_ws_create(int32_t device, int32_t max_kp, int32_t max_candidates, bool with_b,
                         mcs_bow_workspace** out) {
  if (!out || max_kp < 1 || max_kp >= kBowMaxKp || max_candidates < 1) {
    set_error("bow workspace: need 1 <= max_kp < 2^19 and max_candidates >= 1");
    return MCS_ERR_ARG;
  }
  *out = nullptr;
  if (int rc = host::open_device(device, "bow workspace")) return rc;
  auto* w = new (std::nothrow) mcs_bow_workspace();
  if (!w) return MCS_ERR_ARG;
  w->device = device; w->max_kp = max_kp; w->max_cand = max_candidates;
  const size_t n = (size_t)max_kp, c = (size_t)max_candidates;
  hipError_t e = hipMalloc((void**)&w->hist, 4 * c * kHisto);
  if (e == hipSuccess) e = hipMalloc((void**)&w->keep, 4 * c * 3);
  if (e == hipSuccess && with_b) e = hipMalloc((void**)&w->cand, 4 * c * n * kBowCap);
  if (e == hipSuccess && with_b) e = hipMalloc((void**)&w->cnt, 4 * c * n * kBowSeg);
  if (e == hipSuccess) e = hipMalloc((void**)&w->key_in, 4 * n);
  if (e == hipSuccess) e = hipMalloc((void**)&w->key_out, 4 * n);
  if (e == hipSuccess) e = hipMalloc((void**)&w->val_in, 4 * n);
  if (e == hipSuccess) e = hipMalloc((void**)&w->val_out, 4 * n);
  if (e == hipSuccess) e = hipMalloc((void**)&w->seg, 4 * (n + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->flag, 4 * (n + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&w->pos, 4 * (n + 1));
  size_t b_scan = 0, b_sort = 0;
  if (e == hipSuccess)
    e = rocprim::exclusive_scan(nullptr, b_scan, w->flag, w->pos, 0, n + 1, rocprim::plus<int32_t>(), (hipStream_t)0);
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, b_sort, w->key_in, w->key_out, w->val_in, w->val_in, n, 0, 32,
                                  (hipStream_t)0);
  w->tmp_bytes = std::max<size_t>(16, std::max(b_scan, b_sort));
  if (e == hipSuccess) e = hipMalloc(&w->tmp, w->tmp_bytes);
  if (e != hipSuccess) {
    mcs_bow_workspace_destroy(w);
    set_hip_error(e, "bow workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

extern "C" {

int mcs_bow_workspace_create(int32_t device, int32_t max_kp, int32_t max_candidates,
                             mcs_bow_workspace** out) {
  return bow_ws_create(device, max_kp, max_candidates, true, out);
}

void mcs_bow_workspace_destroy(mcs_bow_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  void* bufs[] = {w->hist, w->keep, w->cand, w->cnt, w->key_in, w->key_out, w->val_in, w->val_out, w->seg,
                  w->flag, w->pos, w->tmp};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  delete w;
}

int mcs_feature_vector_device(mcs_bow_workspace* ws, const uint32_t* d_node, const double* d_weight,
                              int32_t n, uint32_t* d_fv_node, int32_t* d_fv_ptr,
                              uint32_t* d_fv_feat, int32_t* d_fv_n, void* stream) {
  if (!ws || n < 0 || !d_fv_ptr || !d_fv_n || (n > 0 && (!d_node || !d_weight || !d_fv_node || !d_fv_feat))) {
    set_error("feature_vector_device: bad arguments");
    return MCS_ERR_ARG;
  }
  if (n > ws->max_kp) { set_error("feature_vector_device: n above the workspace's max_kp"); return MCS_ERR_ARG; }
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    MCS_HIP_CHECK(hipMemsetAsync(d_fv_n, 0, 4, st));
    MCS_HIP_CHECK(hipMemsetAsync(d_fv_ptr, 0, 4, st));
    return MCS_OK;
  }
  const int nb = (n + 1 + 255) / 256;
  hipLaunchKernelGGL(k_fv_keys, dim3(nb), dim3(256), 0, st, d_node, d_weight, n, ws->key_in, ws->val_in);
  // stable by construction (LSD radix sort): features of one node stay in feature order
  size_t need = 0;
  MCS_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, ws->key_in, ws->key_out, ws->val_in, d_fv_feat, (size_t)n,
                                          0, 32, st));
  if (need > ws->tmp_bytes) { set_error("feature_vector_device: sort storage above the workspace"); return MCS_ERR_CAPACITY; }
  size_t b = ws->tmp_bytes;
  MCS_HIP_CHECK(rocprim::radix_sort_pairs(ws->tmp, b, ws->key_in, ws->key_out, ws->val_in, d_fv_feat, (size_t)n,
                                          0, 32, st));
  hipLaunchKernelGGL(k_fv_flag, dim3(nb), dim3(256), 0, st, ws->key_out, n, ws->flag);
  b = ws->tmp_bytes;
  MCS_HIP_CHECK(rocprim::exclusive_scan(ws->tmp, b, ws->flag, ws->pos, 0, (size_t)n + 1, rocprim::plus<int32_t>(), st));
  hipLaunchKernelGGL(k_fv_emit, dim3(nb), dim3(256), 0, st, ws->key_out, ws->flag, ws->pos, n, d_fv_node, d_fv_ptr,
                     d_fv_n);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_bow_vector_device(mcs_bow_workspace* ws, const mcs_vocab* voc, const uint32_t* d_word,
                          const double* d_weight, int32_t n, uint32_t* d_bow_word, double* d_bow_value,
                          int32_t* d_bow_n, void* stream) {
  int32_t info[6];
  if (!ws || !voc || n < 0 || !d_bow_n || (n > 0 && (!d_word || !d_weight || !d_bow_word || !d_bow_value)) ||
      mcs_vocab_info(voc, info) != MCS_OK) {
    set_error("bow_vector_device: bad arguments");
    return MCS_ERR_ARG;
  }
  if (n > ws->max_kp) { set_error("bow_vector_device: n above the workspace's max_kp"); return MCS_ERR_ARG; }
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || info[5] == 0) {   // v.clear(); an empty vocabulary returns at once (:1133-1138)
    MCS_HIP_CHECK(hipMemsetAsync(d_bow_n, 0, 4, st));
    return MCS_OK;
  }
  const int nb = (n + 1 + 255) / 256;
  hipLaunchKernelGGL(k_fv_keys, dim3(nb), dim3(256), 0, st, d_word, d_weight, n, ws->key_in, ws->val_in);
  // stable (LSD radix sort): the occurrences of one word stay in feature order
  size_t need = 0;
  MCS_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, ws->key_in, ws->key_out, ws->val_in, ws->val_out, (size_t)n,
                                          0, 32, st));
  if (need > ws->tmp_bytes) { set_error("bow_vector_device: sort storage above the workspace"); return MCS_ERR_CAPACITY; }
  size_t b = ws->tmp_bytes;
  MCS_HIP_CHECK(rocprim::radix_sort_pairs(ws->tmp, b, ws->key_in, ws->key_out, ws->val_in, ws->val_out, (size_t)n,
                                          0, 32, st));
  hipLaunchKernelGGL(k_fv_flag, dim3(nb), dim3(256), 0, st, ws->key_out, n, ws->flag);
  b = ws->tmp_bytes;
  MCS_HIP_CHECK(rocprim::exclusive_scan(ws->tmp, b, ws->flag, ws->pos, 0, (size_t)n + 1, rocprim::plus<int32_t>(), st));
  hipLaunchKernelGGL(k_fv_emit, dim3(nb), dim3(256), 0, st, ws->key_out, ws->flag, ws->pos, n, d_bow_word, ws->seg,
                     d_bow_n);
  const int scoring = info[2], weighting = info[3];
  const bool tf = weighting == 0 || weighting == 1;
  // mustNormalize (ScoringObject.h:74-89): L2 scoring with L2, DOT_PRODUCT not at all, the rest L1
  const int mode = scoring == 5 ? (tf ? 3 : 0) : scoring == 1 ? 2 : 1;
  hipLaunchKernelGGL(k_bow_values, dim3(nb), dim3(256), 0, st, ws->seg, ws->val_out, d_weight, d_bow_n, n,
                     tf ? 1 : 0, d_bow_value);
  hipLaunchKernelGGL(k_bow_normalize, dim3(1), dim3(256), 0, st, d_bow_n, n, mode, d_bow_value);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_search_by_bow_device(mcs_bow_workspace* ws, const mcs_bow_set* f, const mcs_bow_set* kfs,
                             int32_t bytes, int32_t th_low, double nnratio,
                             int32_t check_orientation, int32_t* d_match_f, int32_t* d_n_matches,
                             void* stream) {
  int rc = bow_check_call(f, kfs, bytes, false, check_orientation, d_match_f, d_n_matches);
  if (rc == MCS_OK) rc = bow_check_ws(ws, f, kfs);
  if (rc != MCS_OK) return rc;
  if (kfs->n_frames == 0) return MCS_OK;
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  const hipError_t e = bow_run_a(ws, *f, *kfs, bytes, th_low, nnratio, check_orientation, d_match_f, d_n_matches,
                                 (hipStream_t)stream);
  if (e != hipSuccess) { set_hip_error(e, "SearchByBoW", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

int mcs_search_by_bow(int32_t device, const mcs_bow_set* f, const mcs_bow_set* kfs, int32_t bytes,
                      int32_t th_low, double nnratio, int32_t check_orientation, int32_t* match_f,
                      int32_t* n_matches) {
  int rc = bow_check_call(f, kfs, bytes, false, check_orientation, match_f, n_matches);
  if (rc == MCS_OK) rc = bow_check_host(f, "f", true);
  if (rc == MCS_OK) rc = bow_check_host(kfs, "kfs", true);
  if (rc != MCS_OK) return rc;
  return bow_host_run(false, device, f, kfs, bytes, th_low, nnratio, check_orientation, match_f, n_matches);
}

int mcs_search_by_bow_kf_device(mcs_bow_workspace* ws, const mcs_bow_set* kf1,
                                const mcs_bow_set* kf2s, int32_t bytes, int32_t th_low,
                                double nnratio, int32_t* d_matches12, int32_t* d_n_matches,
                                void* stream) {
  int rc = bow_check_call(kf1, kf2s, bytes, true, 0, d_matches12, d_n_matches);
  if (rc == MCS_OK) rc = bow_check_ws(ws, kf1, kf2s);
  if (rc != MCS_OK) return rc;
  if (kf2s->n_frames == 0) return MCS_OK;
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  const hipError_t e = bow_run_b(ws, *kf1, *kf2s, bytes, th_low, nnratio, d_matches12, d_n_matches,
                                 (hipStream_t)stream);
  if (e != hipSuccess) { set_hip_error(e, "SearchByBoW", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

int mcs_search_by_bow_kf(int32_t device, const mcs_bow_set* kf1, const mcs_bow_set* kf2s,
                         int32_t bytes, int32_t th_low, double nnratio, int32_t* matches12,
                         int32_t* n_matches) {
  int rc = bow_check_call(kf1, kf2s, bytes, true, 0, matches12, n_matches);
  if (rc == MCS_OK) rc = bow_check_host(kf1, "kf1", false);
  if (rc == MCS_OK) rc = bow_check_host(kf2s, "kf2s", false);
  if (rc != MCS_OK) return rc;
  return bow_host_run(true, device, kf1, kf2s, bytes, th_low, nnratio, 0, matches12, n_matches);
}

}  // extern "C"
