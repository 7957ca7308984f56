// The ordered selection of the windowed matchers on the device (track_match.hip): rules 0, 1
// and 3 of mcs_window_select (window_host.cpp), bit-equal.
//
// The sequential loop gives query q the assignment state left by every earlier query, and that
// state reaches q only through keypoints of its own candidate list that are still unassigned.
// So q's outcome is fixed once every earlier query sharing such a keypoint is settled.  Rounds:
//   mark    every unsettled query raises mark[k] to (round, lowest query) on each unassigned
//           candidate k, with one atomic per candidate;
//   decide  a query that holds the mark on all of them has no earlier unsettled query on any:
//           it scans its list in order as the host loop does (skip assigned, strict < for best,
//           else-if for second, octaves for rule 0), applies the rule's accept test and settles.
//           Two such queries share no unassigned candidate, so they race on nothing;
//   commit  the accepted keypoints become assigned, after a barrier, for the next round.
// The lowest unsettled query always holds its marks, so a round settles at least one query and
// the result does not depend on scheduling.  One workgroup per camera: a query's candidates are
// keypoints of its own camera's cells, so the workgroups share nothing but the match counter.
// Nothing waits on another workgroup.  The round number in the mark's high half makes older
// marks lose without a reset pass.
// A workgroup whose queries average kWideAvg candidates or more gives every query a wave instead
// of a thread (long lists, few queries: the windows of rule 1); the sequential scan then becomes
// the two smallest keys distance << 32 | position in the list, which is the same pair: under
// strict < and the else-if, best and second are the first and second of the list ordered by
// (distance, position).
#pragma once
#include "track_grid.hpp"
#include <climits>

namespace mcs {
namespace trk {

constexpr int kSelThreads = 1024;
constexpr int kWideAvg = 24;     // candidates per live query from which a query gets a wave

struct SelectArgs {
  int rule, nq, n_kp, th, max_q;
  double nnratio;
  int64_t cap;
  const int32_t* q_cl; const int32_t* cand_ptr; const int32_t* cand_kp; const int32_t* cand_dist;
  const int32_t* kp_oct;
  int64_t* status;
  uint8_t* assigned; int32_t* match; int32_t* kp_query; int32_t* n_matches;
  unsigned long long* mark;   // [n_kp], zeroed
  int32_t* live;              // [2][kMaxCams][max_q]
};

__device__ __forceinline__ unsigned long long mark_key(int round, int q) {
  return ((unsigned long long)(unsigned)(round + 1) << 32) | (unsigned)(INT_MAX - q);
}

// the rule's accept test on (best, second) as window_host.cpp spells it
__device__ __forceinline__ bool accept_match(const SelectArgs& a, int best, int best2, int lvl, int lvl2) {
  if (a.rule == 0) return best <= a.th && !(lvl == lvl2 && best > a.nnratio * best2);   // :154-157
  if (a.rule == 1) return best <= a.th;                                                 // :2078
  return best <= best2 * a.nnratio && best <= a.th;                                     // :416
}

// A query that does not hold all its marks is settled all the same when no earlier unsettled
// query can change its outcome.  Earlier queries only ever take keypoints away, so best and
// second only move up the list ordered by (distance, position):
//   no unassigned candidate, or best > th: no match, whatever is taken (every rule);
//   rule 1 (best only): the match stands if the mark on best is its own, i.e. no earlier unsettled
//     query has best in its list;
//   rule 3: an accepted match stands likewise (a larger second keeps best <= second * ratio).
// Rule 0's ratio test reads the second's octave, which can change either way: it waits for all
// its marks.
__device__ __forceinline__ bool settled_early(const SelectArgs& a, int bk, int best, bool accept,
                                              bool best_is_mine) {
  if (bk < 0 || best > a.th) return true;
  if (a.rule == 1) return best_is_mine;
  if (a.rule == 3) return accept && best_is_mine;
  return false;
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// decide for the query with mark `key` and candidates [s, e) by one thread, the host loop as it
// stands: false = an earlier unsettled query holds a mark; else *bi = the keypoint to take or -1
__device__ __forceinline__ bool decide_thread(const SelectArgs& a, unsigned long long key, int s, int e,
                                              int* bi) {
  int best = INT_MAX, best2 = INT_MAX, bk = -1, lvl = -1, lvl2 = -1;
  bool foreign = false, best_is_mine = false;
  for (int c = s; c < e; c++) {
    const int k = a.cand_kp[c];
    if ((unsigned)k >= (unsigned)a.n_kp || a.assigned[k]) continue;
    const bool mine = __hip_atomic_load(&a.mark[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key;
    if (!mine) {
      if (a.rule == 0) return false;
      foreign = true;
    }
    const int d = a.cand_dist[c];
    if (d < best) {
      best2 = best; best = d;
      lvl2 = lvl; lvl = a.rule == 0 ? a.kp_oct[k] : 0;
      bk = k;
      best_is_mine = mine;
    } else if (d < best2) {
      lvl2 = a.rule == 0 ? a.kp_oct[k] : 0;
      best2 = d;
    }
  }
  const bool accept = bk >= 0 && accept_match(a, best, best2, lvl, lvl2);
  if (foreign && !settled_early(a, bk, best, accept, best_is_mine)) return false;
  *bi = accept ? bk : -1;
  return true;
}

// decide for the query with mark `key` and candidates [s, e) by one wave: false = an earlier
// unsettled query holds a mark; else *bi = the keypoint to take or -1
__device__ __forceinline__ bool decide_wide(const SelectArgs& a, int lane, unsigned long long key, int s,
                                            int e, int* bi) {
  constexpr unsigned long long kNone = ~0ull;
  unsigned long long k1 = kNone, k2 = kNone;   // this lane's two smallest distance << 32 | position
  bool foreign = false;
  for (int c = s + lane; c < e; c += 64) {
    const int k = a.cand_kp[c];
    if ((unsigned)k >= (unsigned)a.n_kp || a.assigned[k]) continue;
    if (__hip_atomic_load(&a.mark[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != key) foreign = true;
    const unsigned long long v = ((unsigned long long)(unsigned)a.cand_dist[c] << 32) | (unsigned)(c - s);
    if (v < k1) { k2 = k1; k1 = v; }
    else if (v < k2) k2 = v;
  }
  const bool any_foreign = __ballot(foreign) != 0;
  if (any_foreign && a.rule == 0) return false;
  const unsigned long long m1 = wave_min64(k1);
  const unsigned long long m2 = wave_min64(k1 == m1 ? k2 : k1);
  *bi = -1;
  if (m1 == kNone) return true;
  const int best = (int)(m1 >> 32), k_best = a.cand_kp[s + (int)(unsigned)m1];
  int best2 = INT_MAX, lvl2 = -1;
  if (m2 != kNone) {
    best2 = (int)(m2 >> 32);
    lvl2 = a.rule == 0 ? a.kp_oct[a.cand_kp[s + (int)(unsigned)m2]] : 0;
  }
  const bool accept = accept_match(a, best, best2, a.rule == 0 ? a.kp_oct[k_best] : 0, lvl2);
  if (any_foreign) {
    const bool best_is_mine =
        __hip_atomic_load(&a.mark[k_best], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key;
    if (!settled_early(a, k_best, best, accept, best_is_mine)) return false;
  }
  if (accept) *bi = k_best;
  return true;
}

__global__ __launch_bounds__(kSelThreads) void k_track_select(SelectArgs a) {
  __shared__ int s_n[2];
  __shared__ int s_len;
  __shared__ int s_sum[kSelThreads / 64];
  const int64_t total = a.status[0];
  if (total > a.cap) return;                       // overflow: the lists were not written
  const int cam = blockIdx.x, tid = threadIdx.x;
  const int lim = (int)total;
  int32_t* cur = a.live + (int64_t)cam * a.max_q;
  int32_t* nxt = a.live + (int64_t)(kMaxCams + cam) * a.max_q;
  if (tid == 0) { s_n[0] = 0; s_n[1] = 0; s_len = 0; }
  __syncthreads();
  for (int q = tid; q < a.nq; q += kSelThreads) {  // a query without candidates is settled
    const int len = a.cand_ptr[q + 1] - a.cand_ptr[q];
    if (a.q_cl[3 * q] == cam && len > 0) {
      cur[atomicAdd(&s_n[0], 1)] = q;
      atomicAdd(&s_len, min(len, 1 << 16));
    }
  }
  __syncthreads();
  int n_live = s_n[0], w = 0, round = 0, mine = 0;
  const int max_rounds = n_live;
  const bool wide = n_live > 0 && s_len / n_live >= kWideAvg;
  const int lane = tid & 63, wave = tid >> 6;
  // a query's lanes: a wave (lane 0 leads) or one thread
  const int first = wide ? wave : tid, stride = wide ? kSelThreads / 64 : kSelThreads;
  const int l0 = wide ? lane : 0, step = wide ? 64 : 1;
  while (n_live > 0 && round < max_rounds) {
    for (int i = first; i < n_live; i += stride) {             // mark
      const int q = cur[i];
      const unsigned long long key = mark_key(round, q);
      const int s = min(max(a.cand_ptr[q], 0), lim), e = min(max(a.cand_ptr[q + 1], s), lim);
      for (int c = s + l0; c < e; c += step) {
        const int k = a.cand_kp[c];
        if ((unsigned)k >= (unsigned)a.n_kp || a.assigned[k]) continue;
        atomicMax(&a.mark[k], key);
      }
    }
    __syncthreads();
    for (int i = first; i < n_live; i += stride) {             // decide
      const int q = cur[i];
      const int s = min(max(a.cand_ptr[q], 0), lim), e = min(max(a.cand_ptr[q + 1], s), lim);
      int bi;
      const bool ready = wide ? decide_wide(a, lane, mark_key(round, q), s, e, &bi)
                              : decide_thread(a, mark_key(round, q), s, e, &bi);
      if (l0 != 0) continue;
      if (!ready) { nxt[atomicAdd(&s_n[w ^ 1], 1)] = q; continue; }
      if (bi >= 0) {
        a.match[q] = bi;
        a.kp_query[bi] = q;
        mine++;
      }
    }
    __syncthreads();
    for (int i = tid; i < n_live; i += kSelThreads) {          // commit
      const int m = a.match[cur[i]];
      if (m >= 0) a.assigned[m] = 1;
    }
    n_live = s_n[w ^ 1];
    __syncthreads();
    if (tid == 0) s_n[w] = 0;
    int32_t* const t = cur; cur = nxt; nxt = t;
    w ^= 1;
    round++;
  }
  mine = dev::wave_sum(mine);
  if ((tid & 63) == 0) s_sum[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
    for (int i = 0; i < kSelThreads / 64; i++) sum += s_sum[i];
    if (sum) atomicAdd(a.n_matches, sum);
    // the call's rounds in the flags' high half (cleared before the launch): the most of any camera
    atomicMax(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)round << 32);
  }
}

}  // namespace trk
}  // namespace mcs
