// Keyframe database on gfx950: loop and relocalisation candidates (include/mcs_kfdb.h).
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cMultiKeyFrameDatabase::add / erase / clear            src/cMultiKeyFrameDatabase.cpp:43-79
//   DetectLoopCandidates / DetectRelocalisationCandidates  :82-221, :223-340
//   L1Scoring::score                                       ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//   the minScore loop of cLoopClosing::DetectLoop          src/cLoopClosing.cpp:141-157
//
// The reference walks an inverted file (word -> keyframes).  Here the BowVectors of the added
// keyframes lie packed in add order (word u32 + value f64 = 12 B per entry) and one query is one
// streaming pass over them:
//   k_table    scatter the query's entry index into a word -> query-slot table (n_words int32,
//              all -1 between calls)
//   k_scan     one wave per keyframe, 64 entries at a time: table lookup per lane, ballot, common
//              += popcount, the smallest shared word from the first set bit of the first non-empty
//              ballot, and the L1 terms of the matching lanes added IN LANE ORDER (= ascending
//              word order, the order of L1Scoring::score) by a wave-uniform loop over the set bits
//   k_classify per keyframe: the list membership rules and the member updates of :97-117 /
//              :231-248, the maximum of the words over the list, the sort key
//   rocprim    radix sort of (smallest shared word, slot): the order in which the reference's walk
//              (query words ascending, each inverted list in add order) first meets a keyframe
//   k_finish   one block: scores of the keyframes above minCommonWords into the members, the
//              covisibility accumulation (neighbours added serially in the given order), the
//              retain test, first-occurrence dedupe and the ordered output
//   k_table    clear the entries the query set
// A table lookup costs one 4-byte gather from an L2-resident table per entry; a binary search of
// each entry in the query's words would cost log2(n_query) dependent gathers instead.
//
// Exactness: every double is produced by + - / fabs on correctly rounded IEEE operations in the
// reference's order; the only multiplies feed a truncation and a comparison, so no FMA can form.
#include "host_util.hpp"
#include "kfdb_host.hpp"
#include "../../include/mcs_kfdb.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <climits>
#include <new>

struct mcs_kfdb {
  int device = 0, n_words = 0;
  mcs::kfdb::Account acct;
  // the packed BowVectors and the members per slot
  uint32_t* word = nullptr;      // [max_entries]
  double* value = nullptr;       // [max_entries]
  int32_t* ptr = nullptr;        // [max_keyframes + 1]
  uint8_t* alive = nullptr;      // [max_keyframes]
  int64_t* query[2] = {nullptr, nullptr};   // loop_query, reloc_query   (index 0 = loop, 1 = reloc)
  int32_t* words[2] = {nullptr, nullptr};   // loop_words, reloc_words
  double* score[2] = {nullptr, nullptr};    // loop_score, reloc_score
  int32_t* table = nullptr;      // [n_words], -1 between calls
  // scratch of one call, [max_keyframes] each
  int32_t* s_common = nullptr;
  uint32_t* s_minword = nullptr;
  double* s_score = nullptr;
  uint64_t* key_in = nullptr;
  uint64_t* key_out = nullptr;
  int32_t* first = nullptr;
  double* acc = nullptr;
  int32_t* best = nullptr;
  uint8_t* in_sm = nullptr;
  int32_t* stats = nullptr;      // [0] maxCommonWords, [1] length of lKFsSharingWords
  void* tmp = nullptr; size_t tmp_bytes = 0;
};

namespace mcs {
namespace kfdb {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct Query { const uint32_t* word; const double* value; const int32_t* n; int cap; };

__device__ __forceinline__ int query_len(const Query& q) { return min(max(*q.n, 0), q.cap); }

// set: table[word[i]] = i;  clear: table[word[i]] = -1.  Words outside the vocabulary are skipped.
__global__ __launch_bounds__(kBlock) void k_table(Query q, int32_t* __restrict__ table, int n_words, int set) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= query_len(q)) return;
  const uint32_t w = q.word[i];
  if (w < (uint32_t)n_words) table[w] = set ? i : -1;
}

// add(): copy a BowVector behind the last one and start the keyframe's members
__global__ __launch_bounds__(kBlock) void k_add(const uint32_t* __restrict__ bw, const double* __restrict__ bv,
                                                const int32_t* __restrict__ bn, int n_upper, int slot,
                                                int max_entries, double score_init, uint32_t* __restrict__ word,
                                                double* __restrict__ value, int32_t* __restrict__ ptr,
                                                uint8_t* __restrict__ alive, int64_t* __restrict__ lq,
                                                int32_t* __restrict__ lw, double* __restrict__ ls,
                                                int64_t* __restrict__ rq, int32_t* __restrict__ rw,
                                                double* __restrict__ rs) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const int base = min(max(ptr[slot], 0), max_entries);
  const int n = min(min(max(*bn, 0), n_upper), max_entries - base);
  if (i < n) { word[base + i] = bw[i]; value[base + i] = bv[i]; }
  if (i == 0) {
    ptr[slot + 1] = base + n;
    alive[slot] = 1;
    lq[slot] = 0; rq[slot] = 0;   // cMultiKeyFrame.cpp:44-45
    lw[slot] = 0; rw[slot] = 0;
    ls[slot] = score_init; rs[slot] = score_init;
  }
}

__device__ __forceinline__ double read_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// One wave per item.  list == null: item = slot, erased keyframes share nothing.  list != null:
// item i is slot list[i] (the minScore loop; the caller leaves out bad keyframes).
__global__ __launch_bounds__(kBlock) void k_scan(const uint32_t* __restrict__ word, const double* __restrict__ value,
                                                 const int32_t* __restrict__ ptr, const uint8_t* __restrict__ alive,
                                                 const int32_t* __restrict__ list, int n_items, int n_slots,
                                                 int max_entries, const int32_t* __restrict__ table, int n_words,
                                                 Query q, int32_t* __restrict__ o_common,
                                                 uint32_t* __restrict__ o_minword, double* __restrict__ o_score) {
  const int item = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = dev::lane_id();
  const int s = list ? list[item] : item;
  const bool ok = s >= 0 && s < n_slots && (list || alive[s]);
  int common = 0;
  uint32_t minword = 0xFFFFFFFFu;
  double sum = 0.0;
  if (ok) {
    const int qn = query_len(q);
    const int b = max(ptr[s], 0), e = min(ptr[s + 1], max_entries);
    for (int i = b; i < e; i += 64) {
      const int j = i + lane;
      uint32_t w = 0;
      int qi = -1;
      if (j < e) {
        w = word[j];
        if (w < (uint32_t)n_words) qi = table[w];
      }
      if (qi >= qn) qi = -1;
      uint64_t m = __ballot(qi >= 0);
      if (m == 0) continue;
      double t = 0.0;
      if (qi >= 0) {
        const double vi = q.value[qi], wi = value[j];   // vi: the query is score()'s first argument
        t = fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
      if (common == 0) minword = (uint32_t)__builtin_amdgcn_readlane((int)w, __ffsll((unsigned long long)m) - 1);
      common += __popcll(m);
      // score += term, one shared word after the other in ascending word order: serial on purpose
      while (m) {
        const int bit = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        sum += read_lane(t, bit);
      }
    }
  }
  if (lane == 0) {
    o_common[item] = common;
    o_minword[item] = minword;
    o_score[item] = -sum / 2.0;
  }
}

// The list rules of :97-117 (loop) and :231-248 (reloc) for one keyframe that shares `c` words.
// The walk meets the keyframe once per shared word; what it leaves behind after c meetings:
//   stored query != id, connected (loop only): words reset at every meeting, then ++ -> 1
//   stored query != id otherwise: query = id, words = c, listed
//   stored query == id: words += c, not listed
__global__ __launch_bounds__(kBlock) void k_classify(int loop, int n_slots, int64_t qid,
                                                     const uint8_t* __restrict__ connected,
                                                     const int32_t* __restrict__ s_common,
                                                     const uint32_t* __restrict__ s_minword,
                                                     const double* __restrict__ s_score, int64_t* __restrict__ query,
                                                     int32_t* __restrict__ words, uint64_t* __restrict__ key,
                                                     int32_t* __restrict__ first, int32_t* __restrict__ stats,
                                                     int32_t* __restrict__ d_common, double* __restrict__ d_score) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  bool listed = false;
  int w = 0;
  if (s < n_slots) {
    const int c = s_common[s];
    if (c > 0) {
      if (query[s] != qid) {
        if (loop && connected[s]) {
          words[s] = 1;
        } else {
          query[s] = qid;
          words[s] = c;
          w = c;
          listed = true;
        }
      } else {
        words[s] += c;
      }
    }
    key[s] = listed ? (((uint64_t)s_minword[s] << 32) | (uint32_t)s) : ~0ull;
    first[s] = INT_MAX;
    if (d_common) d_common[s] = c;
    if (d_score) d_score[s] = s_score[s];
  }
  // maxCommonWords over the list and the list's length: one atomic pair per wave
  const uint64_t m = __ballot(listed);
  if (m == 0) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o, 64));
  if (dev::lane_id() == 0) {
    atomicMax(&stats[0], w);
    atomicAdd(&stats[1], __popcll(m));
  }
}

// Steps 3 and 4 and the output loop (:136-220, :262-339) over the sorted list, one block.
__global__ __launch_bounds__(kBlock) void k_finish(int loop, int n_slots, int64_t qid,
                                                   const double* __restrict__ d_min_score,
                                                   const int32_t* __restrict__ neigh,
                                                   const uint64_t* __restrict__ key,
                                                   const double* __restrict__ s_score,
                                                   const int64_t* __restrict__ query,
                                                   const int32_t* __restrict__ words, double* __restrict__ score,
                                                   int32_t* __restrict__ first, double* __restrict__ acc,
                                                   int32_t* __restrict__ best, uint8_t* __restrict__ in_sm,
                                                   const int32_t* __restrict__ stats, int32_t* __restrict__ cand,
                                                   int cap, int32_t* __restrict__ n_cand) {
  __shared__ double s_best[kWaves];
  __shared__ int s_tmp[kWaves + 1];
  const int tid = threadIdx.x;
  const int M = min(max(stats[1], 0), n_slots);
  const int min_common = (int)((double)stats[0] * 0.8);   // a double multiply, then truncation
  const double min_score = loop ? *d_min_score : 0.0;
  // mLoopScore / mRelocScore are written for scored keyframes only; every write precedes every
  // neighbour read, as the reference's step 3 precedes its step 4
  for (int i = tid; i < M; i += kBlock) {
    const int s = (int)(uint32_t)key[i];
    bool in = false;
    if (s >= 0 && s < n_slots && words[s] > min_common) {
      const double si = s_score[s];
      score[s] = si;
      in = !loop || si >= min_score;
    }
    in_sm[i] = in;
  }
  __threadfence_block();
  __syncthreads();
  double best_acc = min_score;   // bestAccScore: minScore (loop, :164) or 0 (reloc, :287)
  for (int i = tid; i < M; i += kBlock) {
    if (!in_sm[i]) continue;
    const int s = (int)(uint32_t)key[i];
    const double si = s_score[s];
    double a = si, bs = si;
    int bk = s;
    for (int k = 0; k < MCS_KFDB_NEIGH; k++) {   // serial, in the given order
      const int s2 = neigh[(size_t)s * MCS_KFDB_NEIGH + k];
      if (s2 < 0 || s2 >= n_slots) continue;
      if (query[s2] != qid) continue;
      if (loop && !(words[s2] > min_common)) continue;
      const double v = score[s2];   // reloc: possibly a stale value of an earlier query (:306)
      a += v;
      if (v > bs) { bk = s2; bs = v; }
    }
    acc[i] = a;
    best[i] = bk;
    if (a > best_acc) best_acc = a;
  }
  // a maximum is the same in any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(best_acc, o, 64);
    if (other > best_acc) best_acc = other;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = best_acc;
  __syncthreads();
  best_acc = s_best[0];
  for (int k = 1; k < kWaves; k++)
    if (s_best[k] > best_acc) best_acc = s_best[k];
  const double retain = 0.75 * best_acc;
  // spAlreadyAddedKF: the first list position that names a keyframe keeps it
  for (int i = tid; i < M; i += kBlock)
    if (in_sm[i] && acc[i] > retain) atomicMin(&first[best[i]], i);
  __threadfence_block();
  __syncthreads();
  int base = 0;
  for (int c0 = 0; c0 < M; c0 += kBlock) {
    const int i = c0 + tid;
    const bool f = i < M && in_sm[i] && acc[i] > retain &&
                   __hip_atomic_load(&first[best[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
    int total = 0;
    const int pos = dev::block_excl_scan<kBlock>(f ? 1 : 0, s_tmp, &total);
    if (f && base + pos < cap) cand[base + pos] = best[i];
    base += total;
  }
  if (tid == 0) *n_cand = base;
}

// min over the listed scores, from 1.0 with strict '<' (cLoopClosing.cpp:144-157); a minimum is
// the same in any order
__global__ __launch_bounds__(kBlock) void k_min_score(const double* __restrict__ s_score,
                                                      const int32_t* __restrict__ list, int n, int n_slots,
                                                      double* __restrict__ out) {
  __shared__ double s_min[kWaves];
  double m = 1.0;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const int s = list[i];
    if (s < 0 || s >= n_slots) continue;
    const double v = s_score[i];
    if (v < m) m = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(m, o, 64);
    if (other < m) m = other;
  }
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; k++)
      if (s_min[k] < m) m = s_min[k];
    *out = m;
  }
}

static int check_query(const mcs_kfdb_query* q, const char* who) {
  static thread_local char msg[128];
  const char* err = nullptr;
  if (!q) err = "null query";
  else if (q->cap < 0) err = "negative query capacity";
  else if (!q->d_n) err = "null query count";
  else if (q->cap > 0 && (!q->d_word || !q->d_value)) err = "null query buffers";
  if (!err) return MCS_OK;
  std::snprintf(msg, sizeof msg, "%s: %s", who, err);
  return host::bad_arg(msg);
}

static int detect(mcs_kfdb* db, const mcs_kfdb_query* query, int64_t qid, const uint8_t* d_connected,
                  const double* d_min_score, const int32_t* d_neigh, const mcs_kfdb_result* out, int loop,
                  void* stream) {
  const char* who = loop ? "kfdb detect_loop" : "kfdb detect_reloc";
  if (!db || !out) return host::bad_arg("kfdb detect: null database or result");
  if (int rc = check_query(query, who)) return rc;
  if (out->cap < 0 || !out->d_n_candidates || (out->cap > 0 && !out->d_candidates))
    return host::bad_arg("kfdb detect: bad candidate buffers");
  const int n = db->acct.n_added;
  if (n > 0 && (!d_neigh || (loop && (!d_connected || !d_min_score))))
    return host::bad_arg("kfdb detect: null connected / min_score / neighbours");
  MCS_HIP_CHECK(hipSetDevice(db->device));
  hipStream_t st = (hipStream_t)stream;
  MCS_HIP_CHECK(hipMemsetAsync(out->d_n_candidates, 0, 4, st));
  if (n == 0 || query->cap == 0) {   // nothing shares a word: the list is empty (:120-121)
    if (n > 0 && out->d_common) MCS_HIP_CHECK(hipMemsetAsync(out->d_common, 0, 4 * (size_t)n, st));
    if (n > 0 && out->d_score) {
      // -0.0 per slot, as the scan writes for a keyframe that shares nothing
      hipLaunchKernelGGL(k_scan, dim3((n + kWaves - 1) / kWaves), dim3(kBlock), 0, st, db->word, db->value, db->ptr,
                         db->alive, (const int32_t*)nullptr, n, 0, 0, db->table, 0,
                         Query{query->d_word, query->d_value, query->d_n, 0}, db->s_common, db->s_minword,
                         out->d_score);
      MCS_HIP_CHECK(hipGetLastError());
    }
    return MCS_OK;
  }
  const Query q{query->d_word, query->d_value, query->d_n, query->cap};
  const int gq = (query->cap + kBlock - 1) / kBlock, gs = (n + kBlock - 1) / kBlock;
  MCS_HIP_CHECK(hipMemsetAsync(db->stats, 0, 8, st));
  hipLaunchKernelGGL(k_table, dim3(gq), dim3(kBlock), 0, st, q, db->table, db->n_words, 1);
  hipLaunchKernelGGL(k_scan, dim3((n + kWaves - 1) / kWaves), dim3(kBlock), 0, st, db->word, db->value, db->ptr,
                     db->alive, (const int32_t*)nullptr, n, n, db->acct.max_entries, db->table, db->n_words, q,
                     db->s_common, db->s_minword, db->s_score);
  const int k = loop ? 0 : 1;
  hipLaunchKernelGGL(k_classify, dim3(gs), dim3(kBlock), 0, st, loop, n, qid, d_connected, db->s_common,
                     db->s_minword, db->s_score, db->query[k], db->words[k], db->key_in, db->first, db->stats,
                     out->d_common, out->d_score);
  size_t b = 0;
  MCS_HIP_CHECK(rocprim::radix_sort_keys(nullptr, b, db->key_in, db->key_out, (size_t)n, 0, 64, st));
  if (b > db->tmp_bytes) { set_error("kfdb detect: sort storage above the database's"); return MCS_ERR_CAPACITY; }
  b = db->tmp_bytes;
  MCS_HIP_CHECK(rocprim::radix_sort_keys(db->tmp, b, db->key_in, db->key_out, (size_t)n, 0, 64, st));
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, loop, n, qid, d_min_score, d_neigh, db->key_out,
                     db->s_score, db->query[k], db->words[k], db->score[k], db->first, db->acc, db->best, db->in_sm,
                     db->stats, out->d_candidates, out->cap, out->d_n_candidates);
  hipLaunchKernelGGL(k_table, dim3(gq), dim3(kBlock), 0, st, q, db->table, db->n_words, 0);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

}  // namespace kfdb
}  // namespace mcs

using namespace mcs;
using namespace mcs::kfdb;

extern "C" {

int mcs_kfdb_create_n(int32_t device, int32_t n_words, int32_t scoring, int32_t max_keyframes,
                      int32_t max_entries, mcs_kfdb** out) {
  if (!out) return host::bad_arg("kfdb create: null out");
  *out = nullptr;
  if (n_words < 0 || scoring < 0 || scoring > 5 || max_keyframes < 1 || max_entries < 1)
    return host::bad_arg("kfdb create: need n_words >= 0, a DBoW2 scoring type, max_keyframes >= 1 and max_entries >= 1");
  if (scoring != 0) {
    set_error("kfdb create: only L1 scoring (scoringType 0) is built");
    return MCS_ERR_UNSUPPORTED;
  }
  if (int rc = host::open_device(device, "kfdb create")) return rc;
  auto* db = new (std::nothrow) mcs_kfdb();
  if (!db) return MCS_ERR_ARG;
  db->device = device;
  db->n_words = n_words;
  db->acct.max_keyframes = max_keyframes;
  db->acct.max_entries = max_entries;
  const size_t K = (size_t)max_keyframes, E = (size_t)max_entries, W = (size_t)std::max(n_words, 1);
  hipError_t e = hipSuccess;
  auto get = [&](auto** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc((void**)p, bytes);
  };
  get(&db->word, 4 * E); get(&db->value, 8 * E); get(&db->ptr, 4 * (K + 1)); get(&db->alive, K);
  for (int k = 0; k < 2; k++) { get(&db->query[k], 8 * K); get(&db->words[k], 4 * K); get(&db->score[k], 8 * K); }
  get(&db->table, 4 * W);
  get(&db->s_common, 4 * K); get(&db->s_minword, 4 * K); get(&db->s_score, 8 * K);
  get(&db->key_in, 8 * K); get(&db->key_out, 8 * K); get(&db->first, 4 * K); get(&db->acc, 8 * K);
  get(&db->best, 4 * K); get(&db->in_sm, K); get(&db->stats, 8);
  if (e == hipSuccess) e = rocprim::radix_sort_keys(nullptr, db->tmp_bytes, db->key_in, db->key_out, K, 0, 64,
                                                    (hipStream_t)0);
  db->tmp_bytes = std::max<size_t>(db->tmp_bytes, 16);
  get(&db->tmp, db->tmp_bytes);
  if (e == hipSuccess) e = hipMemset(db->table, 0xFF, 4 * W);
  if (e == hipSuccess) e = hipMemset(db->ptr, 0, 4 * (K + 1));
  if (e == hipSuccess) e = hipMemset(db->alive, 0, K);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    mcs_kfdb_destroy(db);
    set_hip_error(e, "kfdb create", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = db;
  return MCS_OK;
}

int mcs_kfdb_create(int32_t device, const mcs_vocab* voc, int32_t max_keyframes, int32_t max_entries,
                    mcs_kfdb** out) {
  int32_t info[6];
  if (!out) return host::bad_arg("kfdb create: null out");
  *out = nullptr;
  if (!voc || mcs_vocab_info(voc, info) != MCS_OK) return host::bad_arg("kfdb create: null vocabulary");
  return mcs_kfdb_create_n(device, info[5], info[2], max_keyframes, max_entries, out);
}

void mcs_kfdb_destroy(mcs_kfdb* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  void* bufs[] = {db->word, db->value, db->ptr, db->alive, db->query[0], db->query[1], db->words[0], db->words[1],
                  db->score[0], db->score[1], db->table, db->s_common, db->s_minword, db->s_score, db->key_in,
                  db->key_out, db->first, db->acc, db->best, db->in_sm, db->stats, db->tmp};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  delete db;
}

int32_t mcs_kfdb_size(const mcs_kfdb* db) { return db ? db->acct.n_added : 0; }

int mcs_kfdb_add_device(mcs_kfdb* db, const uint32_t* d_bow_word, const double* d_bow_value,
                        const int32_t* d_bow_n, int32_t n_upper, double reloc_score_init, int32_t* slot,
                        void* stream) {
  if (!db || !slot || !d_bow_n || n_upper < 0 || (n_upper > 0 && (!d_bow_word || !d_bow_value)))
    return host::bad_arg("kfdb add: bad arguments");
  int32_t s = -1;
  if (int rc = db->acct.reserve(n_upper, &s)) {
    set_error("kfdb add: max_keyframes or max_entries reached");
    return rc;
  }
  *slot = s;
  MCS_HIP_CHECK(hipSetDevice(db->device));
  hipLaunchKernelGGL(k_add, dim3(std::max(1, (n_upper + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_bow_word, d_bow_value, d_bow_n, n_upper, s, db->acct.max_entries, reloc_score_init, db->word,
                     db->value, db->ptr, db->alive, db->query[0], db->words[0], db->score[0], db->query[1],
                     db->words[1], db->score[1]);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_kfdb_erase(mcs_kfdb* db, int32_t slot, void* stream) {
  if (!db || !db->acct.has(slot)) return host::bad_arg("kfdb erase: no such slot");
  MCS_HIP_CHECK(hipSetDevice(db->device));
  MCS_HIP_CHECK(hipMemsetAsync(db->alive + slot, 0, 1, (hipStream_t)stream));
  return MCS_OK;
}

int mcs_kfdb_clear(mcs_kfdb* db, void* stream) {
  if (!db) return host::bad_arg("kfdb clear: null database");
  MCS_HIP_CHECK(hipSetDevice(db->device));
  db->acct.clear();
  MCS_HIP_CHECK(hipMemsetAsync(db->alive, 0, (size_t)db->acct.max_keyframes, (hipStream_t)stream));
  MCS_HIP_CHECK(hipMemsetAsync(db->ptr, 0, 4 * ((size_t)db->acct.max_keyframes + 1), (hipStream_t)stream));
  return MCS_OK;
}

int mcs_kfdb_min_score_device(mcs_kfdb* db, const mcs_kfdb_query* query, const int32_t* d_slots, int32_t n,
                              double* d_min_score, void* stream) {
  if (!db || !d_min_score || n < 0 || (n > 0 && !d_slots)) return host::bad_arg("kfdb min_score: bad arguments");
  if (int rc = check_query(query, "kfdb min_score")) return rc;
  if (n > db->acct.max_keyframes) return host::bad_arg("kfdb min_score: more slots than max_keyframes");
  MCS_HIP_CHECK(hipSetDevice(db->device));
  hipStream_t st = (hipStream_t)stream;
  const Query q{query->d_word, query->d_value, query->d_n, query->cap};
  const int gq = (query->cap + kBlock - 1) / kBlock;
  if (n > 0 && query->cap > 0) {
    hipLaunchKernelGGL(k_table, dim3(gq), dim3(kBlock), 0, st, q, db->table, db->n_words, 1);
    hipLaunchKernelGGL(k_scan, dim3((n + kWaves - 1) / kWaves), dim3(kBlock), 0, st, db->word, db->value, db->ptr,
                       db->alive, d_slots, n, db->acct.n_added, db->acct.max_entries, db->table, db->n_words, q,
                       db->s_common, db->s_minword, db->s_score);
    hipLaunchKernelGGL(k_table, dim3(gq), dim3(kBlock), 0, st, q, db->table, db->n_words, 0);
  } else if (n > 0) {   // an empty query scores -0.0 against everything
    hipLaunchKernelGGL(k_scan, dim3((n + kWaves - 1) / kWaves), dim3(kBlock), 0, st, db->word, db->value, db->ptr,
                       db->alive, d_slots, n, 0, 0, db->table, 0, q, db->s_common, db->s_minword, db->s_score);
  }
  hipLaunchKernelGGL(k_min_score, dim3(1), dim3(kBlock), 0, st, db->s_score, d_slots, n,
                     db->acct.n_added, d_min_score);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_kfdb_detect_loop_device(mcs_kfdb* db, const mcs_kfdb_query* query, int64_t query_id,
                                const uint8_t* d_connected, const double* d_min_score, const int32_t* d_neigh,
                                const mcs_kfdb_result* out, void* stream) {
  return detect(db, query, query_id, d_connected, d_min_score, d_neigh, out, 1, stream);
}

int mcs_kfdb_detect_reloc_device(mcs_kfdb* db, const mcs_kfdb_query* query, int64_t query_id,
                                 const int32_t* d_neigh, const mcs_kfdb_result* out, void* stream) {
  return detect(db, query, query_id, nullptr, nullptr, d_neigh, out, 0, stream);
}

int mcs_kfdb_members_device(const mcs_kfdb* db, int64_t* d_loop_query, int32_t* d_loop_words, double* d_loop_score,
                            int64_t* d_reloc_query, int32_t* d_reloc_words, double* d_reloc_score, void* stream) {
  if (!db) return host::bad_arg("kfdb members: null database");
  MCS_HIP_CHECK(hipSetDevice(db->device));
  const size_t n = (size_t)db->acct.n_added;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return MCS_OK;
  if (d_loop_query) MCS_HIP_CHECK(hipMemcpyAsync(d_loop_query, db->query[0], 8 * n, hipMemcpyDeviceToDevice, st));
  if (d_loop_words) MCS_HIP_CHECK(hipMemcpyAsync(d_loop_words, db->words[0], 4 * n, hipMemcpyDeviceToDevice, st));
  if (d_loop_score) MCS_HIP_CHECK(hipMemcpyAsync(d_loop_score, db->score[0], 8 * n, hipMemcpyDeviceToDevice, st));
  if (d_reloc_query) MCS_HIP_CHECK(hipMemcpyAsync(d_reloc_query, db->query[1], 8 * n, hipMemcpyDeviceToDevice, st));
  if (d_reloc_words) MCS_HIP_CHECK(hipMemcpyAsync(d_reloc_words, db->words[1], 4 * n, hipMemcpyDeviceToDevice, st));
  if (d_reloc_score) MCS_HIP_CHECK(hipMemcpyAsync(d_reloc_score, db->score[1], 8 * n, hipMemcpyDeviceToDevice, st));
  return MCS_OK;
}

// ---- host-buffer forms: argument checks before any device use, then upload, run, download

static int host_query_check(const mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                            const char* who) {
  static thread_local char msg[128];
  const char* err = nullptr;
  if (!db) err = "null database";
  else if (q_n < 0) err = "negative query length";
  else if (q_n > 0 && (!q_word || !q_value)) err = "null query buffers";
  if (!err) return MCS_OK;
  std::snprintf(msg, sizeof msg, "%s: %s", who, err);
  return host::bad_arg(msg);
}

int mcs_kfdb_add(mcs_kfdb* db, const uint32_t* bow_word, const double* bow_value, int32_t n,
                 double reloc_score_init, int32_t* slot) {
  if (int rc = host_query_check(db, bow_word, bow_value, n, "kfdb add")) return rc;
  if (!slot) return host::bad_arg("kfdb add: null slot");
  if (int rc = host::open_device(db->device, "kfdb add")) return rc;
  host::DevBufs B;
  const uint32_t* d_w = B.up(bow_word, (size_t)n);
  const double* d_v = B.up(bow_value, (size_t)n);
  const int32_t* d_n = B.up(&n, 1);
  if (B.err != hipSuccess) { set_hip_error(B.err, "kfdb add", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (int rc = mcs_kfdb_add_device(db, d_w, d_v, d_n, n, reloc_score_init, slot, nullptr)) return rc;
  MCS_HIP_CHECK(hipStreamSynchronize(nullptr));   // the staging buffers go with this call
  return MCS_OK;
}

int mcs_kfdb_min_score(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                       const int32_t* slots, int32_t n, double* min_score) {
  if (int rc = host_query_check(db, q_word, q_value, q_n, "kfdb min_score")) return rc;
  if (n < 0 || (n > 0 && !slots) || !min_score) return host::bad_arg("kfdb min_score: bad slot list or output");
  if (int rc = host::open_device(db->device, "kfdb min_score")) return rc;
  host::DevBufs B;
  const mcs_kfdb_query q{B.up(q_word, (size_t)q_n), B.up(q_value, (size_t)q_n), B.up(&q_n, 1), q_n};
  const int32_t* d_slots = B.up(slots, (size_t)n);
  double* d_min = B.alloc<double>(1);
  int rc = MCS_OK;
  if (B.err == hipSuccess) rc = mcs_kfdb_min_score_device(db, &q, d_slots, n, d_min, nullptr);
  if (rc == MCS_OK) B.down(min_score, d_min, 1);
  if (B.err != hipSuccess) { set_hip_error(B.err, "kfdb min_score", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return rc;
}

static int host_detect(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n, int64_t query_id,
                       const uint8_t* connected, double min_score, const int32_t* neigh, int32_t* candidates,
                       int32_t cap, int32_t* n_candidates, int32_t* common, double* score, int loop) {
  const char* who = loop ? "kfdb detect_loop" : "kfdb detect_reloc";
  if (int rc = host_query_check(db, q_word, q_value, q_n, who)) return rc;
  const size_t n = (size_t)db->acct.n_added;
  if (cap < 0 || !n_candidates || (cap > 0 && !candidates)) return host::bad_arg("kfdb detect: bad candidate buffers");
  if (n > 0 && (!neigh || (loop && !connected))) return host::bad_arg("kfdb detect: null connected / neighbours");
  if (int rc = host::open_device(db->device, who)) return rc;
  host::DevBufs B;
  const mcs_kfdb_query q{B.up(q_word, (size_t)q_n), B.up(q_value, (size_t)q_n), B.up(&q_n, 1), q_n};
  const uint8_t* d_conn = loop ? B.up(connected, n) : nullptr;
  const double* d_min = loop ? B.up(&min_score, 1) : nullptr;
  const int32_t* d_neigh = B.up(neigh, n * MCS_KFDB_NEIGH);
  mcs_kfdb_result r{};
  r.d_candidates = B.alloc<int32_t>((size_t)cap);
  r.cap = cap;
  r.d_n_candidates = B.alloc<int32_t>(1);
  r.d_common = common ? B.alloc<int32_t>(n) : nullptr;
  r.d_score = score ? B.alloc<double>(n) : nullptr;
  int rc = MCS_OK;
  if (B.err == hipSuccess)
    rc = loop ? mcs_kfdb_detect_loop_device(db, &q, query_id, d_conn, d_min, d_neigh, &r, nullptr)
              : mcs_kfdb_detect_reloc_device(db, &q, query_id, d_neigh, &r, nullptr);
  if (rc == MCS_OK) {
    B.down(n_candidates, r.d_n_candidates, 1);
    if (B.err == hipSuccess) B.down(candidates, r.d_candidates, (size_t)std::min(std::max(*n_candidates, 0), cap));
    B.down(common, r.d_common, n);
    B.down(score, r.d_score, n);
  }
  if (B.err != hipSuccess) { set_hip_error(B.err, who, __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (rc == MCS_OK && *n_candidates > cap) {
    set_error("kfdb detect: more candidates than cap; the first cap are returned");
    return MCS_ERR_CAPACITY;
  }
  return rc;
}

int mcs_kfdb_detect_loop(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                         int64_t query_id, const uint8_t* connected, double min_score, const int32_t* neigh,
                         int32_t* candidates, int32_t cap, int32_t* n_candidates, int32_t* common, double* score) {
  return host_detect(db, q_word, q_value, q_n, query_id, connected, min_score, neigh, candidates, cap, n_candidates,
                     common, score, 1);
}

int mcs_kfdb_detect_reloc(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                          int64_t query_id, const int32_t* neigh, int32_t* candidates, int32_t cap,
                          int32_t* n_candidates, int32_t* common, double* score) {
  return host_detect(db, q_word, q_value, q_n, query_id, nullptr, 0.0, neigh, candidates, cap, n_candidates, common,
                     score, 0);
}

}  // extern "C"
