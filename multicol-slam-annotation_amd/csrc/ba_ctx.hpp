// Host side of a BA context: the device context with its cached buffers and pinned staging,
// the packed problem upload, the polling waits and the sharded exchange layout.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/mcs_ba.h"
#include "ba_dev.hpp"
#include "ba_structure.hpp"
#include "host_util.hpp"
#include "ldlt.hpp"

using namespace mcs;
using namespace mcs::ba;

// a host-pinned buffer that only grows
struct PinnedStage {
  unsigned flags;
  uint8_t* p = nullptr;
  size_t cap = 0;
  uint8_t* get(size_t bytes) {
    if (bytes > cap) {
      release();
      const size_t want = std::max(bytes, (size_t)1 << 20);
      if (hipHostMalloc((void**)&p, want, flags) != hipSuccess) return p = nullptr;
      cap = want;
    }
    return p;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
  }
};

struct mcs_ba_ctx {
  int device = 0;
  HostStruct hs;
  // host threads for config-E-sized calls (structure build, staging copy); made on the first
  // call with at least kParMinEdges edges.  MCS_HOST_THREADS: their number (default 8, 1: off)
  std::unique_ptr<mcs::HostPool> pool;
  mcs::HostPool* pool_for(int n_edges) {
    if (n_edges < kParMinEdges) return nullptr;
    if (!pool) {
      const char* e = std::getenv("MCS_HOST_THREADS");
      int t = e ? std::atoi(e) : 8;
      const int hw = (int)std::thread::hardware_concurrency();
      if (hw > 0) t = std::min(t, hw);
      pool.reset(new mcs::HostPool(std::max(1, std::min(t, 16))));
    }
    return pool->size() > 1 ? pool.get() : nullptr;
  }
  hipStream_t st = nullptr;
  // Device buffers are cached across calls: the driver requests them in the same order
  // every call, so request k reuses slot k when it is large enough (grow-only).
  std::vector<void*> bufs;
  std::vector<size_t> caps;
  size_t next = 0;
  double* pinned = nullptr;   // host-pinned readback scalars
  int32_t* pinned_i = nullptr;
  TrialSig* sig = nullptr;    // host-coherent trial outcome (k_reduce3)
  uint64_t sig_seq = 0;
  LmSig* lsig = nullptr;      // host-coherent progress of the device-driven LM (k_edges_end)
  uint64_t lsig_seq = 0;
  void* pinned_ctl = nullptr; // host-pinned readback of the final LmCtl
  // host-pinned staging of a call's packed problem upload; mapped: k_lba_out writes LocalBA's
  // results into it directly
  PinnedStage stage{hipHostMallocMapped};
  // second staging buffer (threaded calls): the structure arrays, filled while the problem
  // arrays' copy out of `stage` may still be in flight
  PinnedStage stage2{hipHostMallocDefault};
  // optional stage timing (mcs_ba_enable_timing): HIP events on st around each stage,
  // accumulated after the per-trial synchronisation the LM control needs anyway
  bool timing = false;
  // factorisation of multi-tile systems (mcs_ba_set_ldlt_mode): 0 banded pipeline where the
  // size allows it, 1 dense pipeline (band := T), 2 one panel launch per step
  int ldlt_mode = 0;
  // reduced system of the last setup (mcs_ba_read_solve_shape)
  int32_t shape_n = 0, shape_T = 0, shape_band = 0, shape_pipe = 0;
  hipEvent_t ev[8] = {};
  double acc_ms[MCS_BA_NSTAGES] = {};
  double host_ms[MCS_BA_NHOST] = {};   // host phases (mcs_ba_read_host_timing)
  int32_t host_calls = 0;
  int32_t n_iter = 0, n_trial = 0, last_n = 0;
  void* alloc(size_t bytes) {
    bytes += 64;
    if (next < bufs.size() && caps[next] >= bytes) return bufs[next++];
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    if (next < bufs.size()) {
      (void)hipFree(bufs[next]);
      bufs[next] = p; caps[next] = bytes;
    } else {
      bufs.push_back(p); caps.push_back(bytes);
    }
    next++;
    return p;
  }
  void free_all() { next = 0; }   // recycle (buffers stay allocated)
  void release() {
    for (void* p : bufs) (void)hipFree(p);
    bufs.clear(); caps.clear(); next = 0;
  }
};

namespace {

// Wait for a stream by polling instead of a blocking synchronisation: the blocking wait may
// sleep and costs up to ~0.4 ms of wake-up latency at the end of a LocalBA call (measured in
// the bench's host phase "download": 0.12 - 0.52 ms for the same work).
static hipError_t spin_sync(hipStream_t st) {
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q != hipErrorNotReady) return q;
    for (int k = 0; k < 64; k++) __builtin_ia32_pause();
  }
}

// Wait for a signal a kernel on st releases into host-coherent memory: spin on done(), and every
// 1024 spins run each_query() and look at the stream, so that a failed launch cannot spin for
// ever (missing: the error when the stream drained without the signal; what: the HIP error's tag)
template <class Done, class Hook>
int spin_until(hipStream_t st, Done done, Hook each_query, const char* missing, const char* what) {
  for (uint32_t k = 1;; k++) {
    if (done()) return MCS_OK;
    __builtin_ia32_pause();   // spin politely: other ranks' threads may share this core
    if ((k & 1023) == 0) {
      each_query();
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) {
        if (done()) return MCS_OK;
        set_error(missing);
        return MCS_ERR_HIP;
      }
      if (q != hipErrorNotReady) { set_hip_error(q, what, __FILE__, __LINE__); return MCS_ERR_HIP; }
    }
  }
}

// The problem arrays of a call, packed into one device block through one pinned staging
// buffer and ONE host-to-device copy (some thirty pageable copies cost ~0.4 ms per call on a
// config-C LocalBA round).  add() records where each array's device pointer goes; flush()
// fills the pointers.
struct Packer {
  struct Item { void** dst; const void* src; size_t bytes, off; };
  std::vector<Item> items;
  size_t total = 0;
  template <typename D, typename T>
  void add(D** dst, const T* src, size_t n) {
    static_assert(sizeof(D) == sizeof(T), "element type");
    items.push_back({reinterpret_cast<void**>(const_cast<void*>(static_cast<const void*>(dst))), src,
                     src ? n * sizeof(T) : 0, total});
    total += (std::max<size_t>(1, n) * sizeof(T) + 255) & ~(size_t)255;
  }
  template <typename D, typename T>
  void add(D** dst, const std::vector<T>& v) { add(dst, v.data(), v.size()); }
  // second: into stage2, behind a first flush of this call (whose spin_sync already found the
  // previous call's copies done; the first flush's own copy may still be running)
  hipError_t flush(mcs_ba_ctx* c, mcs::HostPool* pool = nullptr, bool second = false) {
    uint8_t* d = (uint8_t*)c->alloc(std::max<size_t>(total, 256));
    if (!d) return hipErrorOutOfMemory;
    if (!second) {
      const hipError_t e = spin_sync(c->st);   // the staging buffer is free again
      if (e != hipSuccess) return e;
    }
    uint8_t* h = (second ? c->stage2 : c->stage).get(std::max<size_t>(total, 256));
    if (!h) return hipErrorOutOfMemory;
    for (const Item& it : items) *it.dst = d + it.off;
    if (pool && total >= ((size_t)4 << 20)) {
      // config E packs ~20 MB: the staging copy split by byte range over the host threads
      const int T = pool->size();
      pool->run([&](int t) {
        const size_t lo = total * t / T, hi = total * (t + 1) / T;
        for (const Item& it : items) {
          const size_t a = std::max(lo, it.off), b = std::min(hi, it.off + it.bytes);
          if (a < b) std::memcpy(h + a, (const uint8_t*)it.src + (a - it.off), b - a);
        }
      });
    } else {
      for (const Item& it : items)
        if (it.bytes) std::memcpy(h + it.off, it.src, it.bytes);
    }
    return total ? hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, c->st) : hipSuccess;
  }
};

unsigned gb(int n) { return (unsigned)std::max(1, (n + 255) / 256); }

// Exchange-buffer layout (offsets in doubles) for T tiles and np active poses: [bs | S tiles |
// hdiag | bpf | scalars]; bs first so that bs and the leading (non-zero) diagonals of S are one
// range.  The head of the buffer is reused for the structure exchange (pose activity counts)
// before T is known.
struct XLayout {
  size_t S, bs, hdiag, bpf, sc, total;
  XLayout(int T, int np) {
    bs = 0;
    S = (size_t)ldlt::TB * T;
    hdiag = S + ldlt::tile_doubles(T);
    bpf = hdiag + 6 * (size_t)np;
    sc = bpf + 6 * (size_t)np;
    total = sc + 16;
  }
};

int64_t xchg_doubles(int32_t n_poses) {
  const int np = std::max(0, n_poses);
  const XLayout x(ldlt::tiles_for(std::max(1, 6 * np)), np);
  return (int64_t)std::max<size_t>(x.total, (size_t)np + 16);
}

struct Shard {
  int rank = 0, world = 1;
  double* xchg = nullptr;
  mcs_ba_allreduce_fn fn = nullptr;
  void* user = nullptr;
  bool ordered = false;   // stream_ordered: the callback enqueues on st, no host drain
};

// host phase clock: add the time since the previous mark to c->host_ms[k]
struct HostClock {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(double* acc, int k) {
    const auto n = std::chrono::steady_clock::now();
    acc[k] += std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
  }
};

}  // namespace
