// Single-thread CPU restatement of the two SearchByBoW loops (reference src/cORBmatcher.cpp
// :179-323 and :885-966, orientation check off) on flat arrays: the CPU baseline that
// tools/bench_bow_match.py times next to the GPU entries.  Same input file as bow_match_demo.
//
//   bow_match_cpu <in.bin> [repeats]   ->  one line "cpu_ms <median> nmatches <sum>"
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Frame {
  int n = 0;
  std::vector<uint8_t> desc, mask, has_mp;
  std::vector<float> angle;
  std::vector<uint32_t> fv_node, fv_feat;
  std::vector<int32_t> fv_ptr;
};

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static inline int dist(const uint8_t* a, const uint8_t* b, const uint8_t* ma, const uint8_t* mb, int bytes) {
  const uint64_t* x = (const uint64_t*)a; const uint64_t* y = (const uint64_t*)b;
  uint64_t d = 0;
  if (!ma) {
    for (int i = 0; i < bytes / 8; i++) d += __builtin_popcountll(x[i] ^ y[i]);
    return (int)d;
  }
  const uint64_t* p = (const uint64_t*)ma; const uint64_t* q = (const uint64_t*)mb;
  for (int i = 0; i < bytes / 8; i++) {
    const uint64_t v = x[i] ^ y[i];
    d += __builtin_popcountll(v & p[i]) + __builtin_popcountll(v & q[i]);
  }
  return (int)(d / 2);
}

static int bow_a(const Frame& K, const Frame& F, int bytes, int th, double ratio, std::vector<int32_t>& m) {
  m.assign(F.n, -1);
  int nm = 0;
  size_t a = 0, b = 0;
  const bool masked = !K.mask.empty();
  while (a < K.fv_node.size() && b < F.fv_node.size()) {
    if (K.fv_node[a] < F.fv_node[b]) { a++; continue; }
    if (K.fv_node[a] > F.fv_node[b]) { b++; continue; }
    for (int i = K.fv_ptr[a]; i < K.fv_ptr[a + 1]; i++) {
      const uint32_t ik = K.fv_feat[i];
      if (!K.has_mp[ik]) continue;
      int b1 = INT_MAX, b2 = INT_MAX, bi = -1;
      for (int j = F.fv_ptr[b]; j < F.fv_ptr[b + 1]; j++) {
        const uint32_t jf = F.fv_feat[j];
        if (m[jf] >= 0) continue;
        const int d = dist(&K.desc[(size_t)ik * bytes], &F.desc[(size_t)jf * bytes],
                           masked ? &K.mask[(size_t)ik * bytes] : nullptr,
                           masked ? &F.mask[(size_t)jf * bytes] : nullptr, bytes);
        if (d < b1) { b2 = b1; b1 = d; bi = (int)jf; }
        else if (d < b2) b2 = d;
      }
      if (b1 <= th && (double)b1 < ratio * (double)b2) { m[bi] = (int32_t)ik; nm++; }
    }
    a++; b++;
  }
  return nm;
}

static int bow_b(const Frame& A, const Frame& B, int bytes, int th, double ratio, std::vector<int32_t>& m) {
  m.assign(A.n, -1);
  std::vector<uint8_t> taken(B.n, 0);
  const bool masked = !A.mask.empty();
  int nm = 0;
  for (int i1 = 0; i1 < A.n; i1++) {
    if (!A.has_mp[i1]) continue;
    int b1 = INT_MAX, b2 = INT_MAX, bi = -1;
    for (int i2 = 0; i2 < B.n; i2++) {
      if (taken[i2] || !B.has_mp[i2]) continue;
      const int d = dist(&A.desc[(size_t)i1 * bytes], &B.desc[(size_t)i2 * bytes],
                         masked ? &A.mask[(size_t)i1 * bytes] : nullptr,
                         masked ? &B.mask[(size_t)i2 * bytes] : nullptr, bytes);
      if (d < b1) { b2 = b1; b1 = d; bi = i2; }
      else if (d < b2) b2 = d;
    }
    if (b1 < th && (double)b1 < ratio * (double)b2) { m[i1] = bi; taken[bi] = 1; nm++; }
  }
  return nm;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s in.bin [repeats]\n", argv[0]); return 2; }
  const int reps = argc > 2 ? atoi(argv[2]) : 5;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[5];
  double ratio = 0;
  if (fread(h, 4, 5, f) != 5 || fread(&ratio, 8, 1, f) != 1) return 2;
  const int mode = h[0], bytes = h[1], th = h[2], nfr = h[4];
  std::vector<Frame> fr(nfr);
  for (auto& x : fr) {
    int32_t g[4];
    if (fread(g, 4, 4, f) != 4) return 2;
    x.n = g[0];
    const size_t n = g[0], m = g[2];
    bool ok = rd(f, x.desc, n * bytes);
    if (g[1]) ok = ok && rd(f, x.mask, n * bytes);
    ok = ok && rd(f, x.angle, n) && rd(f, x.has_mp, n) && rd(f, x.fv_node, m) && rd(f, x.fv_ptr, m ? m + 1 : 0) &&
         rd(f, x.fv_feat, (size_t)g[3]);
    if (!ok) return 2;
  }
  fclose(f);
  std::vector<double> ms;
  std::vector<int32_t> m;
  long total = 0;
  for (int r = 0; r < reps; r++) {
    total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 1; k < nfr; k++)
      total += mode == 0 ? bow_a(fr[k], fr[0], bytes, th, ratio, m) : bow_b(fr[0], fr[k], bytes, th, ratio, m);
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("cpu_ms %.4f nmatches %ld\n", ms[ms.size() / 2], total);
  return 0;
}
