// The host planner of the block-sparse LDL^T of the essential graph (essential_graph_plan.hpp):
// the graph of the free keyframes from the edge list, a nested-dissection ordering by breadth-first
// level sets, the supernodal symbolic factorisation and the schedule.  Pure host code, no HIP.
//
// Everything is a function of the set of unordered pairs alone: neighbours are sorted and made
// unique before anything looks at them and every tie goes to the smaller keyframe index, so a
// permuted edge list gives the same plan to the byte (SparsePlan::digest).
//
// Ordering.  A set of keyframes is split into its connected components, by smallest member.  A
// component of at most `leaf` keyframes is a leaf, in natural order.  Otherwise level sets are
// taken from a pseudo-peripheral keyframe (three sweeps, each from the smallest keyframe of the
// last level of the sweep before); with fewer than three levels the component is a leaf whatever
// its size; else the level that balances the two sides best (the earlier on a tie) is the
// separator, the levels before it and after it are ordered first, by the same rule, and the
// separator last.  On a chain with k neighbours a level is k keyframes; on a ring a level is the
// two arcs at one distance from the start, which is what cuts a ring.
#include "essential_graph_plan.hpp"
#include "essential_graph_math.hpp"
#include <algorithm>
#include <cstring>

namespace mcs {
namespace esg {
namespace {

struct Dissect {
  const std::vector<int32_t>& ap;      // adjacency of the free keyframes, CSR, ascending
  const std::vector<int32_t>& ai;
  int leaf;
  std::vector<int32_t> mark, dist, order, sn_end;
  int stamp = 0;

  Dissect(const std::vector<int32_t>& p, const std::vector<int32_t>& i, int n, int lf)
      : ap(p), ai(i), leaf(lf), mark(n, -1), dist(n, -1) {}

  void emit(const std::vector<int32_t>& vs) {
    order.insert(order.end(), vs.begin(), vs.end());
    sn_end.push_back((int32_t)order.size());
  }

  // level sets of the keyframes marked `id` from root -> vertices in visiting order, level starts
  void sweep(int root, int id, std::vector<int32_t>& seq, std::vector<int32_t>& lv) {
    seq.clear(); lv.clear();
    seq.push_back(root);
    dist[root] = 0;
    lv.push_back(0);
    size_t head = 0;
    while (head < seq.size()) {
      const size_t end = seq.size();
      for (; head < end; head++) {
        const int a = seq[head];
        for (int k = ap[a]; k < ap[a + 1]; k++) {
          const int b = ai[k];
          if (mark[b] == id && dist[b] < 0) { dist[b] = dist[a] + 1; seq.push_back(b); }
        }
      }
      if (seq.size() > end) lv.push_back((int32_t)end);
    }
    lv.push_back((int32_t)seq.size());
    for (int a : seq) dist[a] = -1;
  }

  void run(std::vector<int32_t> vs) {            // ascending
    if (vs.empty()) return;
    const int id = ++stamp;
    for (int a : vs) mark[a] = id;
    std::vector<int32_t> seq, lv;
    sweep(vs[0], id, seq, lv);
    if (seq.size() < vs.size()) {                // components, by smallest member
      std::vector<std::vector<int32_t>> comps;
      const int done = ++stamp;
      size_t next = 0;
      for (;;) {
        for (int a : seq) mark[a] = done;
        std::sort(seq.begin(), seq.end());
        comps.push_back(seq);
        while (next < vs.size() && mark[vs[next]] == done) next++;
        if (next == vs.size()) break;
        sweep(vs[next], id, seq, lv);
      }
      for (auto& c : comps) run(std::move(c));
      return;
    }
    if ((int)vs.size() <= leaf) { emit(vs); return; }
    for (int it = 0; it < 2; it++) {
      const int last = (int)lv.size() - 2;
      const int root = *std::min_element(seq.begin() + lv[last], seq.begin() + lv[last + 1]);
      sweep(root, id, seq, lv);
    }
    const int nlev = (int)lv.size() - 1;
    if (nlev < 3) { emit(vs); return; }
    int best = 1;
    long bestd = -1;
    for (int L = 1; L <= nlev - 2; L++) {
      const long d = std::labs((long)lv[L] - ((long)vs.size() - lv[L + 1]));
      if (bestd < 0 || d < bestd) { bestd = d; best = L; }
    }
    std::vector<int32_t> a(seq.begin(), seq.begin() + lv[best]), sep(seq.begin() + lv[best], seq.begin() + lv[best + 1]),
        b(seq.begin() + lv[best + 1], seq.end());
    std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end()); std::sort(sep.begin(), sep.end());
    run(std::move(a));
    run(std::move(b));
    emit(sep);
  }
};

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(const void* p, size_t bytes) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; i++) { h ^= c[i]; h *= 1099511628211ull; }
  }
  template <class T> void vec(const std::vector<T>& v) {
    const uint64_t n = v.size();
    add(&n, 8);
    if (n) add(v.data(), n * sizeof(T));
  }
};

}  // namespace

int plan_build(int n_kf, int loop, const int32_t* edges, int E, int leaf, int block, SparsePlan* out, std::string* err) {
  auto fail = [&](int rc, const char* msg) { if (err) *err = msg; return rc; };
  if (!out || n_kf < 1 || E < 0 || (E > 0 && !edges) || loop < 0 || loop >= n_kf || block < 1)
    return fail(-1, "essential graph plan: bad argument");
  SparsePlan& p = *out;
  p = SparsePlan();
  p.N = n_kf; p.loop = loop; p.leaf = leaf > 0 ? leaf : kPlanDefaultLeaf;
  const int n = p.n = n_kf - 1;
  const int B = block;

  // the graph of the free keyframes: each unordered pair once
  std::vector<int64_t> pairs;
  pairs.reserve((size_t)E);
  for (int e = 0; e < E; e++) {
    const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
    if (v0 < 0 || v0 >= n_kf || v1 < 0 || v1 >= n_kf || v0 == v1)
      return fail(-1, "essential graph plan: an edge names no keyframe or joins one to itself");
    const int u0 = free_index(v0, loop), u1 = free_index(v1, loop);
    if (u0 < 0 || u1 < 0) continue;
    pairs.push_back(((int64_t)std::min(u0, u1) << 32) | (uint32_t)std::max(u0, u1));
  }
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  std::vector<int32_t> ap((size_t)n + 1, 0), ai(2 * pairs.size());
  for (int64_t q : pairs) { ap[(q >> 32) + 1]++; ap[(q & 0xFFFFFFFF) + 1]++; }
  for (int i = 0; i < n; i++) ap[i + 1] += ap[i];
  {
    std::vector<int32_t> at(ap.begin(), ap.end() - 1);
    for (int64_t q : pairs) {
      const int a = (int)(q >> 32), b = (int)(q & 0xFFFFFFFF);
      ai[at[a]++] = b; ai[at[b]++] = a;
    }
    for (int i = 0; i < n; i++) std::sort(ai.begin() + ap[i], ai.begin() + ap[i + 1]);
  }

  // ordering and supernodes
  Dissect nd(ap, ai, n, p.leaf);
  {
    std::vector<int32_t> all(n);
    for (int i = 0; i < n; i++) all[i] = i;
    nd.run(std::move(all));
  }
  p.iperm = nd.order;
  p.perm.assign(n, 0);
  for (int c = 0; c < n; c++) p.perm[p.iperm[c]] = c;
  const int S = p.S = (int)nd.sn_end.size();
  p.col0.assign(S + 1, 0);
  for (int s = 0; s < S; s++) p.col0[s + 1] = nd.sn_end[s];
  p.sn_of.assign(n, 0);
  for (int s = 0; s < S; s++)
    for (int c = p.col0[s]; c < p.col0[s + 1]; c++) p.sn_of[c] = s;

  // symbolic factorisation: rows(s) = own columns, then the rows of A and of the children below them
  std::vector<std::vector<int32_t>> below(S);
  p.parent.assign(S, -1);
  p.rowptr.assign(S + 1, 0);
  p.blkoff.assign(S + 1, 0);
  int64_t blocks = 0, rows_total = 0;
  for (int s = 0; s < S; s++) {
    std::vector<int32_t>& st = below[s];         // holds what the children pushed
    const int c1 = p.col0[s + 1];
    for (int c = p.col0[s]; c < c1; c++) {
      const int a = p.iperm[c];
      for (int k = ap[a]; k < ap[a + 1]; k++)
        if (p.perm[ai[k]] >= c1) st.push_back(p.perm[ai[k]]);
    }
    std::sort(st.begin(), st.end());
    st.erase(std::unique(st.begin(), st.end()), st.end());
    st.erase(st.begin(), std::lower_bound(st.begin(), st.end(), c1));
    if (!st.empty()) {
      const int par = p.parent[s] = p.sn_of[st[0]];
      below[par].insert(below[par].end(), st.begin(), st.end());
    }
    const int64_t ns = c1 - p.col0[s], nr = ns + (int64_t)st.size();
    p.max_cols = std::max(p.max_cols, (int)ns);
    blocks += ns * nr;
    rows_total += nr;
    p.l_blocks += ns * (ns + 1) / 2 + ns * (int64_t)st.size();
    if (blocks * B * B * 8 > kPlanMaxBytes || rows_total > INT32_MAX / 64)
      return fail(-4, "essential graph plan: the pattern of L is above the plan's byte limit (1 GiB)");
    p.rowptr[s + 1] = (int32_t)rows_total;
    p.blkoff[s + 1] = (int32_t)blocks;
  }
  p.panel_blocks = blocks;
  p.row_blocks = rows_total;
  p.rows.resize((size_t)rows_total);
  for (int s = 0; s < S; s++) {
    int32_t* r = p.rows.data() + p.rowptr[s];
    for (int c = p.col0[s]; c < p.col0[s + 1]; c++) *r++ = c;
    for (int v : below[s]) *r++ = v;
  }

  // sources of every supernode, ascending, with the row maps
  std::vector<std::vector<int32_t>> src(S);      // triples s, p0, p1
  for (int s = 0; s < S; s++) {
    const int ns = p.col0[s + 1] - p.col0[s], nr = p.rowptr[s + 1] - p.rowptr[s];
    const int32_t* r = p.rows.data() + p.rowptr[s];
    for (int q = ns; q < nr;) {
      const int t = p.sn_of[r[q]];
      int q1 = q;
      while (q1 < nr && p.sn_of[r[q1]] == t) q1++;
      src[t].insert(src[t].end(), {s, q, q1});
      q = q1;
    }
  }
  p.srcptr.assign(S + 1, 0);
  for (int t = 0; t < S; t++) {
    const int32_t* rt = p.rows.data() + p.rowptr[t];
    const int nrt = p.rowptr[t + 1] - p.rowptr[t];
    const int64_t Wt = (int64_t)B * (p.col0[t + 1] - p.col0[t]), Mt = (int64_t)B * nrt;
    for (size_t k = 0; k < src[t].size(); k += 3) {
      const int s = src[t][k], p0 = src[t][k + 1], p1 = src[t][k + 2];
      const int32_t* rs = p.rows.data() + p.rowptr[s];
      const int nrs = p.rowptr[s + 1] - p.rowptr[s];
      p.src_s.push_back(s); p.src_p0.push_back(p0); p.src_p1.push_back(p1);
      if (p.relmap.size() > (size_t)INT32_MAX / 2)
        return fail(-4, "essential graph plan: the row maps are above the int32 index range");
      p.src_map.push_back((int32_t)p.relmap.size());
      int pos = 0;
      for (int q = p0; q < nrs; q++) {
        while (pos < nrt && rt[pos] < rs[q]) pos++;
        if (pos >= nrt || rt[pos] != rs[q]) return fail(-1, "essential graph plan: internal error (pattern not closed)");
        p.relmap.push_back(pos);
      }
      const int64_t Ws = (int64_t)B * (p.col0[s + 1] - p.col0[s]);
      p.flops += 3 * Ws * (int64_t)B * (nrs - p0) * B * (p1 - p0);
    }
    p.srcptr[t + 1] = (int32_t)p.src_s.size();
    for (int64_t c = 0; c < Wt; c++) p.flops += 3 * (Mt - c - 1) * (Wt - c);
  }

  // levels = heights in the supernodal tree
  p.level.assign(S, 0);
  for (int s = 0; s < S; s++)
    if (p.parent[s] >= 0) p.level[p.parent[s]] = std::max(p.level[p.parent[s]], p.level[s] + 1);
  p.levels = 0;
  for (int s = 0; s < S; s++) p.levels = std::max(p.levels, p.level[s] + 1);
  p.lvlptr.assign(p.levels + 1, 0);
  for (int s = 0; s < S; s++) p.lvlptr[p.level[s] + 1]++;
  for (int l = 0; l < p.levels; l++) p.lvlptr[l + 1] += p.lvlptr[l];
  p.lvlsn.assign(S, 0);
  {
    std::vector<int32_t> at(p.lvlptr.begin(), p.lvlptr.end() - 1);
    for (int s = 0; s < S; s++) p.lvlsn[at[p.level[s]]++] = s;
  }
  int top = p.levels;                            // the levels from `top` on hold one supernode each
  while (top > 0 && p.lvlptr[top] - p.lvlptr[top - 1] == 1) top--;
  for (int l = 0; l < top; l++) { p.launch_lo.push_back(l); p.launch_hi.push_back(l + 1); }
  if (top < p.levels) { p.launch_lo.push_back(top); p.launch_hi.push_back(p.levels); }

  // the blocks of A
  p.ablk.assign((size_t)blocks, 0);
  const SpView v = p.view();
  for (int c = 0; c < n; c++) p.ablk[find_block(v, c, c)] = 1;
  for (int64_t q : pairs) {
    const int a = p.perm[q >> 32], b = p.perm[q & 0xFFFFFFFF];
    const int blk = find_block(v, std::max(a, b), std::min(a, b));
    if (blk < 0) return fail(-1, "essential graph plan: internal error (a pair outside the pattern)");
    p.ablk[blk] = 1;
  }
  p.a_blocks = (int64_t)n + (int64_t)pairs.size();

  Fnv f;
  const int32_t head[6] = {p.N, p.loop, p.n, p.S, p.leaf, p.levels};
  f.add(head, sizeof head);
  f.vec(p.perm); f.vec(p.col0); f.vec(p.rowptr); f.vec(p.rows); f.vec(p.blkoff); f.vec(p.srcptr); f.vec(p.src_s);
  f.vec(p.src_p0); f.vec(p.src_p1); f.vec(p.src_map); f.vec(p.relmap); f.vec(p.parent); f.vec(p.level); f.vec(p.lvlsn);
  f.vec(p.ablk); f.vec(p.launch_lo); f.vec(p.launch_hi);
  p.digest = f.h;
  return 0;
}

}  // namespace esg
}  // namespace mcs
