// CPU baseline of the keyframe database queries for tools/bench_kfdb.py: plain single-thread C++
// with a real inverted file (word -> keyframes in add order), so a query touches only the entries
// of the words it holds.  Own code after the algorithm (list the keyframes that share a word, score
// those above 0.8 x the best shared-word count with the L1 score, accumulate over the ten best
// covisibles, keep what comes within 0.75 of the best, first occurrence only); the members per
// keyframe behave as the device's, so both paths can be played through the same query sequence.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Kf {
  std::vector<uint32_t> w;
  std::vector<double> v;
  int64_t query[2] = {0, 0};
  int words[2] = {0, 0};
  double score[2] = {0.0, 0.0};
};

struct Db {
  std::vector<std::vector<int>> inv;
  std::vector<Kf> kfs;
  std::vector<int> mark;
};

double l1(const uint32_t* w1, const double* v1, int n1, const Kf& k) {
  double s = 0.0;
  int i = 0, j = 0;
  const int n2 = (int)k.w.size();
  while (i < n1 && j < n2) {
    if (w1[i] == k.w[j]) {
      s += std::fabs(v1[i] - k.v[j]) - std::fabs(v1[i]) - std::fabs(k.v[j]);
      ++i; ++j;
    } else if (w1[i] < k.w[j]) {
      ++i;
    } else {
      ++j;
    }
  }
  return -s / 2.0;
}

}  // namespace

extern "C" {

void* kfdb_cpu_create(int n_words) {
  Db* d = new Db();
  d->inv.resize(n_words);
  return d;
}

void kfdb_cpu_destroy(void* h) { delete static_cast<Db*>(h); }

int kfdb_cpu_add(void* h, const uint32_t* w, const double* v, int n) {
  Db& d = *static_cast<Db*>(h);
  const int slot = (int)d.kfs.size();
  d.kfs.emplace_back();
  d.kfs.back().w.assign(w, w + n);
  d.kfs.back().v.assign(v, v + n);
  for (int i = 0; i < n; i++)
    if (w[i] < d.inv.size()) d.inv[w[i]].push_back(slot);
  d.mark.push_back(-1);
  return slot;
}

double kfdb_cpu_min_score(void* h, const uint32_t* qw, const double* qv, int qn, const int* slots, int n) {
  Db& d = *static_cast<Db*>(h);
  double m = 1.0;
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= (int)d.kfs.size()) continue;
    const double s = l1(qw, qv, qn, d.kfs[slots[i]]);
    if (s < m) m = s;
  }
  return m;
}

// loop = 1: DetectLoopCandidates, 0: DetectRelocalisationCandidates -> number of candidates
int kfdb_cpu_detect(void* h, int loop, const uint32_t* qw, const double* qv, int qn, int64_t qid,
                    const uint8_t* connected, double min_score, const int* neigh, int* cand) {
  Db& d = *static_cast<Db*>(h);
  const int m = loop ? 0 : 1, N = (int)d.kfs.size();
  std::vector<int> list;
  for (int i = 0; i < qn; i++) {
    if (qw[i] >= d.inv.size()) continue;
    for (int s : d.inv[qw[i]]) {
      Kf& k = d.kfs[s];
      if (k.query[m] != qid) {
        k.words[m] = 0;
        if (!loop || !connected[s]) {
          k.query[m] = qid;
          list.push_back(s);
        }
      }
      k.words[m]++;
    }
  }
  if (list.empty()) return 0;
  int max_common = 0;
  for (int s : list) max_common = d.kfs[s].words[m] > max_common ? d.kfs[s].words[m] : max_common;
  const int min_common = (int)((double)max_common * 0.8);
  std::vector<int> scored;
  for (int s : list) {
    Kf& k = d.kfs[s];
    if (k.words[m] > min_common) {
      k.score[m] = l1(qw, qv, qn, k);
      if (!loop || k.score[m] >= min_score) scored.push_back(s);
    }
  }
  if (scored.empty()) return 0;
  double best_acc = loop ? min_score : 0.0;
  std::vector<double> acc(scored.size());
  std::vector<int> best(scored.size());
  for (size_t i = 0; i < scored.size(); i++) {
    const int s = scored[i];
    double a = d.kfs[s].score[m], bs = a;
    int bk = s;
    for (int j = 0; j < 10; j++) {
      const int s2 = neigh[(size_t)s * 10 + j];
      if (s2 < 0 || s2 >= N) continue;
      const Kf& k2 = d.kfs[s2];
      if (k2.query[m] != qid || (loop && !(k2.words[m] > min_common))) continue;
      a += k2.score[m];
      if (k2.score[m] > bs) { bk = s2; bs = k2.score[m]; }
    }
    acc[i] = a;
    best[i] = bk;
    if (a > best_acc) best_acc = a;
  }
  const double retain = 0.75 * best_acc;
  int n = 0;
  for (size_t i = 0; i < scored.size(); i++)
    if (acc[i] > retain && d.mark[best[i]] != 1) { d.mark[best[i]] = 1; cand[n++] = best[i]; }
  for (int i = 0; i < n; i++) d.mark[cand[i]] = -1;
  return n;
}

}  // extern "C"
