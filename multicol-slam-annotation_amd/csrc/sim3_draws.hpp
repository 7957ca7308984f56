// The sample draws of cSim3Solver::iterate (reference src/cSim3Solver.cpp:202-222) as integers:
// the three dis(gen) values of an iteration -> the three correspondence indices.  Plain C++ with
// no dependency, so a stand-alone program can include it (tests/cpp/sim3solver_draws.cpp).
#pragma once
#include <cstdint>

namespace mcs {

// vAvailableIndices starts as 0 .. n-1; the swap is written to the drawn VALUE (:220) and the
// distribution stays 0 .. n-1 while the vector shrinks, so a draw can read at or past the current
// size: the vector is an array of n whose popped elements keep their value.  Only two writes are
// ever read back, so two overrides stand for the array.  0 = ok, -1 = n < 3 or a draw outside [0, n).
inline int sim3_draw_samples(int32_t n, const int32_t* draws, int32_t n_its, int32_t* samples) {
  if (n < 3) return -1;
  for (int64_t i = 0; i < 3 * (int64_t)n_its; i++)
    if (draws[i] < 0 || draws[i] >= n) return -1;
  for (int32_t it = 0; it < n_its; it++) {
    int32_t pos[2] = {-1, -1}, val[2] = {0, 0}, size = n;
    auto at = [&](int32_t i) { return i == pos[1] ? val[1] : i == pos[0] ? val[0] : i; };
    for (int j = 0; j < 3; j++) {
      const int32_t idx = at(draws[3 * (int64_t)it + j]);
      samples[3 * (int64_t)it + j] = idx;
      if (j < 2) { val[j] = at(size - 1); pos[j] = idx; }      // vAvailableIndices[idx] = back()
      size--;                                                  // pop_back()
    }
  }
  return 0;
}

}  // namespace mcs
