// Host side of the keyframe database's bookkeeping: the slot counter and the capacity account.
// The lengths of the stored BowVectors are device data, so the host accounts every add with the
// caller's upper bound; the packed arrays can then never overflow, whatever the device counts say.
// Plain C++ (no HIP), so the stand-alone host checks compile it as it is.
#pragma once
#include <cstdint>
#include "../../include/mcs_common.h"

namespace mcs {
namespace kfdb {

struct Account {
  int32_t max_keyframes = 0, max_entries = 0;
  int32_t n_added = 0;      // slots handed out; a slot is never reused
  int64_t entries = 0;      // sum of the n_upper of every add

  // MCS_OK and *slot, or MCS_ERR_ARG / MCS_ERR_CAPACITY with nothing changed
  int reserve(int32_t n_upper, int32_t* slot) {
    if (n_upper < 0 || !slot) return MCS_ERR_ARG;
    if (n_added >= max_keyframes || entries + n_upper > (int64_t)max_entries) return MCS_ERR_CAPACITY;
    *slot = n_added++;
    entries += n_upper;
    return MCS_OK;
  }
  bool has(int32_t slot) const { return slot >= 0 && slot < n_added; }
  void clear() { n_added = 0; entries = 0; }
};

}  // namespace kfdb
}  // namespace mcs
