// Which frames of a batch share a group of pack_pyr_units' waves (pyr_units.hpp): frames of
// one registered mask, G to a group.  The mask index of a frame lives on the device and may
// come in any order, so the rule is a stable counting sort by clamped mask index that one
// workgroup can run: per mask m its frames in ascending order fill the groups
// first_group[m] .. first_group[m] + ceil(count[m] / G) - 1, G to a group, the last one of a
// mask partly (absent slots hold -1).  ceil(F / G) + nmasks - 1 groups are always enough.
// The clamp and the group arithmetic are what k_pyr_groups (k_pyramid.hip) computes with;
// pyr_group_frames states the whole rule serially and is the reference that the kernel's
// parallel ranks are tested against (tests/cpp/pyr_packed_check.cpp holds it to a plain
// restatement, the GPU tests hold the kernel's groups to what it implies).  The library
// itself never calls it.
// No HIP include: __host__ __device__ under hipcc, inline under a host compiler.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCS_PYRG_FN __host__ __device__ inline
#else
#define MCS_PYRG_FN inline
#endif

namespace mcs {

// the clamp of k_pyr_rows and k_fast_rows
MCS_PYRG_FN int pyr_clamp_mask(int v, int nmasks) {
  return v < 0 ? 0 : (v > nmasks - 1 ? nmasks - 1 : v);
}
MCS_PYRG_FN int pyr_groups_max(int F, int G, int nmasks) { return (F + G - 1) / G + nmasks - 1; }
MCS_PYRG_FN int pyr_groups_of(int count, int G) { return (count + G - 1) / G; }

// The whole rule, serially (the reference; see above).  mask_index == nullptr: every frame has mask 0.  group_frames:
// [pyr_groups_max][G], group_mask: [pyr_groups_max] (0 for an empty group), count: nmasks
// scratch entries.
MCS_PYRG_FN void pyr_group_frames(const int32_t* mask_index, int F, int nmasks, int G,
                                  int32_t* group_frames, int32_t* group_mask, int32_t* count) {
  const int ng = pyr_groups_max(F, G, nmasks);
  for (int i = 0; i < ng * G; i++) group_frames[i] = -1;
  for (int g = 0; g < ng; g++) group_mask[g] = 0;
  for (int m = 0; m < nmasks; m++) count[m] = 0;
  for (int f = 0; f < F; f++) count[mask_index ? pyr_clamp_mask(mask_index[f], nmasks) : 0]++;
  // count[m] -> first group of mask m
  int first = 0;
  for (int m = 0; m < nmasks; m++) {
    const int n = pyr_groups_of(count[m], G);
    for (int g = first; g < first + n; g++) group_mask[g] = m;
    count[m] = first * G;       // next free entry of mask m (its groups are consecutive)
    first += n;
  }
  for (int f = 0; f < F; f++) {
    const int m = mask_index ? pyr_clamp_mask(mask_index[f], nmasks) : 0;
    group_frames[count[m]++] = f;
  }
}

}  // namespace mcs
