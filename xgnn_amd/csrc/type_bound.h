// type_bound.h -- a wave's 64-way search over the type bytes of a type-sorted list (link_seeds_typed.hip,
// sample_walk_metapath.hip).
#pragma once
#include "ggms_device.h"

namespace ggms {

// the first p in [lo, lo + len] with !(type[p] < key) (UPPER: !(type[p] <= key)); type is non-decreasing on [lo, lo + len).
// One wave, 64 probes per round: 300 000 entries are 4 rounds.
template <bool UPPER>
__device__ __forceinline__ uint64_t wave_type_bound(const uint8_t *__restrict__ type, uint64_t lo, uint64_t len, uint32_t key,
                                                    uint32_t lane) {
  while (len > kWave) {
    const uint64_t step = (len + kWave - 1) / kWave;
    const uint64_t idx = lo + lane * step, end = lo + len;
    bool below = false;
    if (idx < end) below = UPPER ? type[idx] <= key : type[idx] < key;
    const uint32_t c = (uint32_t)__popcll(__ballot(below)); // lanes 0 .. c-1 (sorted); the bound lies behind probe c-1
    if (c == 0u) return lo;
    const uint64_t stop = lo + (uint64_t)c * step; // probe c: not below, or past the end
    lo += (uint64_t)(c - 1u) * step + 1u;
    len = (stop < end ? stop : end) - lo;
  }
  bool below = false;
  if (lane < len) below = UPPER ? type[lo + lane] <= key : type[lo + lane] < key;
  return lo + (uint64_t)__popcll(__ballot(below));
}

} // namespace ggms
