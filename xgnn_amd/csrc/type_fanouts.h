// type_fanouts.h -- the fanouts per edge type of one layer, by value in the kernel arguments (sample_typed.hip,
// sample_typed_temporal.hip).
#pragma once
#include "ggms_device.h"

namespace ggms {

// k_r, r < GGMS_MAX_EDGE_TYPES, one byte each
struct TypeFanouts {
  uint32_t w[GGMS_MAX_EDGE_TYPES / 4];
  __device__ __forceinline__ uint32_t get(uint32_t r) const {
    uint32_t v = w[0];
#pragma unroll
    for (uint32_t j = 1; j < GGMS_MAX_EDGE_TYPES / 4; ++j) v = (r >> 2) == j ? w[j] : v;
    return (v >> ((r & 3u) * 8u)) & 0xffu;
  }
};

// a host row of R fanouts (every one < 256: typed_fanout_sum has refused the rest)
inline TypeFanouts type_fanouts_of(const uint32_t *type_fanout, uint32_t R) {
  TypeFanouts f{};
  for (uint32_t r = 0; r < R; ++r) f.w[r >> 2] |= (type_fanout[r] & 0xffu) << ((r & 3u) * 8u);
  return f;
}

} // namespace ggms
