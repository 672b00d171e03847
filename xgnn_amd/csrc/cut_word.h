// cut_word.h -- a word of the temporal batch's cut table (sample_temporal.hip, sample_typed_temporal.hip).
#pragma once
#include "ggms_device.h"

namespace ggms {

// a cut-table word: (stamp << 32) | (0xffffffff - cut) under unsigned 64-bit max -- a newer stamp beats a stale word,
// within a stamp the smaller cut wins; a word with another stamp reads as absent (cut = +inf = 0xffffffff)
__device__ __forceinline__ unsigned long long cut_word(uint32_t stamp, uint32_t cut) {
  return ((unsigned long long)stamp << 32) | (0xffffffffu - cut);
}
__device__ __forceinline__ uint32_t cut_of_word(unsigned long long w, uint32_t stamp) {
  return (uint32_t)(w >> 32) == stamp ? 0xffffffffu - (uint32_t)w : 0xffffffffu;
}

} // namespace ggms
