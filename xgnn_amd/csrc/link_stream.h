// link_stream.h -- the list streaming of the link front's exclude modes: a wave reads a list in chunks of
// 64 ids and tests wave-uniform candidates against them.  Shared by link_seeds.hip (u's whole list) and
// link_seeds_typed.hip (the positive's relation segment of it); the candidates themselves are each file's own.
#pragma once
#include "ggms_device.h"

namespace ggms {

constexpr uint32_t kLinkAttempts = 8; // A of include/ggms.h
constexpr uint32_t kLinkMaxNeg = 64;  // one lane per negative
constexpr uint32_t kLinkChunks = 8;   // 64-id chunks of the list a lane has in flight: the tail of a list (most lists whole)
constexpr uint32_t kLinkWide = 32;    // ... and while at least 32 chunks are left: a long list is one wave's stream, and
                                      // its rate is the bytes that wave keeps in flight

// U chunks of list[0, d) from `base`; FULL: all of them lie inside the list, else a lane beyond it holds `fill`
template <uint32_t U, bool FULL>
__device__ __forceinline__ void link_load(const uint32_t *__restrict__ list, uint32_t d, uint64_t base, uint32_t lane,
                                          uint32_t fill, uint32_t (&t)[U]) {
#pragma unroll
  for (uint32_t c = 0; c < U; ++c) {
    const uint64_t p = base + c * kWave + lane;
    t[c] = (FULL || p < d) ? list[p] : fill;
  }
}
// does any lane hold x in its chunks?  (x is wave-uniform; the compares' results are the ballot)
template <uint32_t U>
__device__ __forceinline__ bool link_any(const uint32_t (&t)[U], uint32_t x) {
  bool h = false;
#pragma unroll
  for (uint32_t c = 0; c < U; ++c) h |= t[c] == x;
  return __ballot(h) != 0ull;
}

// pass 1 over one group of U chunks: the negatives (bits) whose attempt 0 occurs in it
template <uint32_t U, bool FULL>
__device__ __forceinline__ uint64_t link_test_first(const uint32_t *__restrict__ list, uint32_t d, uint64_t base,
                                                    uint32_t lane, uint32_t u, uint32_t c0, uint32_t K) {
  uint32_t t[U];
  link_load<U, FULL>(list, d, base, lane, u, t);
  uint64_t hit = 0;
  for (uint32_t j = 0; j < K; ++j)
    if (link_any<U>(t, __builtin_amdgcn_readlane(c0, j))) hit |= 1ull << j;
  return hit;
}
// pass 2 over one group: attempts 1 .. 7 of the negatives in `rej`, r[a] |= the negatives whose attempt a occurs in it
template <uint32_t U, bool FULL>
__device__ __forceinline__ void link_test_rest(const uint32_t *__restrict__ list, uint32_t d, uint64_t base, uint32_t lane,
                                               uint32_t u, const uint32_t (&c)[kLinkAttempts], uint64_t rej,
                                               uint64_t (&r)[kLinkAttempts]) {
  uint32_t t[U];
  link_load<U, FULL>(list, d, base, lane, u, t);
  for (uint64_t m = rej; m != 0ull; m &= m - 1ull) {
    const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((long long)m) - 1));
#pragma unroll
    for (uint32_t a = 1; a < kLinkAttempts; ++a)
      if (link_any<U>(t, __builtin_amdgcn_readlane(c[a], j))) r[a] |= 1ull << j;
  }
}

} // namespace ggms
