// labor_hash.h -- khop_labor's hash and salt rules (include/ggms.h), one copy for the kernels and the engine.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ggms {

// MurmurHash3's 32-bit finaliser
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// the salt of layer `layer` (the index into `fanouts`) of a batch
inline uint32_t labor_layer_salt(uint32_t batch_salt, uint32_t layer) {
  return fmix32(batch_salt + 0x9e3779b9u * (layer + 1u));
}

// the engine's batch salt: a function of the run's seed, the epoch and the batch's GLOBAL index in its epoch -- not of
// the pipeline, stream, worker or process that happens to draw the batch
inline uint32_t labor_batch_salt(uint64_t seed, uint64_t epoch, uint64_t batch_index) {
  return fmix32(fmix32((uint32_t)seed + (uint32_t)epoch) ^ (uint32_t)batch_index);
}

} // namespace ggms
