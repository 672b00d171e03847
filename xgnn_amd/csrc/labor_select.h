// labor_select.h -- the bottom-k selection of khop_labor (include/ggms.h), one copy for the samplers that use it:
// khop_labor over a seed's whole list (sample_labor.hip) and khop_temporal over the list's eligible prefix
// (sample_temporal.hip).  The callers differ in where the length comes from and in what an emitted edge writes, so both
// are the caller's: `d` is an argument and every selected position leaves through emit(o, p, t) -- o its rank among the
// seed's selected positions (ascending position), p the position in the list, t = list[p].
//   labor_wave_select<R>  one WAVE, k < d <= 64 R: the hashes of the whole list sit in registers, the k-th smallest is
//                         found by a bitwise threshold search (32 rounds of ballot + popcount), ties break by position
//   labor_hub_list        one WORKGROUP, any d > 2 k + 64: pre-filter into LDS, else the exact route over the list
#pragma once
#include "ggms_device.h"
#include "labor_hash.h"

namespace ggms {

constexpr uint32_t kLaborWave1 = 64;     // list lengths up to which a lane of the seed's wave holds 1 key,
constexpr uint32_t kLaborWave4 = 256;    // 4 keys,
constexpr uint32_t kLaborWaveMax = 1024; // 16 keys; longer lists take a workgroup (labor_hub_list)
constexpr uint32_t kLaborCand = 1024;    // keys the hub pre-filter's LDS buffer holds (8 KB)
constexpr uint32_t kLaborMaxFanout = 127;

// fanout < d <= 64 R: the whole list in the wave's registers, position p = 64 r + lane
template <int R, typename Emit>
__device__ __forceinline__ void labor_wave_select(const uint32_t *__restrict__ list, uint32_t d, uint32_t k, uint32_t salt,
                                                  const Emit &emit) {
  const uint32_t lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t t[R], h[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = 64u * r + lane;
    t[r] = p < d ? list[p] : 0u;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) h[r] = fmix32(t[r] ^ salt);
  // V = the k-th smallest hash: the largest V with fewer than k hashes below it
  uint32_t V = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t T = V | (1u << bit);
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) c += (uint32_t)__popcll(__ballot(64u * r + lane < d && h[r] < T));
    if (c < k) V = T;
  }
  uint32_t less = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) less += (uint32_t)__popcll(__ballot(64u * r + lane < d && h[r] < V));
  const uint32_t need = k - less; // of the positions whose hash IS V, the first `need`
  uint32_t ties = 0, out = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool in = 64u * r + lane < d;
    const uint64_t eq = __ballot(in && h[r] == V);
    const bool sel = in && (h[r] < V || (h[r] == V && ties + (uint32_t)__popcll(eq & below) < need));
    const uint64_t sm = __ballot(sel);
    if (sel) emit(out + (uint32_t)__popcll(sm & below), 64u * r + lane, t[r]);
    ties += (uint32_t)__popcll(eq);
    out += (uint32_t)__popcll(sm);
  }
}

// sum of x over the workgroup; buf: 2 x 4 words, `turn` alternates between calls (one barrier per call)
__device__ __forceinline__ uint32_t labor_block_sum(uint32_t x, uint32_t (*buf)[kBlock / kWave], uint32_t turn) {
  x = wave_reduce_sum(x);
  if (lane_id() == 0) buf[turn & 1u][threadIdx.x >> 6] = x;
  __syncthreads();
  return buf[turn & 1u][0] + buf[turn & 1u][1] + buf[turn & 1u][2] + buf[turn & 1u][3];
}

// hashes of list[0, d) below T, counted by the workgroup's lanes (U loads in flight each); the caller sums
template <uint32_t U = 8>
__device__ __forceinline__ uint32_t labor_count_below(const uint32_t *__restrict__ list, uint32_t d, uint32_t salt,
                                                      uint32_t T) {
  uint32_t c = 0;
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + threadIdx.x;
      v[u] = p < d ? list[p] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) c += (base + u * kBlock + threadIdx.x < d && fmix32(v[u] ^ salt) < T) ? 1u : 0u;
  }
  return c;
}

// One list by the whole workgroup (every thread calls it with the same arguments; d > kLaborWaveMax >= 2 k + 64).  A
// first pass keeps the keys whose hash is under the threshold that k / d predicts with slack ((2 k + 64) / d of the hash
// range) in an LDS buffer of kLaborCand keys; the k-th smallest KEY among the survivors is found by the bitwise search
// over LDS, and the k selected positions are ranked by position.  Fewer than k survivors, or more than the buffer
// holds: the exact route -- the bitwise search over the list itself and an ordered emit with block scans.  Ends with a
// barrier: the next call may rewrite the LDS at once.
template <typename Emit>
__device__ __forceinline__ void labor_hub_list(const uint32_t *__restrict__ list, uint32_t d, uint32_t k, uint32_t salt,
                                               const Emit &emit) {
  constexpr uint32_t U = 32; // list entries a lane has in flight in the first pass: one workgroup streams the whole list
  __shared__ unsigned long long s_key[kLaborCand];
  __shared__ uint32_t s_sel[kLaborMaxFanout + 1];
  __shared__ uint32_t s_sum[2][kBlock / kWave];
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ uint32_t s_cnt, s_nsel;
  const uint32_t tid = threadIdx.x;
  // ---- first pass: the keys under the predicted threshold (d > kLaborWaveMax >= 2 k + 64, so T0 < 2^32)
  const uint32_t T0 = (uint32_t)(((uint64_t)(2u * k + 64u) << 32) / d);
  if (tid == 0) {
    s_cnt = 0;
    s_nsel = 0;
  }
  __syncthreads();
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + tid;
      v[u] = p < d ? list[p] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + tid;
      const uint32_t h = fmix32(v[u] ^ salt);
      if (p < d && h < T0) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        if (slot < kLaborCand) s_key[slot] = ((unsigned long long)h << 32) | (uint32_t)p;
      }
    }
  }
  __syncthreads();
  const uint32_t m = s_cnt;
  uint32_t turn = 0;
  if (m >= k && m <= kLaborCand) {
    // ---- the k-th smallest key among the survivors: hashes are below T0 and positions below d, the bits above
    // either are zero in every key
    unsigned long long K = 0;
    const int hash_top = 63 - __clzll(((unsigned long long)T0 << 32) | 0xffffffffull);
    const int pos_top = 31 - __clz((int)(d - 1u));
    for (int bit = hash_top; bit >= 0; --bit) {
      if (bit < 32 && bit > pos_top) continue;
      const unsigned long long T = K | (1ull << bit);
      uint32_t c = 0;
      for (uint32_t j = tid; j < m; j += kBlock) c += s_key[j] < T ? 1u : 0u;
      if (labor_block_sum(c, s_sum, turn++) < k) K = T;
    }
    for (uint32_t j = tid; j < m; j += kBlock)
      if (s_key[j] <= K) { // exactly k of them: keys are distinct
        const uint32_t slot = atomicAdd(&s_nsel, 1u);
        if (slot <= kLaborMaxFanout) s_sel[slot] = (uint32_t)s_key[j];
      }
    __syncthreads();
    if (tid < k) {
      const uint32_t p = s_sel[tid];
      uint32_t rank = 0;
      for (uint32_t x = 0; x < k; ++x) rank += s_sel[x] < p ? 1u : 0u;
      emit(rank, p, list[p]);
    }
  } else {
    // ---- the exact route: the k-th smallest hash over the list itself, then an emit in position order
    uint32_t V = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t T = V | (1u << bit);
      if (labor_block_sum(labor_count_below(list, d, salt, T), s_sum, turn++) < k) V = T;
    }
    const uint32_t need = k - labor_block_sum(labor_count_below(list, d, salt, V), s_sum, turn++);
    uint32_t ties = 0, out = 0;
    for (uint64_t base = 0; base < d && out < k; base += kBlock) {
      const uint64_t p = base + tid;
      const uint32_t t = p < d ? list[p] : 0u;
      const uint32_t h = fmix32(t ^ salt);
      const bool lt = p < d && h < V, eq = p < d && h == V;
      if (!__syncthreads_or(lt || eq)) continue;
      uint32_t tie_total, sel_total;
      const uint32_t tie_rank = ties + block_exclusive_scan(eq ? 1u : 0u, s_scan, tie_total);
      const bool sel = lt || (eq && tie_rank < need);
      const uint32_t o = out + block_exclusive_scan(sel ? 1u : 0u, s_scan, sel_total);
      if (sel) emit(o, (uint32_t)p, t);
      ties += tie_total;
      out += sel_total;
    }
  }
  __syncthreads(); // s_key / s_sel / the counters are rewritten by the next list
}

} // namespace ggms
