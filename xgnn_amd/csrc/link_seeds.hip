// link_seeds.hip -- the front of a link-prediction batch: edge ids -> endpoints + negative destinations.
//
// There is no reference counterpart; the definition is in include/ggms.h (ggms_link_seeds) and tests/link_ref.py
// restates it in numpy.  Stateless like khop_labor: the output is a pure function of (graph, edge ids, K, mode, salt),
// the variate of a negative is a hash of its EDGE ID, not of the edge's place in the call.
//
// One launch, one WAVE per positive edge e, grid-stride:
//   source       u = the row of CSR position e: a 64-way search over indptr (wave_find_node, 5 rounds at 10^8 nodes
//                instead of 27 dependent probes); v = indices[e]
//   candidates   lane j holds the candidates of negative j (K <= 64): attempt 0 always, attempts 1 .. 7 only once
//                something was rejected
//   mode EXCLUDE pass 1 streams u's list in chunks of 64 ids, 8 chunks in flight per lane (32 while the list has that
//                many left: a long list is one wave's stream, bound by the bytes it keeps in flight), and tests attempt 0 of
//                every negative: the candidate of negative j is broadcast (v_readlane) and compared with the lane's ids
//                -- the compare's result IS the ballot.  A rejection has probability about d / N, so in nearly every
//                wave that is all.  Only if something was rejected, pass 2 streams the list once more and tests the
//                attempts 1 .. 7 of the rejected negatives together: a hub's list is read twice at most, never once
//                per attempt.  The list is not sorted (khop2 permutes it): no search inside it.
// Lanes beyond the list read nothing and hold u itself, which every candidate is tested against anyway.
// No LDS, no scratch, no workspace; the forced count is one 64-bit atomic per wave that forced something.
#include "edge_tiles.h"
#include "ggms_internal.h"
#include "labor_hash.h"

namespace ggms {

constexpr uint32_t kLinkAttempts = 8; // A of include/ggms.h
constexpr uint32_t kLinkMaxNeg = 64;  // one lane per negative
constexpr uint32_t kLinkChunks = 8;   // 64-id chunks of the list a lane has in flight: the tail of a list (most lists whole)
constexpr uint32_t kLinkWide = 32;    // ... and while at least 32 chunks are left: a long list is one wave's stream, and
                                      // its rate is the bytes that wave keeps in flight

// cand(e, j, a) with h0 = fmix32(e ^ salt)
__device__ __forceinline__ uint32_t link_cand(uint32_t h0, uint32_t j, uint32_t a, uint32_t num_node) {
  return __umulhi(fmix32(h0 + 0x9e3779b9u * (j * kLinkAttempts + a + 1u)), num_node);
}

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

__global__ __launch_bounds__(kBlock) void k_link_seeds(const uint32_t *__restrict__ indptr,
                                                       const uint32_t *__restrict__ indices, uint32_t num_node,
                                                       const uint32_t *__restrict__ edge_ids, uint64_t B, uint32_t K,
                                                       int exclude, uint32_t salt, uint32_t *__restrict__ out,
                                                       unsigned long long *num_forced) {
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t E = indptr[num_node];
  uint32_t forced_total = 0; // wave-uniform
  for (uint64_t i = wave; i < B; i += waves) {
    const uint32_t e = edge_ids[i];
    uint32_t *const neg = out + 2 * B + i * K;
    if (e >= E) { // a caller error: nothing is read, the positive's positions say so
      if (lane == 0) {
        out[i] = GGMS_EMPTY_KEY;
        out[B + i] = GGMS_EMPTY_KEY;
      }
      if (lane < K) neg[lane] = GGMS_EMPTY_KEY;
      continue;
    }
    // the last row u with indptr[u] <= e: rows of degree 0 in front of it share its offset and are passed over
    const uint32_t u = (uint32_t)wave_find_node(indptr, num_node, e);
    if (lane == 0) {
      out[i] = u;
      out[B + i] = indices[e];
    }
    const uint32_t h0 = fmix32(e ^ salt);
    const uint32_t c0 = link_cand(h0, lane, 0, num_node);
    uint32_t pick = c0;
    if (exclude) {
      const uint32_t b = indptr[u], d = indptr[u + 1] - b;
      const uint32_t *__restrict__ list = indices + b;
      const bool mine = lane < K;
      // ---- pass 1: attempt 0 of every negative
      uint64_t rej = __ballot(mine && c0 == u);
      uint64_t base = 0;
      for (; base + kLinkWide * kWave <= d; base += kLinkWide * kWave)
        rej |= link_test_first<kLinkWide, true>(list, d, base, lane, u, c0, K);
      for (; base < d; base += kLinkChunks * kWave) rej |= link_test_first<kLinkChunks, false>(list, d, base, lane, u, c0, K);
      if (rej != 0ull) {
        // ---- pass 2: attempts 1 .. 7 of the rejected negatives, all in one more pass over the list
        uint32_t c[kLinkAttempts];
        uint64_t r[kLinkAttempts];
        c[0] = c0;
        r[0] = rej;
#pragma unroll
        for (uint32_t a = 1; a < kLinkAttempts; ++a) {
          c[a] = link_cand(h0, lane, a, num_node);
          r[a] = __ballot(c[a] == u) & rej;
        }
        for (base = 0; base + kLinkWide * kWave <= d; base += kLinkWide * kWave)
          link_test_rest<kLinkWide, true>(list, d, base, lane, u, c, rej, r);
        for (; base < d; base += kLinkChunks * kWave) link_test_rest<kLinkChunks, false>(list, d, base, lane, u, c, rej, r);
        // the first accepted attempt; none: the last candidate, counted
        bool open = true;
#pragma unroll
        for (uint32_t a = 0; a < kLinkAttempts; ++a) {
          const bool ok = !((r[a] >> lane) & 1ull);
          pick = (open && ok) ? c[a] : pick;
          open = open && !ok;
        }
        pick = open ? c[kLinkAttempts - 1] : pick;
        forced_total += (uint32_t)__popcll(__ballot(mine && open));
      }
    }
    if (lane < K) neg[lane] = pick;
  }
  if (num_forced && forced_total != 0u && lane == 0) atomicAdd(num_forced, (unsigned long long)forced_total);
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_link_seeds(const ggms_graph_t *graph, const ggms_id_t *edge_ids, size_t num_pos, uint32_t num_negative,
                    int mode, uint32_t salt, ggms_id_t *endpoints, uint64_t *num_forced_dev, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph);
  if (graph->num_part != 0) {
    set_error("ggms_link_seeds: num_part %u: edge ids are positions of ONE CSR, the call takes unsharded graphs only",
              graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (num_negative < 1 || num_negative > kLinkMaxNeg) {
    set_error("ggms_link_seeds: num_negative %u (1 .. %u: one lane of the positive's wave per negative)", num_negative,
              kLinkMaxNeg);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(mode == GGMS_NEG_UNIFORM || mode == GGMS_NEG_EXCLUDE);
  if (num_pos == 0) return GGMS_OK;
  GGMS_CHECK_ARG(graph->indptr && graph->indices && edge_ids && endpoints);
  GGMS_CHECK_ARG(graph->num_node >= 1);
  hipLaunchKernelGGL(k_link_seeds, dim3(grid_for(num_pos, kBlock / kWave)), dim3(kBlock), 0, to_stream(stream),
                     graph->indptr, graph->indices, graph->num_node, edge_ids, (uint64_t)num_pos, num_negative,
                     mode == GGMS_NEG_EXCLUDE ? 1 : 0, salt, endpoints, (unsigned long long *)num_forced_dev);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
