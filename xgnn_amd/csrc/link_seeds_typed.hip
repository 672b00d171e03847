// link_seeds_typed.hip -- the front of a HETEROGENEOUS link-prediction batch: edge ids -> endpoints, the positives'
// relations, and negative destinations of the positive destination's node type.
//
// There is no reference counterpart; the definition is in include/ggms.h (ggms_link_seeds_typed) and
// tests/link_typed_ref.py restates it in numpy.  link_seeds.hip's design with two changes:
//   candidates   the hash of 8d scaled to n_t, the number of nodes of type t = node_type[v], and sent through the type's
//                node list: one dependent load per candidate.  Lane j issues attempt 0's load of negative j BEFORE the
//                segment is looked for, so its round trip lies under the search and the first chunk loads; the seven loads
//                of attempts 1 .. 7 are issued together, by the lanes of rejected negatives only, in a wave that rejected
//                something.
//   mode EXCLUDE only the positions of u's list whose type is r = edge_type[e] reject (the list is sorted by type, so they
//                are one segment, and it holds e).  Its two ends are found by 64-way searches over the type bytes -- a
//                list of at most 64 entries: one load, one ballot -- never by a per-lane binary search (wave_find_node's
//                argument: 64 independent probes per round trip).  Passes 1 and 2 are link_seeds.hip's (link_stream.h),
//                over the segment: a hub with 300 000 neighbours and 40 under r streams 40 ids.
// One launch, one WAVE per positive, grid-stride; no LDS, no scratch, no workspace; the forced count is one 64-bit atomic
// per wave that forced something.
#include "edge_tiles.h"
#include "ggms_internal.h"
#include "labor_hash.h"
#include "link_stream.h"
#include "type_bound.h" // wave_type_bound

namespace ggms {

// h -> the node of type t the hash picks: mulhi32(h, n_t) through the type's list
__device__ __forceinline__ uint32_t typed_cand_at(uint32_t h0, uint32_t j, uint32_t a, uint32_t n_t) {
  return __umulhi(fmix32(h0 + 0x9e3779b9u * (j * kLinkAttempts + a + 1u)), n_t);
}

__global__ __launch_bounds__(kBlock) void k_link_seeds_typed(
    const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint32_t num_node,
    const uint8_t *__restrict__ edge_type, const uint8_t *__restrict__ node_type, const uint32_t *__restrict__ type_nodes,
    const uint32_t *__restrict__ type_base, uint32_t T, const uint32_t *__restrict__ edge_ids, uint64_t B, uint32_t K,
    int exclude, uint32_t salt, uint32_t *__restrict__ out, uint8_t *__restrict__ out_rel, unsigned long long *num_forced) {
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t E = indptr[num_node];
  uint32_t forced_total = 0; // wave-uniform
  for (uint64_t i = wave; i < B; i += waves) {
    const uint32_t e = edge_ids[i];
    uint32_t *const neg = out + 2 * B + i * K;
    // a destination that is no node, a type that is none or a type list without nodes is a broken data set: treated like
    // e >= E, nothing is read through it
    const uint32_t v = e < E ? indices[e] : GGMS_EMPTY_KEY;
    const uint32_t t = v < num_node ? node_type[v] : T;
    const uint32_t tb = t < T ? type_base[t] : 0u, n_t = t < T ? type_base[t + 1] - tb : 0u;
    if (n_t == 0u || tb >= num_node || n_t > num_node - tb) {
      if (lane == 0) {
        out[i] = GGMS_EMPTY_KEY;
        out[B + i] = GGMS_EMPTY_KEY;
        if (out_rel) out_rel[i] = 0xffu;
      }
      if (lane < K) neg[lane] = GGMS_EMPTY_KEY;
      continue;
    }
    const uint32_t r = edge_type[e];
    const uint32_t *__restrict__ pool = type_nodes + tb;
    const uint32_t h0 = fmix32(e ^ salt);
    const bool mine = lane < K;
    // attempt 0 of negative `lane`: in flight from here on
    const uint32_t c0 = mine ? pool[typed_cand_at(h0, lane, 0, n_t)] : GGMS_EMPTY_KEY;
    // the last row u with indptr[u] <= e: rows of degree 0 in front of it share its offset and are passed over
    const uint32_t u = (uint32_t)wave_find_node(indptr, num_node, e);
    if (lane == 0) {
      out[i] = u;
      out[B + i] = v;
      if (out_rel) out_rel[i] = (uint8_t)r;
    }
    uint32_t pick = c0;
    if (exclude) {
      const uint32_t b = indptr[u], d_all = indptr[u + 1] - b;
      // ---- the segment [sb, se) of relation r in u's list: sb in [b, e], se in (e, b + d_all]
      uint64_t sb, se;
      if (d_all <= (uint32_t)kWave) {
        const bool in_r = lane < d_all && edge_type[(uint64_t)b + lane] == r;
        const uint64_t m = __ballot(in_r); // holds e's bit: never 0
        sb = (uint64_t)b + (uint32_t)(__ffsll((long long)m) - 1);
        se = (uint64_t)b + (64u - (uint32_t)__clzll((long long)m));
      } else {
        sb = wave_type_bound<false>(edge_type, b, (uint64_t)e - b, r, lane);
        se = wave_type_bound<true>(edge_type, (uint64_t)e + 1u, (uint64_t)b + d_all - e - 1u, r, lane);
      }
      const uint32_t d = (uint32_t)(se - sb);
      const uint32_t *__restrict__ list = indices + sb;
      // ---- pass 1: attempt 0 of every negative
      uint64_t rej = __ballot(mine && c0 == u);
      uint64_t base = 0;
      for (; base + kLinkWide * kWave <= d; base += kLinkWide * kWave)
        rej |= link_test_first<kLinkWide, true>(list, d, base, lane, u, c0, K);
      for (; base < d; base += kLinkChunks * kWave) rej |= link_test_first<kLinkChunks, false>(list, d, base, lane, u, c0, K);
      if (rej != 0ull) {
        // ---- pass 2: attempts 1 .. 7 of the rejected negatives, all in one more pass over the segment.  Their seven
        // gathers go out together, from the rejected lanes only; the others' words are never read (link_test_rest walks
        // the bits of rej)
        const bool again = (rej >> lane) & 1ull;
        uint32_t c[kLinkAttempts];
        uint64_t rr[kLinkAttempts];
        c[0] = c0;
        rr[0] = rej;
#pragma unroll
        for (uint32_t a = 1; a < kLinkAttempts; ++a) c[a] = again ? pool[typed_cand_at(h0, lane, a, n_t)] : GGMS_EMPTY_KEY;
#pragma unroll
        for (uint32_t a = 1; a < kLinkAttempts; ++a) rr[a] = __ballot(c[a] == u) & rej;
        for (base = 0; base + kLinkWide * kWave <= d; base += kLinkWide * kWave)
          link_test_rest<kLinkWide, true>(list, d, base, lane, u, c, rej, rr);
        for (; base < d; base += kLinkChunks * kWave) link_test_rest<kLinkChunks, false>(list, d, base, lane, u, c, rej, rr);
        // the first accepted attempt; none: the last candidate, counted
        bool open = true;
#pragma unroll
        for (uint32_t a = 0; a < kLinkAttempts; ++a) {
          const bool ok = !((rr[a] >> lane) & 1ull);
          pick = (open && ok) ? c[a] : pick;
          open = open && !ok;
        }
        pick = open ? c[kLinkAttempts - 1] : pick;
        forced_total += (uint32_t)__popcll(__ballot(mine && open));
      }
    }
    if (mine) neg[lane] = pick;
  }
  if (num_forced && forced_total != 0u && lane == 0) atomicAdd(num_forced, (unsigned long long)forced_total);
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_link_seeds_typed(const ggms_graph_t *graph, const uint8_t *edge_type, const uint8_t *node_type,
                          const ggms_id_t *type_nodes, const uint32_t *type_base, uint32_t num_node_type,
                          const ggms_id_t *edge_ids, size_t num_pos, uint32_t num_negative, int mode, uint32_t salt,
                          ggms_id_t *endpoints, uint8_t *out_rel, uint64_t *num_forced_dev, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph);
  if (graph->num_part != 0) {
    set_error("ggms_link_seeds_typed: num_part %u: edge ids are positions of ONE CSR, the call takes unsharded graphs only",
              graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (num_node_type < 1 || num_node_type > GGMS_MAX_NODE_TYPES) {
    set_error("ggms_link_seeds_typed: num_node_type %u (1 .. %u)", num_node_type, (unsigned)GGMS_MAX_NODE_TYPES);
    return GGMS_ERR_INVALID;
  }
  if (num_negative < 1 || num_negative > kLinkMaxNeg) {
    set_error("ggms_link_seeds_typed: num_negative %u (1 .. %u: one lane of the positive's wave per negative)",
              num_negative, kLinkMaxNeg);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(mode == GGMS_NEG_TYPED_UNIFORM || mode == GGMS_NEG_TYPED_EXCLUDE);
  if (num_pos == 0) return GGMS_OK;
  GGMS_CHECK_ARG(graph->indptr && graph->indices && edge_ids && endpoints);
  GGMS_CHECK_ARG(edge_type && node_type && type_nodes && type_base);
  GGMS_CHECK_ARG(graph->num_node >= 1);
  hipLaunchKernelGGL(k_link_seeds_typed, dim3(grid_for(num_pos, kBlock / kWave)), dim3(kBlock), 0, to_stream(stream),
                     graph->indptr, graph->indices, graph->num_node, edge_type, node_type, type_nodes, type_base,
                     num_node_type, edge_ids, (uint64_t)num_pos, num_negative, mode == GGMS_NEG_TYPED_EXCLUDE ? 1 : 0, salt,
                     endpoints, out_rel, (unsigned long long *)num_forced_dev);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
