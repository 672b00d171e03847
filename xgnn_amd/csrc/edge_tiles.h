// edge_tiles.h -- every neighbour of a list of nodes, walked in edge tiles: a hub is spread over many workgroups.
//
// Reference: GPUExtractNeighbour (cuda/cuda_extract_neighbour.cu), the one extraction behind DoGPUSampleAllNeighbour
// and DoGPUSampleDyCache -- a count kernel, a cub scan and a compact kernel with one thread per NODE, so a hub's list
// is one lane's loop.  Here the work is cut by EDGE.  Users: khop_closure.hip (a hop's frontier), prefetch.hip (arch4's
// expansion list).  Both run the same two steps:
//   tile_scan(ListDegree, StorePrefix)   pre[i] = first edge of list node i; the edge total E stays on the device
//   walk_edge_tiles on a persistent grid tiles of kEdgeTile edges: a workgroup finds the node of its tile's first edge,
//                                        stages the list heads of the nodes the tile touches in LDS, each lane takes
//                                        kPerThread edges, and the kernel's sink gets the neighbour ids
#pragma once
#include "tile_scan.h"

namespace ggms {

constexpr uint32_t kPerThread = 8;
constexpr uint32_t kEdgeTile = kBlock * kPerThread; // edges per workgroup round
constexpr uint32_t kWin = kEdgeTile;                // list nodes staged per round at most

// scan value / emit over a node list: degree of nodes[*first + i] (first may be NULL: 0); pre[i] = edges of the list
// nodes before i
struct ListDegree {
  GraphView g;
  const uint32_t *nodes;
  const uint64_t *first;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    uint32_t len;
    g.neighbours(nodes[(first ? *first : 0) + i], len);
    return len;
  }
};
struct StorePrefix {
  uint32_t *pre;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { pre[i] = excl; }
};
// words of the scan area of that tile_scan over a list of at most n nodes
inline size_t edge_scan_words(size_t n) { return tile_scan_words(n) + 2; }

// the last index i < F with pre[i] <= e, pre non-decreasing with pre[0] = 0 <= e (the owner of edge e): one wave, 64
// probes per step
__device__ __forceinline__ uint64_t wave_find_node(const uint32_t *pre, uint64_t F, uint64_t e) {
  const uint32_t lane = lane_id();
  uint64_t lo = 0, len = F;
  while (len > kWave) {
    const uint64_t step = (len + kWave - 1) / kWave;
    const uint64_t idx = lo + lane * step;
    const bool ok = idx < lo + len && pre[idx] <= e;
    const uint32_t c = (uint32_t)__popcll(__ballot(ok)); // lanes 0 .. c-1 (pre is non-decreasing; lane 0 always)
    const uint64_t end = lo + len;
    lo += (uint64_t)(c - 1) * step;
    len = end - lo < step ? end - lo : step;
  }
  const bool ok = lane < len && pre[lo + lane] <= e;
  return lo + (uint64_t)__popcll(__ballot(ok)) - 1;
}

// The walk: edge e of the concatenated lists of nodes[0, F) is entry e - pre[i] of the list of its owner i.  Called by
// every thread of a kBlock-wide workgroup of a persistent grid.  Once per round the WHOLE workgroup calls
// sink(v, have, cur): v[k] is the neighbour id of edge cur + k * kBlock + threadIdx.x where bit k of `have` is set (0
// elsewhere).  The sink may use barriers and LDS of its own; the LDS staged here is not rewritten before every lane
// has returned from it (each round ends with the walk's own barrier).
// Precondition: E < 2^32 -- pre and the staged copies are 32-bit, edge positions 64-bit.
//
// Two sink flavours, one body (walk_edge_tiles_any; kWhere is a compile-time switch, so the plain flavour compiles to
// what it did before the second one existed):
//   walk_edge_tiles        sink(v, have, cur) as above; every list node is a valid id.
//   walk_edge_tiles_where  sink(v, have, cur, own, ent): own[k] = the index i of the edge's owner in `nodes`, ent[k] = the
//                          address the neighbour id was loaded from -- its list offset is ent[k] minus the list's start,
//                          its CSR position ent[k] - g.indices on an unsharded graph, with no further load.  The list may
//                          hold ids that own no edges (pre[i + 1] == pre[i]): an id >= num_node among them (a padding
//                          word, GGMS_EMPTY_KEY) is never looked up in indptr.
template <bool kWhere, typename Sink>
__device__ __forceinline__ void walk_edge_tiles_any(const GraphView &g, const uint32_t *nodes, uint64_t F,
                                                    const uint32_t *__restrict__ pre, uint64_t E, uint32_t num_node,
                                                    Sink sink) {
  __shared__ uint32_t s_pre[kWin + 1];
  __shared__ const uint32_t *s_ptr[kWin];
  __shared__ uint64_t s_lo;
  for (uint64_t t = blockIdx.x; t * kEdgeTile < E; t += gridDim.x) {
    const uint64_t e0 = t * kEdgeTile;
    const uint64_t e1 = E - e0 < kEdgeTile ? E : e0 + kEdgeTile;
    if (threadIdx.x < kWave) {
      const uint64_t n = wave_find_node(pre, F, e0);
      if (threadIdx.x == 0) s_lo = n;
    }
    __syncthreads();
    uint64_t nw = s_lo, cur = e0;
    while (cur < e1) { // uniform; more than one round only where a long run of short or empty lists meets the tile
      // stage the list heads of nodes nw, nw + 1, ... up to the first one that starts at or past e1
      uint32_t wlen = 0;
      for (;;) {
        const uint32_t j = wlen + threadIdx.x;
        const uint64_t i = nw + j;
        const uint64_t p = i < F ? pre[i] : E;
        s_pre[j] = (uint32_t)p;
        if (p < e1) {
          uint32_t len;
          if constexpr (kWhere) {
            const uint32_t u = nodes[i];
            s_ptr[j] = u < num_node ? g.neighbours(u, len) : nullptr; // (an id out of range owns no edge: never read)
          } else {
            s_ptr[j] = g.neighbours(nodes[i], len);
          }
        }
        wlen += kBlock;
        if (__syncthreads_or(p >= e1) || wlen == kWin) break;
      }
      if (threadIdx.x == 0) s_pre[wlen] = (uint32_t)(nw + wlen < F ? pre[nw + wlen] : E);
      __syncthreads();
      const uint64_t s_end = s_pre[wlen];
      const uint64_t stop = s_end < e1 ? s_end : e1;
      uint32_t v[kPerThread], have = 0;
      [[maybe_unused]] uint32_t own[kPerThread];
      [[maybe_unused]] const uint32_t *ent[kPerThread];
#pragma unroll
      for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint64_t e = cur + k * kBlock + threadIdx.x;
        v[k] = 0;
        if constexpr (kWhere) {
          own[k] = 0;
          ent[k] = nullptr;
        }
        if (e < stop) {
          uint32_t lo = 0, len = wlen; // the last staged node that starts at or before e (s_pre[0] <= cur <= e)
          while (len > 1) {
            const uint32_t half = len >> 1;
            if (s_pre[lo + half] <= (uint32_t)e) lo += half;
            len -= half;
          }
          v[k] = s_ptr[lo][(uint32_t)e - s_pre[lo]];
          if constexpr (kWhere) {
            own[k] = (uint32_t)nw + lo;
            ent[k] = s_ptr[lo] + ((uint32_t)e - s_pre[lo]);
          }
          have |= 1u << k;
        }
      }
      if constexpr (kWhere) sink(v, have, cur, own, ent);
      else sink(v, have, cur);
      __syncthreads(); // every read of s_pre / s_ptr / s_lo is done before the next round restages them
      cur = stop;
      nw += wlen;
    }
  }
}

template <typename Sink>
__device__ __forceinline__ void walk_edge_tiles(const GraphView &g, const uint32_t *nodes, uint64_t F,
                                                const uint32_t *__restrict__ pre, uint64_t E, Sink sink) {
  walk_edge_tiles_any<false>(g, nodes, F, pre, E, 0u, sink);
}
// F < 2^32 (own is 32-bit)
template <typename Sink>
__device__ __forceinline__ void walk_edge_tiles_where(const GraphView &g, const uint32_t *nodes, uint64_t F,
                                                      const uint32_t *__restrict__ pre, uint64_t E, uint32_t num_node,
                                                      Sink sink) {
  walk_edge_tiles_any<true>(g, nodes, F, pre, E, num_node, sink);
}

} // namespace ggms
