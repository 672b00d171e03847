// khop_closure.hip -- L-hop closure of a seed set (presample_static's per-batch work).
//
// Reference: DoGPUSampleAllNeighbour (cuda/cuda_loops.cc:526-598) over GPUExtractNeighbour
// (cuda/cuda_extract_neighbour.cu): per hop a count kernel, a cub scan and a compact kernel over EVERY unique node so
// far, then a hash-table dedup, with four host syncs per hop.  Here the result is a set, not an ordered unique list, so
// a node is claimed with one atomic on a direct-indexed stamp word, and only the frontier is expanded:
//   hop 0      k_closure_seeds: every seed claims its word; the winners are hop 0
//   hop h > 0  the frontier's edges in tiles (edge_tiles.h): a tile_scan over the frontier's degrees (size and edge
//              total on the device), then k_closure_expand = the shared walk with a sink that claims and appends
//   boundary   k_closure_mark: hop_offsets[h] = the append cursor, and the size of the next frontier
// Appends: a lane that wins a word keeps the node in a register; the workgroup sums its winners and takes its range of
// the closure with ONE atomic per round on the cursor (cdna_hip_programming.md Guideline 12).  No host round trip.
#include "edge_tiles.h"

namespace ggms {

// workspace: these control words, then pre (num_node words), then the scan area
struct ClosureCtl {
  unsigned long long tail;  // append cursor = nodes in the closure so far
  uint64_t edges;           // edges of the current frontier (scan total)
  uint64_t front;           // nodes of the current frontier
  uint64_t _pad[5];
};
inline size_t closure_pre_words(size_t num_node) { return (num_node + 3) & ~(size_t)3; }

struct ClosureOut {
  uint32_t *visit;
  uint32_t stamp;
  uint32_t num_node;
  uint32_t *freq; // may be NULL
  uint32_t *closure;
  unsigned long long *tail;
};

// Claim up to kPerThread nodes per lane (bit k of `valid`: v[k] is one) and append the winners.  Called by the whole
// workgroup (barriers inside).  A plain load first: a node already in the closure costs no atomic.
__device__ __forceinline__ void claim_append(const ClosureOut &o, const uint32_t (&v)[kPerThread], uint32_t valid,
                                             uint32_t *smem, unsigned long long &s_base) {
  uint32_t seen[kPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kPerThread; ++k) seen[k] = ((valid >> k) & 1u) ? o.visit[v[k]] : o.stamp;
  uint32_t won = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPerThread; ++k)
    if (seen[k] != o.stamp && atomicExch(&o.visit[v[k]], o.stamp) != o.stamp) won |= 1u << k;
  uint32_t total;
  const uint32_t excl = block_exclusive_scan((uint32_t)__builtin_popcount(won), smem, total);
  if (total == 0) return; // uniform
  if (threadIdx.x == 0) s_base = atomicAdd(o.tail, (unsigned long long)total);
  __syncthreads();
  unsigned long long pos = s_base + excl;
#pragma unroll
  for (uint32_t k = 0; k < kPerThread; ++k) {
    if (!((won >> k) & 1u)) continue;
    if (pos < o.num_node) o.closure[pos] = v[k]; // a node is won once per call: never more than num_node appends
    if (o.freq) o.freq[v[k]] += 1u;              // only the winner touches freq[v] in this call
    ++pos;
  }
  __syncthreads(); // s_base is rewritten by the next round
}

__global__ __launch_bounds__(kBlock) void k_closure_seeds(const uint32_t *__restrict__ seeds, uint64_t n, ClosureOut o) {
  __shared__ uint32_t smem[kBlock / kWave];
  __shared__ unsigned long long s_base;
  for (uint64_t base = (uint64_t)blockIdx.x * kEdgeTile; base < n; base += (uint64_t)gridDim.x * kEdgeTile) {
    uint32_t v[kPerThread], valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k) {
      const uint64_t i = base + k * kBlock + threadIdx.x;
      v[k] = i < n ? seeds[i] : 0u;
      if (i < n && v[k] < o.num_node) valid |= 1u << k; // an id out of range is not written anywhere
    }
    claim_append(o, v, valid, smem, s_base);
  }
}

// hop_offsets[h] = cursor; the frontier of the next hop is [hop_offsets[h - 1], hop_offsets[h])
__global__ void k_closure_mark(uint64_t *hop_offsets, uint32_t h, ClosureCtl *ctl, uint64_t num_node) {
  if (threadIdx.x != 0) return;
  const uint64_t end = ctl->tail < num_node ? ctl->tail : num_node;
  hop_offsets[h] = end;
  ctl->front = end - hop_offsets[h - 1];
}

// hop h: the walk over the frontier closure[hop_offsets[h - 1], +ctl->front); a neighbour in range is claimed
__global__ __launch_bounds__(kBlock) void k_closure_expand(GraphView g, ClosureOut o, const uint32_t *__restrict__ pre,
                                                           const uint64_t *hop_offsets, uint32_t h,
                                                           const ClosureCtl *ctl) {
  __shared__ uint32_t smem[kBlock / kWave];
  __shared__ unsigned long long s_base;
  const uint64_t f0 = hop_offsets[h - 1];
  const uint64_t F = ctl->front;
  const uint64_t E = ctl->edges;
  walk_edge_tiles(g, o.closure + f0, F, pre, E, [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t) {
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k)
      if (v[k] < o.num_node) valid |= have & (1u << k);
    claim_append(o, v, valid, smem, s_base);
  });
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_khop_closure_workspace_bytes(size_t num_node) {
  return sizeof(ClosureCtl) + closure_pre_words(num_node) * 4 + edge_scan_words(num_node) * 4;
}

int ggms_khop_closure(const ggms_graph_t *graph, const ggms_id_t *seeds, size_t num_seeds, uint32_t num_hop,
                      uint32_t *visit, uint32_t stamp, uint32_t *freq, ggms_id_t *closure, uint64_t *hop_offsets_dev,
                      void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph && visit && closure && hop_offsets_dev && workspace);
  GGMS_CHECK_ARG(stamp != 0);
  GGMS_CHECK_ARG(num_seeds == 0 || seeds);
  const size_t N = graph->num_node;
  GGMS_CHECK_ARG(workspace_bytes >= ggms_khop_closure_workspace_bytes(N));
  GGMS_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
  GraphView g;
  if (!view_of(graph, g)) return GGMS_ERR_INVALID;
  hipStream_t s = to_stream(stream);
  ClosureCtl *ctl = (ClosureCtl *)workspace;
  uint32_t *pre = (uint32_t *)(ctl + 1);
  uint32_t *scan_words = pre + closure_pre_words(N);
  GGMS_HIP(hipMemsetAsync(ctl, 0, sizeof(ClosureCtl), s));
  GGMS_HIP(hipMemsetAsync(hop_offsets_dev, 0, (num_hop + 2) * sizeof(uint64_t), s));
  const ClosureOut o{visit, stamp, (uint32_t)N, freq, closure, &ctl->tail};
  hipLaunchKernelGGL(k_closure_seeds, dim3(grid_for(num_seeds, kEdgeTile)), dim3(kBlock), 0, s, seeds,
                     (uint64_t)num_seeds, o);
  GGMS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_closure_mark, dim3(1), dim3(kWave), 0, s, hop_offsets_dev, 1u, ctl, (uint64_t)N);
  GGMS_LAUNCH_CHECK();
  for (uint32_t h = 1; h <= num_hop; ++h) {
    // pre[i] over the frontier closure[hop_offsets[h - 1], hop_offsets[h]); its size and edge total stay on the device
    int rc = tile_scan(ListDegree{g, closure, hop_offsets_dev + (h - 1)}, StorePrefix{pre}, N,
                       count_of(N, &ctl->front), ScanArea{scan_words, false}, nullptr, nullptr, &ctl->edges, s);
    if (rc != GGMS_OK) return rc;
    // a persistent grid: the frontier's edge count is only known on the device
    hipLaunchKernelGGL(k_closure_expand, dim3(grid_cap()), dim3(kBlock), 0, s, g, o, pre, hop_offsets_dev, h, ctl);
    GGMS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_closure_mark, dim3(1), dim3(kWave), 0, s, hop_offsets_dev, h + 1, ctl, (uint64_t)N);
    GGMS_LAUNCH_CHECK();
  }
  return GGMS_OK;
}

} // extern "C"
