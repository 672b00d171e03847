// prefetch.hip -- arch4's early feature prefetch: the neighbour list of every node entered so far.
//
// Reference: DoGPUSampleDyCache (cuda/cuda_loops.cc:294-524) calls GPUExtractNeighbour (cuda/cuda_extract_neighbour.cu)
// on the unique list after the second-to-last layer -- a count kernel, a cub scan and a compact kernel with a host sync
// in between -- and enters the result with FillWithDupMutable (cuda/cuda_hashtable.cu:914-960).  The superset is known
// before the last layer is sampled, so the feature gather can start while the sampler is still busy.
//
// Here, with no host round trip (ggms_sample_batch_prefetch, sample_batch.hip, drives it):
//   tile_scan over the degrees of n2o[0, k)      pre[i] = first edge of node i; the total stays on the device
//   k_prefetch_cap                               total > capacity: the batch's status word gets GGMS_STATUS_PREFETCH_FULL
//                                                and the expansion (and the last layer) shrink to nothing -- never a write
//                                                past the caller's buffers
//   k_prefetch_list                              keys[e] = e-th entry of the concatenation of the lists of n2o[0, k):
//                                                the shared edge-tiled walk (edge_tiles.h) with a sink that stores
// The keys then go through the batch's own table fill (ht_fill_impl, batch mode): one returning atomicMin per edge, and
// the ordered owner scan appends the new nodes to n2o in first-occurrence order.  The reference's insert is a CAS race
// (generate_count_hashmap_duplicates_mutable + compact_hashmap_revised_mutable); "lowest position wins" is this
// project's canonical reading of it, as for the other racy kernels: a node's local id follows its first occurrence.
#include "edge_tiles.h"
#include "ggms_internal.h"

namespace ggms {

namespace {

// over capacity: report it, record what was needed, and let nothing downstream read past the buffers
__global__ void k_prefetch_cap(uint64_t *total, uint64_t cap, uint64_t *last_layer_n, uint32_t *status, uint64_t *need) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint64_t t = *total;
  *need = t;
  if (t > cap) {
    atomicOr(status, (uint32_t)GGMS_STATUS_PREFETCH_FULL);
    *total = 0;
    *last_layer_n = 0;
  }
}

__global__ __launch_bounds__(kBlock) void k_prefetch_list(GraphView g, const uint32_t *__restrict__ nodes,
                                                          const uint64_t *num_nodes, const uint32_t *__restrict__ pre,
                                                          const uint64_t *total, uint32_t *__restrict__ keys) {
  walk_edge_tiles(g, nodes, *num_nodes, pre, *total,
                  [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t cur) {
#pragma unroll
                    for (uint32_t k = 0; k < kPerThread; ++k)
                      if ((have >> k) & 1u) keys[cur + k * kBlock + threadIdx.x] = v[k];
                  });
}

} // namespace

size_t prefetch_scan_words(size_t max_nodes) { return edge_scan_words(max_nodes); }

int prefetch_list_impl(const GraphView &g, const uint32_t *nodes, size_t max_nodes, uint64_t *num_nodes_dev,
                       uint32_t *pre, uint32_t *scan_words, uint32_t *status, uint64_t *total_dev, size_t max_edges,
                       uint64_t *need_dev, uint32_t *keys, hipStream_t s) {
  ScanArea area{scan_words, false};
  area.status = status;
  int rc = tile_scan(ListDegree{g, nodes, nullptr}, StorePrefix{pre}, max_nodes, count_of(max_nodes, num_nodes_dev),
                     area, nullptr, nullptr, total_dev, s);
  if (rc != GGMS_OK) return rc;
  hipLaunchKernelGGL(k_prefetch_cap, dim3(1), dim3(64), 0, s, total_dev, (uint64_t)max_edges, num_nodes_dev, status,
                     need_dev);
  GGMS_LAUNCH_CHECK();
  if (max_edges == 0 || max_nodes == 0) return GGMS_OK;
  // a persistent grid: the edge count is only known on the device
  hipLaunchKernelGGL(k_prefetch_list, dim3(grid_for(max_edges, kEdgeTile)), dim3(kBlock), 0, s, g, nodes,
                     (const uint64_t *)num_nodes_dev, (const uint32_t *)pre, (const uint64_t *)total_dev, keys);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // namespace ggms
