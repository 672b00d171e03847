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
//   k_prefetch_list                              keys[e] = e-th entry of the concatenation of the lists of n2o[0, k), in
//                                                tiles of kEdgeTile edges on a persistent grid: a workgroup finds the node
//                                                of its first edge, stages the list heads of the nodes its tile touches in
//                                                LDS, and each lane takes kPerThread edges -- a hub's list is spread over
//                                                as many workgroups as it has tiles (as k_closure_expand)
// The keys then go through the batch's own table fill (ht_fill_impl, batch mode): one returning atomicMin per edge, and
// the ordered owner scan appends the new nodes to n2o in first-occurrence order.  The reference's insert is a CAS race
// (generate_count_hashmap_duplicates_mutable + compact_hashmap_revised_mutable); "lowest position wins" is this
// project's canonical reading of it, as for the other racy kernels: a node's local id follows its first occurrence.
#include "ggms_internal.h"

namespace ggms {

namespace {

constexpr uint32_t kPerThread = 8;
constexpr uint32_t kEdgeTile = kBlock * kPerThread; // edges per workgroup round
constexpr uint32_t kWin = kEdgeTile;                // nodes staged per round at most

struct NodeDegree {
  GraphView g;
  const uint32_t *nodes;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    uint32_t len;
    g.neighbours(nodes[i], len);
    return len;
  }
};
struct FirstEdge {
  uint32_t *pre;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { pre[i] = excl; }
};

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
  __shared__ uint32_t s_pre[kWin + 1];
  __shared__ const uint32_t *s_ptr[kWin];
  __shared__ uint64_t s_lo;
  const uint64_t F = *num_nodes;
  const uint64_t E = *total;
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
      uint32_t wlen = 0;
      for (;;) {
        const uint32_t j = wlen + threadIdx.x;
        const uint64_t i = nw + j;
        const uint64_t p = i < F ? pre[i] : E;
        s_pre[j] = (uint32_t)p;
        if (p < e1) {
          uint32_t len;
          s_ptr[j] = g.neighbours(nodes[i], len);
        }
        wlen += kBlock;
        if (__syncthreads_or(p >= e1) || wlen == kWin) break;
      }
      if (threadIdx.x == 0) s_pre[wlen] = (uint32_t)(nw + wlen < F ? pre[nw + wlen] : E);
      __syncthreads();
      const uint64_t s_end = s_pre[wlen];
      const uint64_t stop = s_end < e1 ? s_end : e1;
#pragma unroll
      for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint64_t e = cur + k * kBlock + threadIdx.x;
        if (e < stop) {
          uint32_t lo = 0, len = wlen; // the last staged node that starts at or before e (s_pre[0] <= cur <= e)
          while (len > 1) {
            const uint32_t half = len >> 1;
            if (s_pre[lo + half] <= (uint32_t)e) lo += half;
            len -= half;
          }
          keys[e] = s_ptr[lo][(uint32_t)e - s_pre[lo]];
        }
      }
      __syncthreads(); // every read of s_pre / s_ptr / s_lo is done before the next round restages them
      cur = stop;
      nw += wlen;
    }
  }
}

} // namespace

size_t prefetch_scan_words(size_t max_nodes) { return tile_scan_words(max_nodes) + 2; }

int prefetch_list_impl(const GraphView &g, const uint32_t *nodes, size_t max_nodes, uint64_t *num_nodes_dev,
                       uint32_t *pre, uint32_t *scan_words, uint32_t *status, uint64_t *total_dev, size_t max_edges,
                       uint64_t *need_dev, uint32_t *keys, hipStream_t s) {
  ScanArea area{scan_words, false};
  area.status = status;
  int rc = tile_scan(NodeDegree{g, nodes}, FirstEdge{pre}, max_nodes, count_of(max_nodes, num_nodes_dev), area, nullptr,
                     nullptr, total_dev, s);
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
