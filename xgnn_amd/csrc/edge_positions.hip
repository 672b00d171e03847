// edge_positions.hip -- which edge of the graph is each edge of a sampled batch: CSR positions for every layer.
//
// There is no reference counterpart; the definition is in include/ggms.h (ggms_edge_positions) and
// tests/edge_positions_ref.py restates it in numpy.  A finished batch names its edges as (row, col) pairs of local ids;
// with the batch's id map (n2o) they are pairs (s, t) of global ids, and the edge is the FIRST position p of s's list with
// indices[p] == t.  The call is a post-pass: it runs behind any sampler (and behind ggms_drop_pair_edges), reads the
// frontier's lists once more -- the read khop_labor does -- and touches no sampler kernel.
//
// One 16-byte memset and two launches per call, whatever num_layer and the layers' sizes are (all layers share each):
//   memset           the long-list queue's counter
//   k_edgepos_main   a workgroup takes 256 consecutive edges of a layer, each of its waves 64 of them (a "chunk").  A lane
//                    maps its edge's col / row through the id map and loads its seed's list bounds (one 8-byte load; the
//                    whole chunk's bounds are one round trip).  The samplers emit edges in seed order, so equal seeds
//                    are neighbours: the wave finds the RUNS of equal s among its lanes (a ballot of "differs from the
//                    lane before") and walks them one after the other.  A run's list streams by once in coalesced
//                    64-entry pieces; every piece is matched against the run's targets that are still open: target j is
//                    broadcast with readlane, one compare + ballot finds its first copy in the piece, the open set is a
//                    64-bit scalar mask.  No LDS, no barrier: the four waves of a workgroup never talk.  Pieces go by in
//                    ascending position and a target leaves the open set at its first hit, so the hit is the smallest p;
//                    the walk stops when the open set is empty (a fanout-k run of a degree-d list reads the list up to
//                    its last picked neighbour).  A run cut by a chunk boundary reads its list in both chunks.
//                    A list longer than kEdgePosLong entries is not one wave's loop: its run's edges get GGMS_EMPTY_KEY
//                    here and the chunk's number goes to the queue (one atomic per chunk that holds such a run).
//   k_edgepos_long   a queued chunk is taken by kEdgePosParts workgroups = 16 waves.  Every wave rebuilds the chunk's runs
//                    (the same 64 loads) and walks the long ones, piece c of a list going to wave c % 16, four pieces in
//                    flight; what a wave finds is combined with atomicMin on eid (the smallest position wins, whichever
//                    wave saw it: k_labor_hub's and edge_tiles.h's way of spreading one list).  The queue's order is not
//                    observable.
// Nothing survives the call: the workspace holds the counter and the queue only.
//
// Why readlane + ballot and not an LDS set of the run's targets: a run has at most 64 targets and typically `fanout`
// (5 .. 25) of them, a piece is matched in (open targets) x {v_readlane, v_cmp, s_ff1} with the piece in ONE register per
// lane, and the scalar mask gives the early exit for free.  An LDS set would add a write, a barrier-free but
// latency-bound probe per list entry and 4 KB per wave for nothing the scalar unit does not do.
#include "ggms_internal.h"

namespace ggms {

constexpr uint32_t kEdgePosMaxLayers = 16;
constexpr uint32_t kEdgePosChunk = kWave;                              // edges of a wave
constexpr uint32_t kEdgePosWaves = kBlock / kWave;                     // 4
constexpr uint32_t kEdgePosUnit = kEdgePosChunk * kEdgePosWaves;       // edges of a workgroup per round: 256
constexpr uint32_t kEdgePosLong = 1024;                                // longer lists go to k_edgepos_long
constexpr uint32_t kEdgePosParts = 4;                                  // workgroups per queued chunk
constexpr uint32_t kEdgePosStripes = kEdgePosParts * kEdgePosWaves;    // waves a long list is spread over: 16
static_assert(kEdgePosWaves == 4, "a chunk's number is (unit << 2) | wave");

// all layers of a call, by value in the kernel arguments (the layer index is uniform per wave: scalar loads)
struct EdgePosJobs {
  const uint32_t *row[kEdgePosMaxLayers], *col[kEdgePosMaxLayers];
  uint32_t *eid[kEdgePosMaxLayers];
  uint64_t max_edges[kEdgePosMaxLayers];
  uint32_t unit_base[kEdgePosMaxLayers + 1]; // first unit of layer k in the launch's flat unit numbering
  uint32_t num_layer;
  __device__ __forceinline__ uint32_t layer_of(uint32_t flat) const {
    uint32_t k = 0;
#pragma unroll 1
    for (uint32_t j = 1; j < num_layer; ++j) k = flat >= unit_base[j] ? j : k;
    return k;
  }
};

struct EdgePosGraph {
  const uint32_t *indptr, *indices;
  const uint32_t *id_map; // NULL: row / col hold global ids
  uint32_t num_node, num_id_map;
};

// a wave's 64 edges: global ids, list bounds
struct EdgePosChunk {
  uint32_t t;        // the lane's target
  uint32_t b, len;   // its seed's list
  bool ok_s, ok_t, head;
};

__device__ __forceinline__ uint32_t edgepos_global(const EdgePosGraph &g, uint32_t local) {
  if (!g.id_map) return local;
  return local < g.num_id_map ? g.id_map[local] : kEmptyKey;
}

__device__ __forceinline__ EdgePosChunk edgepos_load(const EdgePosGraph &g, const uint32_t *__restrict__ row,
                                                     const uint32_t *__restrict__ col, uint64_t e, uint64_t n) {
  EdgePosChunk c;
  const bool in = e < n;
  const uint32_t cl = in ? col[e] : kEmptyKey;
  const uint32_t rl = in ? row[e] : kEmptyKey;
  const uint32_t s = edgepos_global(g, cl);
  c.t = edgepos_global(g, rl);
  c.ok_s = s < g.num_node; // (kEmptyKey is no node: num_node <= 2^32 - 1)
  c.ok_t = c.t < g.num_node;
  c.b = 0;
  c.len = 0;
  if (c.ok_s) {
    uint32_t end;
    GraphView::bounds(g.indptr, s, c.b, end);
    c.len = end - c.b;
  }
  const uint32_t prev = __shfl_up(s, 1, 64);
  c.head = lane_id() == 0 || s != prev;
  return c;
}

__device__ __forceinline__ uint32_t edgepos_readlane(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// pieces first, first + stride, ... of list [b, b + len) against the targets of the lanes in `open`; U pieces in flight.
// found: the lane's smallest position so far among the pieces this wave walks.
template <uint32_t U>
__device__ __forceinline__ uint32_t edgepos_match(const uint32_t *__restrict__ indices, uint32_t b, uint32_t len,
                                                  uint32_t first, uint32_t stride, uint32_t t, uint64_t open,
                                                  uint32_t found) {
  const uint32_t lane = lane_id();
  const uint32_t *__restrict__ const list = indices + (uint64_t)b;
  for (uint64_t c0 = first; c0 * kEdgePosChunk < len && open != 0ull; c0 += (uint64_t)U * stride) {
    uint32_t v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = (c0 + (uint64_t)u * stride) * kEdgePosChunk + lane;
      v[u] = p < len ? list[p] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t base = (c0 + (uint64_t)u * stride) * kEdgePosChunk;
      const bool in = base + lane < len;
      uint64_t it = open;
      while (it != 0ull) {
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(it));
        it &= it - 1ull;
        const uint32_t tj = edgepos_readlane(t, j);
        const uint64_t hit = __ballot(in && v[u] == tj);
        if (hit != 0ull) {
          const uint32_t pos = b + (uint32_t)base + (uint32_t)__builtin_ctzll(hit);
          if (lane == j) found = pos;
          open &= ~(1ull << j);
        }
      }
    }
  }
  return found;
}

__device__ __forceinline__ uint64_t edgepos_layer_edges(const uint64_t *counts, const EdgePosJobs &jobs, uint32_t k) {
  const uint64_t n = counts[GGMS_COUNT_EDGES(k)];
  return n < jobs.max_edges[k] ? n : jobs.max_edges[k]; // (a count beyond the bound is a caller error: nothing is read there)
}

// the runs of a chunk, one after the other; LONG picks the lists this kernel walks
template <bool LONG, uint32_t U>
__device__ __forceinline__ uint32_t edgepos_runs(const EdgePosGraph &g, const EdgePosChunk &c, uint32_t first,
                                                 uint32_t stride, bool &deferred) {
  uint32_t found = kEmptyKey;
  uint64_t heads = __ballot(c.head);
  const uint64_t targets = __ballot(c.ok_t);
  deferred = false;
  while (heads != 0ull) {
    const uint32_t h = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(heads));
    heads &= heads - 1ull;
    const uint64_t upto = heads != 0ull ? (heads & (~heads + 1ull)) - 1ull : ~0ull; // lanes below the next head
    const uint64_t open = upto & ~((1ull << h) - 1ull) & targets;
    const uint32_t len = edgepos_readlane(c.len, h);
    if (len == 0u || open == 0ull) continue; // (an invalid seed has len 0)
    if ((len > kEdgePosLong) != LONG) {
      deferred = deferred || !LONG;
      continue;
    }
    found = edgepos_match<U>(g.indices, edgepos_readlane(c.b, h), len, first, stride, c.t, open, found);
  }
  return found;
}

__global__ __launch_bounds__(kBlock) void k_edgepos_main(EdgePosJobs jobs, const uint64_t *__restrict__ counts,
                                                         EdgePosGraph g, uint32_t *qcount, uint32_t *__restrict__ queue) {
  const uint32_t total = jobs.unit_base[jobs.num_layer];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint32_t flat = blockIdx.x; flat < total; flat += gridDim.x) {
    const uint32_t k = jobs.layer_of(flat);
    const uint64_t n = edgepos_layer_edges(counts, jobs, k);
    const uint64_t e0 = (uint64_t)(flat - jobs.unit_base[k]) * kEdgePosUnit + wave * kEdgePosChunk;
    if (e0 >= n) continue; // uniform per wave
    const uint64_t e = e0 + lane_id();
    const EdgePosChunk c = edgepos_load(g, jobs.row[k], jobs.col[k], e, n);
    bool deferred;
    const uint32_t found = edgepos_runs<false, 1>(g, c, 0u, 1u, deferred);
    if (e < n) jobs.eid[k][e] = found;
    if (deferred && lane_id() == 0) queue[atomicAdd(qcount, 1u)] = (flat << 2) | wave;
  }
}

__global__ __launch_bounds__(kBlock) void k_edgepos_long(EdgePosJobs jobs, const uint64_t *__restrict__ counts,
                                                         EdgePosGraph g, const uint32_t *qcount,
                                                         const uint32_t *__restrict__ queue) {
  const uint64_t total = (uint64_t)*qcount * kEdgePosParts;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint64_t unit = blockIdx.x; unit < total; unit += gridDim.x) {
    const uint32_t chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)queue[unit / kEdgePosParts]);
    const uint32_t part = (uint32_t)(unit % kEdgePosParts);
    const uint32_t flat = chunk >> 2;
    const uint32_t k = jobs.layer_of(flat);
    const uint64_t n = edgepos_layer_edges(counts, jobs, k);
    const uint64_t e = (uint64_t)(flat - jobs.unit_base[k]) * kEdgePosUnit + (chunk & 3u) * kEdgePosChunk + lane_id();
    const EdgePosChunk c = edgepos_load(g, jobs.row[k], jobs.col[k], e, n);
    bool deferred;
    const uint32_t found = edgepos_runs<true, 4>(g, c, part * kEdgePosWaves + wave, kEdgePosStripes, deferred);
    if (found != kEmptyKey) atomicMin(jobs.eid[k] + e, found); // (found only by a lane with e < n)
  }
}

inline size_t edgepos_units_for(size_t n) { return (n + kEdgePosUnit - 1) / kEdgePosUnit; }
// the workspace: [counter, 16 bytes | one word per chunk of any layer], behind a 16-byte alignment of the caller's pointer
static bool edgepos_layout(const size_t *max_edges, uint32_t num_layer, uint64_t &units, size_t &bytes) {
  units = 0;
  for (uint32_t k = 0; k < num_layer; ++k) {
    if (max_edges[k] > 0xffffffffull) return false;
    units += edgepos_units_for(max_edges[k]);
  }
  if (units >= (1ull << 30)) return false; // a chunk's number is 32-bit
  bytes = 16 + 16 + (size_t)units * kEdgePosWaves * sizeof(uint32_t);
  return true;
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_edge_positions_workspace_bytes(const size_t *max_edges, uint32_t num_layer) {
  uint64_t units;
  size_t bytes;
  if (!max_edges || num_layer < 1 || num_layer > kEdgePosMaxLayers || !edgepos_layout(max_edges, num_layer, units, bytes))
    return 0;
  return bytes;
}

int ggms_edge_positions(const ggms_graph_t *graph, uint64_t num_edge, const ggms_id_t *id_map, size_t num_id_map,
                        const ggms_id_t *const *row, const ggms_id_t *const *col, ggms_id_t *const *eid,
                        const size_t *max_edges, uint32_t num_layer, const uint64_t *counts_dev, void *workspace,
                        size_t workspace_bytes, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph);
  if (graph->num_part != 0) {
    set_error("ggms_edge_positions: a sharded graph (num_part %u): a position is an index into ONE CSR", graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (num_edge >= 0xffffffffull) {
    set_error("ggms_edge_positions: %llu edges: positions are 32-bit and GGMS_EMPTY_KEY is none (at most 2^32 - 2)",
              (unsigned long long)num_edge);
    return GGMS_ERR_INVALID;
  }
  if (num_layer < 1 || num_layer > kEdgePosMaxLayers) {
    set_error("ggms_edge_positions: num_layer %u (1 .. %u)", num_layer, kEdgePosMaxLayers);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(graph->indptr && graph->indices && row && col && eid && max_edges && counts_dev);
  if (num_id_map > 0xffffffffull) num_id_map = 0xffffffffull; // local ids are 32-bit
  uint64_t units;
  size_t bytes;
  if (!edgepos_layout(max_edges, num_layer, units, bytes)) {
    set_error("ggms_edge_positions: a layer bound is out of range (layers of at most 2^32 - 1 edges, 2^38 in all)");
    return GGMS_ERR_INVALID;
  }
  if (!workspace || workspace_bytes < bytes) {
    set_error("ggms_edge_positions: workspace of %zu bytes, %zu needed (ggms_edge_positions_workspace_bytes)",
              workspace ? workspace_bytes : (size_t)0, bytes);
    return GGMS_ERR_INVALID;
  }
  EdgePosJobs jobs{};
  jobs.num_layer = num_layer;
  uint64_t at = 0;
  for (uint32_t k = 0; k < num_layer; ++k) {
    if (max_edges[k] != 0 && (!row[k] || !col[k] || !eid[k])) {
      set_error("ggms_edge_positions: row[%u] / col[%u] / eid[%u] is null", k, k, k);
      return GGMS_ERR_INVALID;
    }
    jobs.row[k] = row[k];
    jobs.col[k] = col[k];
    jobs.eid[k] = eid[k];
    jobs.max_edges[k] = max_edges[k];
    jobs.unit_base[k] = (uint32_t)at;
    at += edgepos_units_for(max_edges[k]);
  }
  jobs.unit_base[num_layer] = (uint32_t)at;
  if (units == 0) return GGMS_OK; // every bound is 0
  char *const ws = (char *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  uint32_t *const qcount = (uint32_t *)ws;
  uint32_t *const queue = (uint32_t *)(ws + 16);
  const EdgePosGraph g{graph->indptr, graph->indices, id_map, graph->num_node, (uint32_t)num_id_map};
  hipStream_t s = to_stream(stream);
  GGMS_HIP(hipMemsetAsync(qcount, 0, 16, s));
  hipLaunchKernelGGL(k_edgepos_main, dim3(grid_for((size_t)units, 1)), dim3(kBlock), 0, s, jobs, counts_dev, g, qcount,
                     queue);
  // kEdgePosParts workgroups per queued chunk; how many there are is only known on the device
  hipLaunchKernelGGL(k_edgepos_long, dim3(grid_for((size_t)units * kEdgePosWaves * kEdgePosParts, 1)), dim3(kBlock), 0, s,
                     jobs, counts_dev, g, (const uint32_t *)qcount, (const uint32_t *)queue);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
