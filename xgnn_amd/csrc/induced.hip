// induced.hip -- the subgraph a node set induces: every edge of the graph with both ends in the set, as one COO.
//
// There is no reference counterpart (DGL / PyG: ShaDowKHopSampler, GraphSAINT's node sampler, Cluster-GCN); the
// definition is in include/ggms.h (ggms_induced_edges) and tests/induced_ref.py restates it in numpy.  The call is a
// post-pass behind a finished batch, as ggms_edge_positions is: it reads the batch's node list and the CSR, and touches no
// sampler kernel.
//
// Membership is one caller-owned 32-bit word per node id (local_of), GGMS_EMPTY_KEY everywhere between calls.  Six
// launches per call, whatever n and M are (plus the scans' own: tile_scan.h):
//   k_induced_mark     atomicMin(local_of[nodes[j]], j): the word of a member holds the FIRST position that lists it, which
//                      is its local id and names the one position that owns its list (a repeated id emits once)
//   tile_scan          pre[j] = list entries of the owners before j; a position that does not own its id counts 0.  The
//                      total E (entries to walk) stays on the device
//   k_induced_count    the edge-tiled walk (edge_tiles.h): one random 4-byte read of local_of per entry; a tile's number of
//                      members goes to tile_hits[tile]
//   tile_scan          tile_base[t] = hits of the tiles before t; the total M goes to out_counts_dev[0]
//   k_induced_emit     the same walk again, looking local_of up again (below).  A lane knows each entry's owner and address
//                      from the walk (walk_edge_tiles_where); its rank inside the round comes from one ballot per
//                      register slot and a 32-word workgroup prefix, the rounds of a tile add up in a register, the tile's
//                      base comes from the scan: the output position is a function of the edge's position alone, so the
//                      result is the same bit for bit whatever grid runs it
//   k_induced_unmark   local_of[nodes[j]] = GGMS_EMPTY_KEY: the map is clean again, at the cost of the batch, not the graph
//
// Why the second walk looks the map up again instead of reading hit flags the first one left behind: the flags would be
// a bit per walked entry laid out by (tile, round, slot, lane) -- rounds are data dependent, so the layout needs a word
// per lane and round, 4 bytes written and read per 8 entries and a workspace that grows with num_edge / 2 bytes -- to
// save a read that the first walk has just pulled into the cache hierarchy (a batch's neighbourhood is far smaller than
// the map).  Not measured against each other; DESIGN.md 8l says so.
#include "edge_tiles.h"

namespace ggms {

namespace {

struct InducedCtl {
  uint64_t n;     // nodes of this call (clamped to max_nodes)
  uint64_t edges; // list entries of the owners: the walked total E
  uint64_t tiles; // edge tiles of the walk (clamped to the workspace's tile words)
  uint64_t _pad[5];
};

inline size_t induced_pre_words(size_t max_nodes) { return (max_nodes + 3) & ~(size_t)3; }
inline size_t induced_tile_words(uint64_t num_edge) {
  const uint64_t e = num_edge < 0xffffffffull ? num_edge : 0xffffffffull;
  const size_t t = (size_t)((e + kEdgeTile - 1) / kEdgeTile) + 1;
  return (t + 3) & ~(size_t)3;
}

__global__ __launch_bounds__(kBlock) void k_induced_mark(const uint32_t *__restrict__ nodes, uint64_t max_nodes,
                                                         const uint64_t *num_nodes_dev, uint32_t *local_of,
                                                         uint32_t num_node, InducedCtl *ctl) {
  uint64_t n = num_nodes_dev ? *num_nodes_dev : max_nodes;
  n = n < max_nodes ? n : max_nodes;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n = n;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t v = nodes[j];
    if (v < num_node) atomicMin(local_of + v, (uint32_t)j);
  }
}

__global__ __launch_bounds__(kBlock) void k_induced_unmark(const uint32_t *__restrict__ nodes, const InducedCtl *ctl,
                                                           uint32_t *local_of, uint32_t num_node) {
  const uint64_t n = ctl->n;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t v = nodes[j];
    if (v < num_node) local_of[v] = kEmptyKey;
  }
}

__global__ void k_induced_kept(const uint64_t *counts, uint64_t max_edges, uint64_t *kept) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *kept = counts[0] < max_edges ? counts[0] : max_edges;
}

// scan value: the degree of position j if it owns its id, else 0
struct OwnerDegree {
  GraphView g;
  const uint32_t *nodes;
  const uint32_t *local_of;
  uint32_t num_node;
  __device__ __forceinline__ uint32_t operator()(uint64_t j) const {
    const uint32_t u = nodes[j];
    if (u >= num_node || local_of[u] != (uint32_t)j) return 0u;
    uint32_t len;
    g.neighbours(u, len);
    return len;
  }
};
struct TileHits {
  const uint32_t *hits;
  __device__ __forceinline__ uint32_t operator()(uint64_t t) const { return hits[t]; }
};

// the local ids of a round's entries (kEmptyKey: not in the set); all loads are issued before any is looked at
__device__ __forceinline__ uint32_t induced_lookup(const uint32_t *__restrict__ local_of, uint32_t num_node,
                                                   const uint32_t (&v)[kPerThread], uint32_t have,
                                                   uint32_t (&loc)[kPerThread]) {
#pragma unroll
  for (uint32_t k = 0; k < kPerThread; ++k)
    loc[k] = (((have >> k) & 1u) && v[k] < num_node) ? local_of[v[k]] : kEmptyKey;
  uint32_t hit = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPerThread; ++k) hit |= loc[k] != kEmptyKey ? 1u << k : 0u;
  return hit;
}

__global__ __launch_bounds__(kBlock) void k_induced_count(GraphView g, const uint32_t *__restrict__ nodes,
                                                          const uint32_t *__restrict__ pre, InducedCtl *ctl,
                                                          const uint32_t *__restrict__ local_of, uint32_t num_node,
                                                          uint32_t *__restrict__ tile_hits, uint64_t max_tiles,
                                                          uint64_t *out_counts) {
  __shared__ uint32_t smem[kBlock / kWave];
  const uint64_t F = ctl->n;
  const uint64_t E = ctl->edges;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t tiles = (E + kEdgeTile - 1) / kEdgeTile;
    ctl->tiles = tiles < max_tiles ? tiles : max_tiles;
    out_counts[1] = E;
  }
  uint32_t run = 0; // hits of the tile's earlier rounds (thread 0)
  walk_edge_tiles_where(g, nodes, F, pre, E, num_node,
                        [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t cur, const uint32_t (&)[kPerThread],
                            const uint32_t *const (&)[kPerThread]) {
                          uint32_t loc[kPerThread];
                          const uint32_t hit = induced_lookup(local_of, num_node, v, have, loc);
                          const uint32_t c = wave_reduce_sum((uint32_t)__builtin_popcount(hit));
                          if (lane_id() == 0) smem[threadIdx.x >> 6] = c;
                          __syncthreads(); // (smem is rewritten behind the walk's own barrier)
                          if (threadIdx.x == 0) {
                            const uint64_t t = cur / kEdgeTile;
                            if (cur % kEdgeTile == 0) run = 0;
                            run += smem[0] + smem[1] + smem[2] + smem[3];
                            if (t < max_tiles) tile_hits[t] = run; // the tile's last round leaves its total
                          }
                        });
}

struct InducedOut {
  uint32_t *row, *col, *eid; // eid may be NULL
  uint64_t max_edges;
};

__global__ __launch_bounds__(kBlock) void k_induced_emit(GraphView g, const uint32_t *__restrict__ nodes,
                                                         const uint32_t *__restrict__ pre, const InducedCtl *ctl,
                                                         const uint32_t *__restrict__ local_of, uint32_t num_node,
                                                         const uint32_t *__restrict__ tile_base, uint64_t max_tiles,
                                                         InducedOut o) {
  __shared__ uint32_t s_cnt[kPerThread][kBlock / kWave];
  const uint64_t F = ctl->n;
  const uint64_t E = ctl->edges;
  const uint32_t w = threadIdx.x >> 6;
  uint32_t run = 0; // hits of the tile's earlier rounds (every thread: the same sum)
  walk_edge_tiles_where(
      g, nodes, F, pre, E, num_node,
      [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t cur, const uint32_t (&own)[kPerThread],
          const uint32_t *const (&ent)[kPerThread]) {
        uint32_t loc[kPerThread];
        const uint32_t hit = induced_lookup(local_of, num_node, v, have, loc);
        // edge order inside a round: slot k, then thread -- a ballot per slot, a prefix over (slot, wave)
        uint32_t below[kPerThread];
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; ++k) {
          const uint64_t b = __ballot((hit >> k) & 1u);
          below[k] = (uint32_t)__popcll(b & ((1ull << lane_id()) - 1ull));
          if (lane_id() == 0) s_cnt[k][w] = (uint32_t)__popcll(b);
        }
        __syncthreads(); // (s_cnt is rewritten behind the walk's own barrier)
        const uint64_t t = cur / kEdgeTile;
        if (cur % kEdgeTile == 0) run = 0;
        if (t >= max_tiles) return; // uniform; only if the caller's num_edge was not the graph's
        const uint64_t base = (uint64_t)tile_base[t] + run;
        uint32_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; ++k) {
#pragma unroll
          for (uint32_t x = 0; x < kBlock / kWave; ++x) {
            const uint32_t c = s_cnt[k][x];
            if (x == w) {
              const uint64_t at = base + acc + below[k];
              if (((hit >> k) & 1u) && at < o.max_edges) {
                o.row[at] = loc[k];
                o.col[at] = own[k];
                if (o.eid) o.eid[at] = (uint32_t)(ent[k] - g.indices);
              }
            }
            acc += c;
          }
        }
        run += acc;
      });
}

} // namespace

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_induced_edges_workspace_bytes(size_t max_nodes, uint64_t num_edge) {
  const size_t tw = induced_tile_words(num_edge);
  return 16 + sizeof(InducedCtl) +
         4 * (induced_pre_words(max_nodes) + 2 * tw + edge_scan_words(max_nodes) + 2 + edge_scan_words(tw) + 2);
}

int ggms_induced_map_init(uint32_t *local_of, size_t num_node, ggms_stream_t stream) {
  if (num_node == 0) return GGMS_OK;
  if (!local_of) {
    set_error("ggms_induced_map_init: local_of is null");
    return GGMS_ERR_INVALID;
  }
  GGMS_HIP(hipMemsetAsync(local_of, 0xff, num_node * sizeof(uint32_t), to_stream(stream)));
  return GGMS_OK;
}

int ggms_induced_kept(const uint64_t *counts_dev, size_t max_edges, uint64_t *kept_dev, ggms_stream_t stream) {
  if (!counts_dev || !kept_dev) {
    set_error("ggms_induced_kept: counts_dev / kept_dev is null");
    return GGMS_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_induced_kept, dim3(1), dim3(kWave), 0, to_stream(stream), counts_dev, (uint64_t)max_edges, kept_dev);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

int ggms_induced_edges(const ggms_graph_t *graph, uint64_t num_edge, const ggms_id_t *nodes, size_t max_nodes,
                       const uint64_t *num_nodes_dev, uint32_t *local_of, ggms_id_t *row, ggms_id_t *col,
                       ggms_id_t *eid, size_t max_edges, uint64_t *out_counts_dev, void *workspace,
                       size_t workspace_bytes, ggms_stream_t stream) {
  if (!graph || !out_counts_dev) {
    set_error("ggms_induced_edges: graph / out_counts_dev is null");
    return GGMS_ERR_INVALID;
  }
  if (num_edge >= 0xffffffffull) {
    set_error("ggms_induced_edges: %llu edges: positions are 32-bit and GGMS_EMPTY_KEY is none (at most 2^32 - 2)",
              (unsigned long long)num_edge);
    return GGMS_ERR_INVALID;
  }
  if ((uint64_t)max_nodes >= 0xffffffffull - 1023ull) {
    set_error("ggms_induced_edges: max_nodes %zu: local ids are 32-bit (below 2^32 - 1024)", max_nodes);
    return GGMS_ERR_INVALID;
  }
  if (eid && graph->num_part != 0) {
    set_error("ggms_induced_edges: eid on a sharded graph (num_part %u): a position is an index into ONE CSR; pass "
              "eid = NULL",
              graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (max_nodes != 0) {
    if (!nodes || !local_of || (max_edges != 0 && (!row || !col))) {
      set_error("ggms_induced_edges: nodes / local_of / row / col is null");
      return GGMS_ERR_INVALID;
    }
    if (graph->num_part == 0 && (!graph->indptr || !graph->indices)) {
      set_error("ggms_induced_edges: graph->indptr / graph->indices is null");
      return GGMS_ERR_INVALID;
    }
    const size_t need = ggms_induced_edges_workspace_bytes(max_nodes, num_edge);
    if (!workspace || workspace_bytes < need) {
      set_error("ggms_induced_edges: workspace of %zu bytes, %zu needed (ggms_induced_edges_workspace_bytes)",
                workspace ? workspace_bytes : (size_t)0, need);
      return GGMS_ERR_INVALID;
    }
  }
  hipStream_t s = to_stream(stream);
  if (max_nodes == 0) {
    GGMS_HIP(hipMemsetAsync(out_counts_dev, 0, 2 * sizeof(uint64_t), s));
    return GGMS_OK;
  }
  GraphView g;
  if (!view_of(graph, g)) return GGMS_ERR_INVALID;
  const uint32_t N = graph->num_node;
  const size_t tw = induced_tile_words(num_edge);
  char *const ws = (char *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  InducedCtl *ctl = (InducedCtl *)ws;
  uint32_t *pre = (uint32_t *)(ctl + 1);
  uint32_t *tile_hits = pre + induced_pre_words(max_nodes);
  uint32_t *tile_base = tile_hits + tw;
  uint32_t *scan_nodes = tile_base + tw;
  uint32_t *scan_tiles = scan_nodes + edge_scan_words(max_nodes) + 2;

  hipLaunchKernelGGL(k_induced_mark, dim3(grid_for(max_nodes, kBlock)), dim3(kBlock), 0, s, nodes, (uint64_t)max_nodes,
                     num_nodes_dev, local_of, N, ctl);
  GGMS_LAUNCH_CHECK();
  int rc = tile_scan(OwnerDegree{g, nodes, local_of, N}, StorePrefix{pre}, max_nodes, count_of(max_nodes, &ctl->n),
                     ScanArea{scan_nodes, false}, nullptr, nullptr, &ctl->edges, s);
  if (rc != GGMS_OK) return rc;
  // persistent grids: the walked total is only known on the device
  hipLaunchKernelGGL(k_induced_count, dim3(grid_cap()), dim3(kBlock), 0, s, g, nodes, (const uint32_t *)pre, ctl,
                     (const uint32_t *)local_of, N, tile_hits, (uint64_t)tw, out_counts_dev);
  GGMS_LAUNCH_CHECK();
  rc = tile_scan(TileHits{tile_hits}, StorePrefix{tile_base}, tw, count_of(tw, &ctl->tiles), ScanArea{scan_tiles, false},
                 nullptr, nullptr, out_counts_dev, s);
  if (rc != GGMS_OK) return rc;
  const InducedOut o{row, col, eid, max_edges < 0xffffffffull ? (uint64_t)max_edges : 0xffffffffull};
  hipLaunchKernelGGL(k_induced_emit, dim3(grid_cap()), dim3(kBlock), 0, s, g, nodes, (const uint32_t *)pre,
                     (const InducedCtl *)ctl, (const uint32_t *)local_of, N, (const uint32_t *)tile_base, (uint64_t)tw, o);
  GGMS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_induced_unmark, dim3(grid_for(max_nodes, kBlock)), dim3(kBlock), 0, s, nodes,
                     (const InducedCtl *)ctl, local_of, N);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
