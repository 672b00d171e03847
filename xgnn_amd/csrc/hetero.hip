// hetero.hip -- the heterogeneous view of a sampled batch: nodes grouped by node type, every layer's edges grouped by
// relation and renumbered into their types' lists.
//
// There is no reference counterpart; the definitions are in include/ggms.h (ggms_hetero_nodes, ggms_hetero_edges) and
// tests/hetero_ref.py restates them in numpy.  Both calls are post-passes behind a finished batch and both are the same
// stable multi-way partition with at most 32 buckets -- radix_sort.h's per-digit machinery with one "digit" and a payload:
//   k_split_count   tiles of 2048 items; a tile's bucket histogram goes to hist[bucket][tile] (one row more than there are
//                   buckets, all zero: its scanned value is the job's end).  For the nodes this launch also does the one
//                   random read of the call, node_type[nodes[i]], and leaves the byte in ntype for the emit.
//   tile_scan       ONE exclusive scan over (jobs x) buckets x tiles: every (bucket, tile) gets its global base, the
//                   values of a bucket's first tile are base[] / off[].
//   k_split_emit    waves own consecutive 64-item chunks of a tile (8 each).  A lane's rank among the equal keys of its
//                   chunk comes from ballots, one per DISTINCT key present in the wave (readlane + ballot: khop_typed emits
//                   a seed's edges in ascending type, so a wave holds a few runs), the chunks' bases from an LDS table
//                   filled in chunk order; the payload is applied in the same pass.  All of a wave's loads -- for the
//                   edges the two dependent look-ups local[row[e]] / local[col[e]] of its eight chunks -- are issued
//                   before its first store.
//   k_hetero_cuts   (nodes only) one workgroup per cut: the scanned histogram gives the count of the whole tiles before
//                   the cut, the cut's own tile is counted from ntype (at most 2047 bytes).
// An item's position is a function of its index alone: no atomic decides an order (the LDS atomics only count), so the
// output does not depend on the grid.  A job is the node list or one layer; all layers of ggms_hetero_edges share each
// launch.  Launches per call: one memset at most (the scan's control words), count, scan (1 or 3), emit (+ cuts).
#include "ggms_internal.h"

namespace ggms {

constexpr uint32_t kSplitTile = 2048;                                   // items of a workgroup per round
constexpr uint32_t kSplitMaxJobs = 16;
constexpr uint32_t kSplitMaxBuckets = 32;
constexpr uint32_t kSplitWaves = kBlock / kWave;                        // 4
constexpr uint32_t kSplitChunks = kSplitTile / kWave / kSplitWaves;     // 64-item chunks per wave: 8
constexpr uint64_t kSplitMaxItems = 0xffffffffull - 1024ull;            // bound of a job (exclusive)
static_assert(kSplitMaxBuckets <= kWave && kSplitMaxBuckets < kBlock, "one thread per bucket row");

// the tiles of all jobs in one flat numbering; job k's histogram is hist[hist_base[k] + bucket * tiles(k) + tile],
// bucket = 0 .. buckets (the last row stays zero).  Every job has at least one tile, so that its totals get written.
struct SplitPlan {
  uint32_t tile_base[kSplitMaxJobs + 1];
  uint32_t hist_base[kSplitMaxJobs + 1];
  uint32_t num_job, buckets;
  __device__ __forceinline__ uint32_t job_of(uint32_t flat) const {
    uint32_t k = 0;
#pragma unroll 1
    for (uint32_t j = 1; j < num_job; ++j) k = flat >= tile_base[j] ? j : k;
    return k;
  }
};

struct SplitPayload {
  uint32_t a, b, c;
};

// the lanes of the wave whose (valid) key equals mine: one ballot per distinct key present
__device__ __forceinline__ uint64_t same_key_mask(uint32_t key, bool valid) {
  uint64_t todo = __ballot(valid), mine = 0ull;
  while (todo != 0ull) {
    const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)l);
    const uint64_t m = __ballot(valid && key == k); // holds lane l: the loop ends
    if (valid && key == k) mine = m;
    todo &= ~m;
  }
  return mine;
}

// ---- the nodes -------------------------------------------------------------------------------------------------------
struct NodeSplit {
  const uint8_t *node_type;
  const uint32_t *nodes;
  const uint64_t *n_dev;
  uint64_t max_nodes;
  uint32_t num_node, num_type;
  uint8_t *ntype;
  uint32_t *local, *slot, *typed_nodes, *base;
  __device__ __forceinline__ uint64_t count(uint32_t) const {
    const uint64_t n = n_dev ? *n_dev : max_nodes;
    return n < max_nodes ? n : max_nodes;
  }
  __device__ __forceinline__ uint32_t count_key(uint32_t, uint64_t i) const { // the call's one random read
    const uint32_t id = nodes[i];
    uint32_t t = 0xffu;
    if (id < num_node) t = node_type[id];
    if (t >= num_type) t = 0xffu;
    ntype[i] = (uint8_t)t;
    return t;
  }
  __device__ __forceinline__ uint32_t emit_key(uint32_t, uint64_t i) const { return ntype[i]; }
  __device__ __forceinline__ SplitPayload load(uint32_t, uint64_t i, bool valid) const {
    return SplitPayload{valid ? nodes[i] : 0u, 0u, 0u};
  }
  // pos: the item's position among the job's valid items in bucket order; rank: among its bucket's
  __device__ __forceinline__ void store(uint32_t, uint64_t i, const SplitPayload &v, uint32_t pos, uint32_t rank) const {
    local[i] = rank;
    slot[i] = pos;
    typed_nodes[pos] = v.a;
  }
  __device__ __forceinline__ void store_invalid(uint32_t, uint64_t i) const {
    local[i] = kEmptyKey;
    slot[i] = kEmptyKey;
  }
  __device__ __forceinline__ void total(uint32_t, uint32_t bucket, uint32_t before) const { base[bucket] = before; }
};

// ---- the layers' edges -------------------------------------------------------------------------------------------------
struct EdgeSplit {
  const uint32_t *row[kSplitMaxJobs], *col[kSplitMaxJobs], *eid[kSplitMaxJobs];
  const uint8_t *etype[kSplitMaxJobs];
  uint32_t *out_row[kSplitMaxJobs], *out_col[kSplitMaxJobs], *out_eid[kSplitMaxJobs];
  uint64_t max_edges[kSplitMaxJobs];
  const uint64_t *counts;
  const uint32_t *local;
  uint32_t *rel_offsets;
  uint32_t num_local, num_rel;
  __device__ __forceinline__ uint64_t count(uint32_t k) const {
    const uint64_t n = counts[GGMS_COUNT_EDGES(k)];
    return n < max_edges[k] ? n : max_edges[k];
  }
  __device__ __forceinline__ uint32_t count_key(uint32_t k, uint64_t e) const { return etype[k][e]; }
  __device__ __forceinline__ uint32_t emit_key(uint32_t k, uint64_t e) const { return etype[k][e]; }
  __device__ __forceinline__ SplitPayload load(uint32_t k, uint64_t e, bool valid) const {
    SplitPayload v{kEmptyKey, kEmptyKey, 0u};
    if (valid) {
      const uint32_t r = row[k][e], c = col[k][e];
      if (eid[k]) v.c = eid[k][e];
      if (r < num_local) v.a = local[r];
      if (c < num_local) v.b = local[c];
    }
    return v;
  }
  __device__ __forceinline__ void store(uint32_t k, uint64_t, const SplitPayload &v, uint32_t pos, uint32_t) const {
    out_row[k][pos] = v.a;
    out_col[k][pos] = v.b;
    if (out_eid[k]) out_eid[k][pos] = v.c;
  }
  __device__ __forceinline__ void store_invalid(uint32_t, uint64_t) const {}
  __device__ __forceinline__ void total(uint32_t k, uint32_t bucket, uint32_t before) const {
    rel_offsets[(uint64_t)k * (num_rel + 1u) + bucket] = before;
  }
};

// ---- count -----------------------------------------------------------------------------------------------------------
template <typename P>
__global__ __launch_bounds__(kBlock) void k_split_count(P p, SplitPlan plan, uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[kSplitMaxBuckets];
  const uint32_t total = plan.tile_base[plan.num_job];
  const uint32_t B = plan.buckets;
  for (uint32_t flat = blockIdx.x; flat < total; flat += gridDim.x) {
    const uint32_t k = plan.job_of(flat);
    const uint32_t tiles = plan.tile_base[k + 1] - plan.tile_base[k], tile = flat - plan.tile_base[k];
    const uint64_t n = p.count(k);
    if (threadIdx.x < kSplitMaxBuckets) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t tile_start = (uint64_t)tile * kSplitTile;
    if (tile_start < n) { // uniform
#pragma unroll
      for (uint32_t c = 0; c < kSplitTile / kBlock; ++c) {
        const uint64_t i = tile_start + c * kBlock + threadIdx.x;
        const uint32_t key = i < n ? p.count_key(k, i) : 0xffffffffu;
        const bool valid = key < B;
        const uint64_t same = same_key_mask(key, valid);
        if (valid && lane_id() == (uint32_t)__builtin_ctzll(same)) atomicAdd(&h[key], (uint32_t)__popcll(same));
      }
    }
    __syncthreads();
    if (threadIdx.x <= B) // (zero beyond n, and in the closing row)
      hist[(uint64_t)plan.hist_base[k] + (uint64_t)threadIdx.x * tiles + tile] = threadIdx.x < B ? h[threadIdx.x] : 0u;
    __syncthreads();
  }
}

struct SplitHistValue {
  const uint32_t *hist;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return hist[i]; }
};
struct SplitHistStore {
  uint32_t *hist;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { hist[i] = excl; }
};

// ---- emit ------------------------------------------------------------------------------------------------------------
template <typename P>
__global__ __launch_bounds__(kBlock) void k_split_emit(P p, SplitPlan plan, const uint32_t *__restrict__ hist) {
  __shared__ uint32_t wave_cnt[kSplitWaves][kSplitMaxBuckets]; // a bucket's items so far inside the tile, per wave
  __shared__ uint32_t base[kSplitMaxBuckets];                   // scanned value of (bucket, this tile)
  __shared__ uint32_t first[kSplitMaxBuckets];                  // scanned value of (bucket, tile 0): the bucket's start
  const uint32_t total = plan.tile_base[plan.num_job];
  const uint32_t B = plan.buckets;
  const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
  for (uint32_t flat = blockIdx.x; flat < total; flat += gridDim.x) {
    const uint32_t k = plan.job_of(flat);
    const uint32_t tiles = plan.tile_base[k + 1] - plan.tile_base[k], tile = flat - plan.tile_base[k];
    const uint32_t *__restrict__ const h = hist + plan.hist_base[k];
    const uint64_t n = p.count(k);
    const uint32_t job0 = h[0]; // the scan runs through all jobs: positions are relative to the job's first value
    if (tile == 0 && threadIdx.x <= B) p.total(k, threadIdx.x, h[(uint64_t)threadIdx.x * tiles] - job0);
    const uint64_t tile_start = (uint64_t)tile * kSplitTile;
    if (tile_start >= n) continue; // uniform per workgroup
    if (threadIdx.x < kSplitMaxBuckets) {
      const bool in = threadIdx.x < B;
      base[threadIdx.x] = in ? h[(uint64_t)threadIdx.x * tiles + tile] : 0u;
      first[threadIdx.x] = in ? h[(uint64_t)threadIdx.x * tiles] : 0u;
#pragma unroll
      for (uint32_t w = 0; w < kSplitWaves; ++w) wave_cnt[w][threadIdx.x] = 0u;
    }
    __syncthreads();
    // every load of the wave's eight chunks, the dependent look-ups included, before the first store
    uint32_t key[kSplitChunks], inw[kSplitChunks];
    SplitPayload v[kSplitChunks];
#pragma unroll
    for (uint32_t c = 0; c < kSplitChunks; ++c) {
      const uint64_t i = tile_start + (uint64_t)(wave * kSplitChunks + c) * kWave + lane;
      key[c] = i < n ? p.emit_key(k, i) : 0xffffffffu;
    }
#pragma unroll
    for (uint32_t c = 0; c < kSplitChunks; ++c) {
      const uint64_t i = tile_start + (uint64_t)(wave * kSplitChunks + c) * kWave + lane;
      v[c] = p.load(k, i, key[c] < B);
    }
    // chunks in order: rank inside the chunk by ballots, the wave's earlier chunks from its LDS row
#pragma unroll
    for (uint32_t c = 0; c < kSplitChunks; ++c) {
      const bool valid = key[c] < B;
      const uint64_t same = same_key_mask(key[c], valid);
      const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
      uint32_t before = 0;
      if (valid) before = wave_cnt[wave][key[c]];
      __builtin_amdgcn_wave_barrier();
      if (valid && rank == 0u) wave_cnt[wave][key[c]] = before + (uint32_t)__popcll(same); // one lane per key
      __builtin_amdgcn_wave_barrier();
      inw[c] = before + rank;
    }
    __syncthreads();
    if (threadIdx.x < kSplitMaxBuckets) { // exclusive prefix over the waves, per bucket
      uint32_t run = 0;
#pragma unroll
      for (uint32_t w = 0; w < kSplitWaves; ++w) {
        const uint32_t cnt = wave_cnt[w][threadIdx.x];
        wave_cnt[w][threadIdx.x] = run;
        run += cnt;
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < kSplitChunks; ++c) {
      const uint64_t i = tile_start + (uint64_t)(wave * kSplitChunks + c) * kWave + lane;
      if (i < n) {
        if (key[c] < B) {
          const uint32_t g = base[key[c]] + wave_cnt[wave][key[c]] + inw[c];
          p.store(k, i, v[c], g - job0, g - first[key[c]]);
        } else {
          p.store_invalid(k, i);
        }
      }
    }
    __syncthreads(); // the LDS tables are rewritten next round
  }
}

// ---- the cut counts ----------------------------------------------------------------------------------------------------
struct HeteroCuts {
  uint32_t word[GGMS_HETERO_MAX_CUTS];
};

// workgroup k: the types of nodes[0, min(cut_k, n)) -- whole tiles from the scanned histogram, the rest from ntype
__global__ __launch_bounds__(kBlock) void k_hetero_cuts(NodeSplit p, uint32_t tiles, const uint32_t *__restrict__ hist,
                                                        const uint64_t *__restrict__ cut_base, HeteroCuts cuts,
                                                        uint32_t *__restrict__ cut_counts) {
  __shared__ uint32_t h[kSplitMaxBuckets];
  const uint32_t T = p.num_type;
  const uint64_t n = p.count(0);
  uint64_t c = cut_base[cuts.word[blockIdx.x]];
  c = c < n ? c : n;
  const uint64_t tile = c / kSplitTile; // <= tiles: n <= max_nodes <= tiles * kSplitTile
  if (threadIdx.x < kSplitMaxBuckets) h[threadIdx.x] = 0u;
  __syncthreads();
  if (tile < tiles)
    for (uint64_t i = tile * kSplitTile + threadIdx.x; i < c; i += kBlock) {
      const uint32_t t = p.ntype[i];
      if (t < T) atomicAdd(&h[t], 1u);
    }
  __syncthreads();
  if (threadIdx.x < T) {
    const uint64_t r = (uint64_t)threadIdx.x * tiles;
    const uint32_t whole = tile < tiles ? hist[r + tile] - hist[r] : hist[r + tiles] - hist[r]; // (row T closes the last)
    cut_counts[(uint64_t)blockIdx.x * T + threadIdx.x] = whole + h[threadIdx.x];
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
inline size_t split_tiles_for(size_t n) {
  const size_t t = (n + kSplitTile - 1) / kSplitTile;
  return t ? t : 1;
}
// the workspace: [histogram | scan scratch], behind a 16-byte alignment of the caller's pointer
static bool split_plan(const size_t *max_items, uint32_t num_job, uint32_t buckets, SplitPlan &plan, size_t &words,
                       size_t &bytes) {
  uint64_t tiles = 0, hist = 0;
  plan.num_job = num_job;
  plan.buckets = buckets;
  for (uint32_t k = 0; k < num_job; ++k) {
    if ((uint64_t)max_items[k] >= kSplitMaxItems) return false;
    plan.tile_base[k] = (uint32_t)tiles;
    plan.hist_base[k] = (uint32_t)hist;
    const uint64_t t = split_tiles_for(max_items[k]);
    tiles += t;
    hist += t * (buckets + 1u);
    if (hist >= (1ull << 31)) return false; // positions and histogram indices are 32-bit
  }
  for (uint32_t k = num_job; k <= kSplitMaxJobs; ++k) {
    plan.tile_base[k] = (uint32_t)tiles;
    plan.hist_base[k] = (uint32_t)hist;
  }
  words = (size_t)hist;
  bytes = 16 + (words + 2 + tile_scan_words(words)) * sizeof(uint32_t);
  return true;
}

template <typename P>
static int split_run(const P &p, const SplitPlan &plan, size_t words, void *workspace, hipStream_t s, uint32_t **hist_out) {
  uint32_t *const hist = (uint32_t *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  uint32_t *const scratch = hist + words;
  const int grid = grid_for(plan.tile_base[plan.num_job], 1);
  hipLaunchKernelGGL(k_split_count<P>, dim3(grid), dim3(kBlock), 0, s, p, plan, hist);
  GGMS_LAUNCH_CHECK();
  const int rc = tile_scan(SplitHistValue{hist}, SplitHistStore{hist}, words, count_of(words), ScanArea{scratch, false},
                           nullptr, nullptr, nullptr, s);
  if (rc != GGMS_OK) return rc;
  hipLaunchKernelGGL(k_split_emit<P>, dim3(grid), dim3(kBlock), 0, s, p, plan, (const uint32_t *)hist);
  GGMS_LAUNCH_CHECK();
  *hist_out = hist;
  return GGMS_OK;
}

#define GGMS_HETERO_ARG(fn, arg)                               \
  do {                                                         \
    if (!(arg)) {                                              \
      set_error(fn ": invalid argument: " #arg " is null");    \
      return GGMS_ERR_INVALID;                                 \
    }                                                          \
  } while (0)

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_hetero_nodes_workspace_bytes(size_t max_nodes, uint32_t num_type) {
  SplitPlan plan;
  size_t words, bytes;
  if (num_type < 1 || num_type > GGMS_MAX_NODE_TYPES || !split_plan(&max_nodes, 1, num_type, plan, words, bytes)) return 0;
  return bytes;
}

int ggms_hetero_nodes(const uint8_t *node_type, size_t num_node, uint32_t num_type, const ggms_id_t *nodes,
                      size_t max_nodes, const uint64_t *num_nodes_dev, const uint64_t *cut_base_dev,
                      const uint32_t *cut_words_host, uint32_t num_cut, uint8_t *ntype, uint32_t *local, uint32_t *slot,
                      ggms_id_t *typed_nodes, uint32_t *base_dev, uint32_t *cut_counts_dev, void *workspace,
                      size_t workspace_bytes, ggms_stream_t stream) {
  if (num_type < 1 || num_type > GGMS_MAX_NODE_TYPES) {
    set_error("ggms_hetero_nodes: num_type %u (1 .. %d)", num_type, GGMS_MAX_NODE_TYPES);
    return GGMS_ERR_INVALID;
  }
  if (num_cut > GGMS_HETERO_MAX_CUTS) {
    set_error("ggms_hetero_nodes: num_cut %u (at most %d)", num_cut, GGMS_HETERO_MAX_CUTS);
    return GGMS_ERR_INVALID;
  }
  GGMS_HETERO_ARG("ggms_hetero_nodes", node_type);
  GGMS_HETERO_ARG("ggms_hetero_nodes", nodes);
  GGMS_HETERO_ARG("ggms_hetero_nodes", ntype);
  GGMS_HETERO_ARG("ggms_hetero_nodes", local);
  GGMS_HETERO_ARG("ggms_hetero_nodes", slot);
  GGMS_HETERO_ARG("ggms_hetero_nodes", typed_nodes);
  GGMS_HETERO_ARG("ggms_hetero_nodes", base_dev);
  if (num_cut != 0) {
    GGMS_HETERO_ARG("ggms_hetero_nodes", cut_base_dev);
    GGMS_HETERO_ARG("ggms_hetero_nodes", cut_words_host);
    GGMS_HETERO_ARG("ggms_hetero_nodes", cut_counts_dev);
  }
  SplitPlan plan;
  size_t words, bytes;
  if (!split_plan(&max_nodes, 1, num_type, plan, words, bytes)) {
    set_error("ggms_hetero_nodes: max_nodes %zu (below 2^32 - 1024)", max_nodes);
    return GGMS_ERR_INVALID;
  }
  if (!workspace || workspace_bytes < bytes) {
    set_error("ggms_hetero_nodes: workspace of %zu bytes, %zu needed (ggms_hetero_nodes_workspace_bytes)",
              workspace ? workspace_bytes : (size_t)0, bytes);
    return GGMS_ERR_INVALID;
  }
  NodeSplit p{};
  p.node_type = node_type;
  p.nodes = nodes;
  p.n_dev = num_nodes_dev;
  p.max_nodes = max_nodes;
  p.num_node = num_node > 0xffffffffull ? 0xffffffffu : (uint32_t)num_node; // (GGMS_EMPTY_KEY is no node)
  p.num_type = num_type;
  p.ntype = ntype;
  p.local = local;
  p.slot = slot;
  p.typed_nodes = typed_nodes;
  p.base = base_dev;
  hipStream_t s = to_stream(stream);
  uint32_t *hist = nullptr;
  const int rc = split_run(p, plan, words, workspace, s, &hist);
  if (rc != GGMS_OK) return rc;
  if (num_cut != 0) {
    HeteroCuts cuts{};
    for (uint32_t k = 0; k < num_cut; ++k) cuts.word[k] = cut_words_host[k];
    // a fixed shape: one workgroup per cut, not capped by GGMS_DEBUG_GRID_CAP
    hipLaunchKernelGGL(k_hetero_cuts, dim3(num_cut), dim3(kBlock), 0, s, p, plan.tile_base[1], (const uint32_t *)hist,
                       cut_base_dev, cuts, cut_counts_dev);
    GGMS_LAUNCH_CHECK();
  }
  return GGMS_OK;
}

size_t ggms_hetero_edges_workspace_bytes(const size_t *max_edges, uint32_t num_layer, uint32_t num_rel) {
  SplitPlan plan;
  size_t words, bytes;
  if (!max_edges || num_layer < 1 || num_layer > kSplitMaxJobs || num_rel < 1 || num_rel > GGMS_MAX_EDGE_TYPES ||
      !split_plan(max_edges, num_layer, num_rel, plan, words, bytes))
    return 0;
  return bytes;
}

int ggms_hetero_edges(const ggms_id_t *const *row, const ggms_id_t *const *col, const ggms_id_t *const *eid,
                      const uint8_t *const *etype, const size_t *max_edges, uint32_t num_layer, uint32_t num_rel,
                      const uint64_t *counts_dev, const uint32_t *local, size_t num_local, ggms_id_t *const *out_row,
                      ggms_id_t *const *out_col, ggms_id_t *const *out_eid, uint32_t *rel_offsets_dev, void *workspace,
                      size_t workspace_bytes, ggms_stream_t stream) {
  if (num_layer < 1 || num_layer > kSplitMaxJobs) {
    set_error("ggms_hetero_edges: num_layer %u (1 .. %u)", num_layer, kSplitMaxJobs);
    return GGMS_ERR_INVALID;
  }
  if (num_rel < 1 || num_rel > GGMS_MAX_EDGE_TYPES) {
    set_error("ggms_hetero_edges: num_rel %u (1 .. %d)", num_rel, GGMS_MAX_EDGE_TYPES);
    return GGMS_ERR_INVALID;
  }
  GGMS_HETERO_ARG("ggms_hetero_edges", row);
  GGMS_HETERO_ARG("ggms_hetero_edges", col);
  GGMS_HETERO_ARG("ggms_hetero_edges", etype);
  GGMS_HETERO_ARG("ggms_hetero_edges", max_edges);
  GGMS_HETERO_ARG("ggms_hetero_edges", counts_dev);
  GGMS_HETERO_ARG("ggms_hetero_edges", local);
  GGMS_HETERO_ARG("ggms_hetero_edges", out_row);
  GGMS_HETERO_ARG("ggms_hetero_edges", out_col);
  GGMS_HETERO_ARG("ggms_hetero_edges", rel_offsets_dev);
  if ((eid == nullptr) != (out_eid == nullptr)) {
    set_error("ggms_hetero_edges: eid and out_eid are both given or both null");
    return GGMS_ERR_INVALID;
  }
  SplitPlan plan;
  size_t words, bytes;
  if (!split_plan(max_edges, num_layer, num_rel, plan, words, bytes)) {
    set_error("ggms_hetero_edges: a bound in max_edges is out of range (layers below 2^32 - 1024 edges)");
    return GGMS_ERR_INVALID;
  }
  if (!workspace || workspace_bytes < bytes) {
    set_error("ggms_hetero_edges: workspace of %zu bytes, %zu needed (ggms_hetero_edges_workspace_bytes)",
              workspace ? workspace_bytes : (size_t)0, bytes);
    return GGMS_ERR_INVALID;
  }
  EdgeSplit p{};
  for (uint32_t k = 0; k < num_layer; ++k) {
    if (max_edges[k] != 0 && (!row[k] || !col[k] || !etype[k] || !out_row[k] || !out_col[k] ||
                              (eid && (!eid[k] || !out_eid[k])))) {
      set_error("ggms_hetero_edges: row[%u] / col[%u] / eid[%u] / etype[%u] or one of their outputs is null", k, k, k, k);
      return GGMS_ERR_INVALID;
    }
    p.row[k] = row[k];
    p.col[k] = col[k];
    p.eid[k] = eid ? eid[k] : nullptr;
    p.etype[k] = etype[k];
    p.out_row[k] = out_row[k];
    p.out_col[k] = out_col[k];
    p.out_eid[k] = out_eid ? out_eid[k] : nullptr;
    p.max_edges[k] = max_edges[k];
  }
  p.counts = counts_dev;
  p.local = local;
  p.rel_offsets = rel_offsets_dev;
  p.num_local = num_local > 0xffffffffull ? 0xffffffffu : (uint32_t)num_local;
  p.num_rel = num_rel;
  uint32_t *hist = nullptr;
  return split_run(p, plan, words, workspace, to_stream(stream), &hist);
}

} // extern "C"
