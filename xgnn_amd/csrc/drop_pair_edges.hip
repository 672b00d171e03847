// drop_pair_edges.hip -- take a batch's positive pairs (and their mirrors) out of its sampled layers.
//
// There is no reference counterpart; the definition is in include/ggms.h (ggms_drop_pair_edges) and
// tests/link_exclude_ref.py restates it in numpy.  A link-prediction batch samples the neighbourhood of the endpoints of
// its positive edges from the very graph that holds those edges; this filter removes them again, on the device, with
// every size left there.
//
// One memset and four launches per call, whatever num_pairs and the layers' sizes are (all layers share each launch):
//   memset      the pair table and the word the id bound is collected in, one range of 0xff bytes
//   k_drop_build     the pair set: keys (col << 32) | row of the edges to drop -- (src, dst) for FORWARD, (dst, src) for
//                    REVERSE -- in an open-addressing table of at least twice as many slots as keys (linear probing, one
//                    64-bit CAS per probe; a key already there is left alone: repeated pairs).  At the engine's sizes
//                    (a few thousand pairs) the table is a few hundred KB: it stays in the L2s while the layers stream by.
//                    The launch also collects the largest id of any pair (one atomic per wave): a batch numbers its nodes by
//                    first occurrence and enters the seeds first, so an edge can only match if row and col are both at most
//                    that id -- one compare, and nearly every edge of the deep layers passes without a probe.
//   k_drop_snapshot  per tile of 1024 edges: copy row / col into the workspace as they are, count the edges that stay
//   k_drop_prefix    per layer, one workgroup: tile counts -> exclusive prefix; the new edge count, the dropped count
//   k_drop_compact   per tile: read the SNAPSHOT, write the kept edges to row / col at prefix + rank
//
// Why it is safe in place (the scheme: copy out, compact back).  A stable compaction moves tile t's edges to
// [prefix(t), ...), which lies at or before the tile -- on the input of earlier tiles.  Nothing orders the workgroups of
// a launch, so a scheme that reads and writes row / col in one launch lets a late tile overwrite what an early tile has
// not read yet, and a look-back that recomputes a predecessor's count from the scan's input (tile_scan.h) would read
// edges that are already compacted.  Here no launch reads an array that the same launch writes:
//   k_drop_snapshot reads row / col, writes the snapshot and its own tile's count;
//   k_drop_compact  reads the snapshot and the prefixes, writes row / col;
// and the kernel boundaries between them order everything else.  No workgroup ever waits for another one: there is no
// look-back, no ticket and no spin in this file.  The price is one more pass over the layers (algorithmic bytes: 32 per
// edge -- 8 read + 8 written, twice -- where an in-place pass would move 16).  A tile in front of the layer's first dropped
// edge is already where it belongs and is not rewritten.
// The predicate is evaluated twice (count, compact) rather than stashed: it is one compare for nearly every edge, and
// both evaluations see the same bytes (the snapshot is a copy), so the two passes agree.
//
// Loads and stores: a thread owns 4 consecutive edges of its tile.  Where row / col are 16-byte aligned the snapshot pass
// loads and stores them as one 16-byte vector each (the snapshot itself is always aligned), and the compact pass loads the
// snapshot that way; the compacted stores start wherever the prefix says and are 4-byte stores, consecutive across the
// lanes.  The last, partial vector of a layer is handled element by element.
#include "ggms_internal.h"
#include "labor_hash.h"

namespace ggms {

constexpr uint32_t kDropMaxLayers = 16;
constexpr uint32_t kDropPerThread = kTile / kBlock; // 4 consecutive edges: one 16-byte vector of row, one of col
constexpr unsigned long long kDropFree = ~0ull;     // a free slot; no key looks like it (a pair holding kEmptyKey is skipped)
constexpr uint32_t kDropMinSlots = 64;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
static_assert(kDropPerThread == 4, "a thread's edges are one 16-byte vector");

// what the first bytes of the workspace hold: cleared (0xff) together with the table that follows
struct DropCtl {
  uint32_t inv_max_id; // ~(largest id of any pair), collected with atomicMin: 0xffffffff = no pair yet (largest id 0)
  uint32_t pad[3];
};

// all layers of a call, by value in the kernel arguments (the layer index is uniform per workgroup: scalar loads)
struct DropJobs {
  uint32_t *row[kDropMaxLayers], *col[kDropMaxLayers];
  uint32_t *srow[kDropMaxLayers], *scol[kDropMaxLayers]; // the snapshot
  uint32_t *tile[kDropMaxLayers];                          // kept edges per tile, then their exclusive prefix (+ total)
  uint64_t max_edges[kDropMaxLayers];
  uint32_t tile_base[kDropMaxLayers + 1]; // first tile of layer k in the launch's flat tile numbering
  uint32_t num_layer;
  uint32_t vec; // bit k: row[k] and col[k] are 16-byte aligned
  __device__ __forceinline__ uint32_t layer_of(uint32_t flat) const {
    uint32_t k = 0;
#pragma unroll 1
    for (uint32_t j = 1; j < num_layer; ++j) k = flat >= tile_base[j] ? j : k;
    return k;
  }
};

struct DropSet {
  const unsigned long long *table;
  uint32_t mask;   // slots - 1
  uint32_t max_id; // the prefilter's bound
  __device__ __forceinline__ static uint32_t slot_of(unsigned long long key, uint32_t mask) {
    return fmix32((uint32_t)(key >> 32) * 0x9e3779b1u ^ (uint32_t)key) & mask;
  }
  __device__ __forceinline__ bool drops(uint32_t row, uint32_t col) const {
    if ((row > col ? row : col) > max_id) return false; // (an edge holding kEmptyKey never gets past this)
    const unsigned long long key = ((unsigned long long)col << 32) | row;
    uint32_t s = slot_of(key, mask);
    for (uint32_t step = 0; step <= mask; ++step) { // at most half of the slots are taken: a free one ends the walk
      const unsigned long long k = table[s];
      if (k == key) return true;
      if (k == kDropFree) return false;
      s = (s + 1u) & mask;
    }
    return false;
  }
};

__device__ __forceinline__ uint32_t wave_reduce_max(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t y = __shfl_xor(x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}

__global__ __launch_bounds__(kBlock) void k_drop_build(const uint32_t *__restrict__ pair_src,
                                                       const uint32_t *__restrict__ pair_dst, uint64_t num_pairs,
                                                       uint32_t which, DropCtl *ctl, unsigned long long *table,
                                                       uint32_t mask) {
  uint32_t top = 0;
  bool any = false;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < num_pairs; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t s = pair_src[i], d = pair_dst[i];
    if (s == kEmptyKey || d == kEmptyKey) continue; // matches nothing
    any = true;
    top = s > top ? s : top;
    top = d > top ? d : top;
#pragma unroll
    for (uint32_t bit = GGMS_DROP_FORWARD; bit <= GGMS_DROP_REVERSE; bit <<= 1) {
      if (!(which & bit)) continue;
      const unsigned long long key = bit == GGMS_DROP_FORWARD ? ((unsigned long long)s << 32) | d
                                                              : ((unsigned long long)d << 32) | s;
      uint32_t p = DropSet::slot_of(key, mask);
      for (uint32_t step = 0; step <= mask; ++step) {
        const unsigned long long old = atomicCAS(table + p, kDropFree, key);
        if (old == kDropFree || old == key) break;
        p = (p + 1u) & mask;
      }
    }
  }
  const uint64_t some = __ballot(any);
  top = wave_reduce_max(top);
  if (some != 0ull && lane_id() == 0) atomicMin(&ctl->inv_max_id, ~top);
}

// a thread's 4 edges of tile t: v[k] = p[base + k] for base + k < n (0 beyond); one 16-byte load where it may be
__device__ __forceinline__ void drop_load4(const uint32_t *__restrict__ p, uint64_t base, uint64_t n, bool vec,
                                           uint32_t (&v)[kDropPerThread]) {
  if (vec && base + kDropPerThread <= n) {
    const u32x4 x = *reinterpret_cast<const u32x4 *>(p + base);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kDropPerThread; ++k) v[k] = base + k < n ? p[base + k] : 0u;
  }
}
__device__ __forceinline__ void drop_store4(uint32_t *__restrict__ p, uint64_t base, uint64_t n,
                                            const uint32_t (&v)[kDropPerThread]) {
  if (base + kDropPerThread <= n) { // (the snapshot is 16-byte aligned whatever row / col are)
    u32x4 x;
    x.x = v[0], x.y = v[1], x.z = v[2], x.w = v[3];
    *reinterpret_cast<u32x4 *>(p + base) = x;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kDropPerThread; ++k)
      if (base + k < n) p[base + k] = v[k];
  }
}

__device__ __forceinline__ uint64_t drop_layer_edges(const uint64_t *counts, const DropJobs &jobs, uint32_t k) {
  const uint64_t n = counts[GGMS_COUNT_EDGES(k)];
  return n < jobs.max_edges[k] ? n : jobs.max_edges[k]; // (a count beyond the bound is a caller error: nothing is read there)
}

__global__ __launch_bounds__(kBlock) void k_drop_snapshot(DropJobs jobs, const uint64_t *counts, const DropCtl *ctl,
                                                          const unsigned long long *table, uint32_t mask) {
  __shared__ uint32_t smem[kBlock / kWave];
  const DropSet set{table, mask, ~ctl->inv_max_id};
  const uint32_t total_tiles = jobs.tile_base[jobs.num_layer];
  for (uint32_t flat = blockIdx.x; flat < total_tiles; flat += gridDim.x) {
    const uint32_t k = jobs.layer_of(flat);
    const uint64_t t = flat - jobs.tile_base[k];
    const uint64_t n = drop_layer_edges(counts, jobs, k);
    if (t * kTile >= n) continue; // uniform: the layer is shorter than its bound
    const uint64_t base = t * kTile + (uint64_t)threadIdx.x * kDropPerThread;
    const bool vec = (jobs.vec >> k) & 1u;
    uint32_t r[kDropPerThread], c[kDropPerThread];
    drop_load4(jobs.row[k], base, n, vec, r);
    drop_load4(jobs.col[k], base, n, vec, c);
    drop_store4(jobs.srow[k], base, n, r);
    drop_store4(jobs.scol[k], base, n, c);
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t j = 0; j < kDropPerThread; ++j) kept += (base + j < n && !set.drops(r[j], c[j])) ? 1u : 0u;
    kept = wave_reduce_sum(kept);
    if (lane_id() == 0) smem[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) jobs.tile[k][t] = smem[0] + smem[1] + smem[2] + smem[3];
    __syncthreads(); // smem is rewritten by the next tile
  }
}

// one workgroup per layer: tile counts -> exclusive prefix in place, tile[nt] = total.  n_old[k] keeps the layer's edge
// count for the compact pass, which runs after the counts word has been replaced.
__global__ __launch_bounds__(kBlock) void k_drop_prefix(DropJobs jobs, uint64_t *counts, uint64_t *n_old,
                                                        uint64_t *num_dropped) {
  __shared__ uint32_t smem[kBlock / kWave];
  const uint32_t k = blockIdx.x;
  const uint64_t n = drop_layer_edges(counts, jobs, k);
  const uint64_t nt = (n + kTile - 1) / kTile;
  uint32_t *const tile = jobs.tile[k];
  uint32_t running = 0;
  for (uint64_t t0 = 0; t0 < nt; t0 += kBlock) {
    const uint64_t t = t0 + threadIdx.x;
    const uint32_t v = t < nt ? tile[t] : 0u;
    uint32_t total;
    const uint32_t excl = block_exclusive_scan(v, smem, total);
    if (t < nt) tile[t] = running + excl;
    running += total;
  }
  if (threadIdx.x == 0) {
    tile[nt] = running;
    n_old[k] = n;
    counts[GGMS_COUNT_EDGES(k)] = (uint64_t)running;
    if (num_dropped) num_dropped[k] += n - (uint64_t)running;
  }
}

__global__ __launch_bounds__(kBlock) void k_drop_compact(DropJobs jobs, const uint64_t *n_old, const DropCtl *ctl,
                                                         const unsigned long long *table, uint32_t mask) {
  __shared__ uint32_t smem[kBlock / kWave];
  const DropSet set{table, mask, ~ctl->inv_max_id};
  const uint32_t total_tiles = jobs.tile_base[jobs.num_layer];
  for (uint32_t flat = blockIdx.x; flat < total_tiles; flat += gridDim.x) {
    const uint32_t k = jobs.layer_of(flat);
    const uint64_t t = flat - jobs.tile_base[k];
    const uint64_t n = n_old[k];
    if (t * kTile >= n) continue; // uniform
    const uint32_t prefix = jobs.tile[k][t], next = jobs.tile[k][t + 1];
    const uint64_t in_tile = n - t * kTile < kTile ? n - t * kTile : kTile;
    // nothing dropped in front of the tile or inside it: its edges are where they belong (uniform)
    if ((uint64_t)prefix == t * kTile && (uint64_t)(next - prefix) == in_tile) continue;
    const uint64_t base = t * kTile + (uint64_t)threadIdx.x * kDropPerThread;
    uint32_t r[kDropPerThread], c[kDropPerThread];
    drop_load4(jobs.srow[k], base, n, true, r);
    drop_load4(jobs.scol[k], base, n, true, c);
    bool keep[kDropPerThread];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kDropPerThread; ++j) {
      keep[j] = base + j < n && !set.drops(r[j], c[j]);
      mine += keep[j] ? 1u : 0u;
    }
    uint32_t total;
    uint64_t out = (uint64_t)prefix + block_exclusive_scan(mine, smem, total);
    uint32_t *__restrict__ const row = jobs.row[k];
    uint32_t *__restrict__ const col = jobs.col[k];
#pragma unroll
    for (uint32_t j = 0; j < kDropPerThread; ++j) {
      if (keep[j]) {
        row[out] = r[j];
        col[out] = c[j];
        ++out;
      }
    }
  }
}

// ---- the workspace: [ctl | table] (one memset), n_old, per layer {tile words, snapshot of row, snapshot of col} ----
struct DropLayout {
  size_t table, n_old, tile[kDropMaxLayers], srow[kDropMaxLayers], scol[kDropMaxLayers], bytes;
  uint32_t slots;
};
inline size_t drop_up16(size_t x) { return (x + 15) & ~(size_t)15; }
static bool drop_layout(size_t num_pairs, const size_t *max_edges, uint32_t num_layer, DropLayout &lay) {
  // both directions of every pair, at most half of the slots taken
  size_t slots = kDropMinSlots;
  while (slots < 4 * num_pairs) slots <<= 1;
  if (slots > ((size_t)1 << 31)) return false;
  lay.slots = (uint32_t)slots;
  size_t at = 0;
  lay.table = at += drop_up16(sizeof(DropCtl));
  lay.n_old = at += slots * sizeof(unsigned long long);
  at += drop_up16(kDropMaxLayers * sizeof(uint64_t));
  for (uint32_t k = 0; k < num_layer; ++k) {
    if (max_edges[k] > 0xffffffffull - kTile) return false; // prefixes and tile numbers are 32-bit
    lay.tile[k] = at;
    at += drop_up16((num_tiles_for(max_edges[k]) + 1) * sizeof(uint32_t));
    lay.srow[k] = at;
    at += drop_up16(max_edges[k] * sizeof(uint32_t));
    lay.scol[k] = at;
    at += drop_up16(max_edges[k] * sizeof(uint32_t));
  }
  lay.bytes = at + 16; // the caller's pointer is aligned to 16 bytes here
  return true;
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_drop_pair_edges_workspace_bytes(size_t num_pairs, const size_t *max_edges, uint32_t num_layer) {
  DropLayout lay;
  if (!max_edges || num_layer < 1 || num_layer > kDropMaxLayers || !drop_layout(num_pairs, max_edges, num_layer, lay))
    return 0;
  return lay.bytes;
}

int ggms_drop_pair_edges(const ggms_id_t *pair_src, const ggms_id_t *pair_dst, size_t num_pairs, uint32_t which,
                         ggms_id_t *const *row, ggms_id_t *const *col, const size_t *max_edges, uint32_t num_layer,
                         uint64_t *counts_dev, uint64_t *num_dropped_dev, void *workspace, size_t workspace_bytes,
                         ggms_stream_t stream) {
  if (which > (GGMS_DROP_FORWARD | GGMS_DROP_REVERSE)) {
    set_error("ggms_drop_pair_edges: which %u (GGMS_DROP_FORWARD = 1, GGMS_DROP_REVERSE = 2, or both)", which);
    return GGMS_ERR_INVALID;
  }
  if (num_layer < 1 || num_layer > kDropMaxLayers) {
    set_error("ggms_drop_pair_edges: num_layer %u (1 .. %u)", num_layer, kDropMaxLayers);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(row && col && max_edges && counts_dev);
  if (which == 0 || num_pairs == 0) return GGMS_OK; // nothing can match
  GGMS_CHECK_ARG(pair_src && pair_dst);
  DropLayout lay;
  if (!drop_layout(num_pairs, max_edges, num_layer, lay)) {
    set_error("ggms_drop_pair_edges: num_pairs %zu or a layer bound is out of range (layers of at most 2^32 - 1025 edges)",
              num_pairs);
    return GGMS_ERR_INVALID;
  }
  if (!workspace || workspace_bytes < lay.bytes) {
    set_error("ggms_drop_pair_edges: workspace of %zu bytes, %zu needed (ggms_drop_pair_edges_workspace_bytes)",
              workspace ? workspace_bytes : (size_t)0, lay.bytes);
    return GGMS_ERR_INVALID;
  }
  char *const ws = (char *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  DropJobs jobs{};
  jobs.num_layer = num_layer;
  uint64_t tiles = 0;
  for (uint32_t k = 0; k < num_layer; ++k) {
    if (max_edges[k] != 0 && (!row[k] || !col[k])) {
      set_error("ggms_drop_pair_edges: row[%u] / col[%u] is null", k, k);
      return GGMS_ERR_INVALID;
    }
    jobs.row[k] = row[k];
    jobs.col[k] = col[k];
    jobs.srow[k] = (uint32_t *)(ws + lay.srow[k]);
    jobs.scol[k] = (uint32_t *)(ws + lay.scol[k]);
    jobs.tile[k] = (uint32_t *)(ws + lay.tile[k]);
    jobs.max_edges[k] = max_edges[k];
    jobs.tile_base[k] = (uint32_t)tiles;
    tiles += num_tiles_for(max_edges[k]);
    if ((((uintptr_t)row[k] | (uintptr_t)col[k]) & 15u) == 0) jobs.vec |= 1u << k;
  }
  if (tiles > 0xffffffffull) {
    set_error("ggms_drop_pair_edges: %llu tiles over all layers (at most 2^32 - 1)", (unsigned long long)tiles);
    return GGMS_ERR_INVALID;
  }
  jobs.tile_base[num_layer] = (uint32_t)tiles;
  hipStream_t s = to_stream(stream);
  DropCtl *const ctl = (DropCtl *)ws;
  unsigned long long *const table = (unsigned long long *)(ws + lay.table);
  uint64_t *const n_old = (uint64_t *)(ws + lay.n_old);
  const uint32_t mask = lay.slots - 1u;
  GGMS_HIP(hipMemsetAsync(ws, 0xff, lay.n_old, s)); // ctl + table
  hipLaunchKernelGGL(k_drop_build, dim3(grid_for(num_pairs, kBlock)), dim3(kBlock), 0, s, pair_src, pair_dst,
                     (uint64_t)num_pairs, which, ctl, table, mask);
  const int grid = grid_for((size_t)tiles, 1);
  hipLaunchKernelGGL(k_drop_snapshot, dim3(grid), dim3(kBlock), 0, s, jobs, (const uint64_t *)counts_dev,
                     (const DropCtl *)ctl, (const unsigned long long *)table, mask);
  hipLaunchKernelGGL(k_drop_prefix, dim3(num_layer), dim3(kBlock), 0, s, jobs, counts_dev, n_old, num_dropped_dev);
  hipLaunchKernelGGL(k_drop_compact, dim3(grid), dim3(kBlock), 0, s, jobs, (const uint64_t *)n_old, (const DropCtl *)ctl,
                     (const unsigned long long *)table, mask);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
