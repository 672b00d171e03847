// extract.hip -- feature row gather: GPUExtract and the cache-combine family.
//
// Reference kernels: gpu_extract (cuda/cuda_extraction.cu:31-49), combine_miss_data,
// extract_miss_data, combine_cache_data, combine_cache_data_for_partition
// (cuda/cuda_cache_manager_device.cu:209-299).  All of them are
//     out[dst(i), :] = SRC(src(i))[ : ]
// and differ only in how a source row is located.  One kernel template does all
// of them; the row locator is a functor evaluated once per row.
//
// MI355X mapping (HBM-bound, no reuse, rows of 8 B .. a few KiB):
//   * one wave owns 64 consecutive output rows; each lane resolves ONE row
//     (index load, optional slot -> shard translation) and keeps its source
//     pointer in registers;
//   * the tile is then swept as a flat array of 16-byte chunks: chunk c of the
//     tile belongs to row c / chunks_per_row; the owning lane's pointer comes
//     through ds_bpermute (no LDS memory), so every wave-instruction moves a full
//     1 KiB even when a row is 400 B (25 chunks), and the store side of an
//     identity-destination gather is one contiguous 1 KiB segment;
//   * U = 16 independent chunk loads per lane are issued before the first store.
// Algorithmic bytes per row: 4 (index) + 2 * row_bytes.
#include <cstdlib>

#include <hip/hip_ext.h>

#include "ggms_device.h"
#include "row_chunks.h"

namespace ggms {

// which tier served a row (0 = not counted); counters[tier - 1] in ggms_extract_tiered
constexpr uint32_t kTierHost = 1, kTierRemote = 2, kTierLocal = 3, kTierReplica = 4;

// ---- row locators -----------------------------------------------------------
// src(i) = index ? index[i] : i ;  row pointer = base + src(i) * row_bytes
struct PlainRows {
  const char *base;
  const uint32_t *index;
  uint64_t row_bytes;
  uint32_t mask = 0xffffffffu; // gpu_mock_extract (cuda_extraction.cu:51-70): rows of a 2^k-row mock table, index & mask
  static constexpr bool kTiers = false;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    tier = 0;
    const uint64_t s = index ? (uint64_t)(index[i] & mask) : i;
    return base + s * row_bytes;
  }
};

// DeviceDistFeature::Get (cuda/dist_graph.h:191-205): slot -> shard slot % P, row slot / P
// The shard pointers travel by value (PtrSet: a select chain on registers, not a load from a device pointer table) and
// the split is a multiply-high by the launch-constant shard count (Divisor) -- both sit on every row's
// index -> slot -> pointer chain, ahead of the row's first byte.
typedef PtrSet<const char, kMaxParts> PartPtrs;
struct PartitionRows {
  PartPtrs parts;
  const uint32_t *index;
  uint64_t row_bytes;
  Divisor num_part;
  static constexpr bool kTiers = false;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    tier = 0;
    uint32_t part, real;
    num_part.divmod(index[i], real, part);
    return parts.pick(part) + (uint64_t)real * row_bytes;
  }
};

// fused hit/miss: table[node] == kEmptyKey -> host tier row `node`, else cache slot
struct CachedRows {
  PartPtrs parts;
  const uint32_t *nodes;
  const uint32_t *table;
  const char *host;
  uint64_t row_bytes;
  Divisor num_part; // d = 1: one cache array parts[0]
  static constexpr bool kTiers = false;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    const uint32_t node = nodes[i];
    const uint32_t slot = table[node];
    tier = (slot == kEmptyKey) ? kTierHost : 0u;
    if (slot == kEmptyKey) return host + (uint64_t)node * row_bytes;
    uint32_t part, real;
    num_part.divmod(slot, real, part);
    return parts.pick(part) + (uint64_t)real * row_bytes;
  }
};

// dynamic_cache (arch4): a row the previous batch also had is read from that batch's feature buffer (HBM), every other
// row from the device-mapped host table.  The stamp word of a node is (seq << 32) | slot of its last batch; prev_seq = 0:
// no previous batch (seq 1, or a reset table), nothing hits.
struct DynamicRows {
  const uint32_t *nodes;
  const unsigned long long *stamps;
  const char *prev;
  const char *host;
  uint64_t row_bytes;
  uint32_t prev_seq;
  static constexpr bool kTiers = false;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    const uint32_t node = nodes[i];
    const unsigned long long e = stamps[node];
    const bool hit = prev_seq != 0 && (uint32_t)(e >> 32) == prev_seq;
    tier = hit ? 0u : kTierHost;
    return hit ? prev + (uint64_t)(uint32_t)e * row_bytes : host + (uint64_t)node * row_bytes;
  }
};

// after batch seq's gather: its rows are in ITS feature buffer at their positions
__global__ __launch_bounds__(kBlock) void k_dynamic_publish(unsigned long long *__restrict__ stamps,
                                                            const uint32_t *__restrict__ nodes, Count n_arg,
                                                            uint32_t seq) {
  const uint64_t n = n_arg.get();
  const unsigned long long hi = (unsigned long long)seq << 32;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    stamps[nodes[i]] = hi | (uint32_t)i;
}

// All tiers of the store in one locator (ggms_extract_tiered): slot = table ? table[node] : node;
//   kEmptyKey            -> host tier, row `node` of the device-mapped host table      (GPUExtractMissData)
//   slot <  num_replica  -> this GPU's replica of the hottest rows, row `slot`         (hot-row replication)
//   else s = slot - num_replica -> shard s % P at row s / P: local HBM or a peer's over xGMI
//                                                                      (combine_cache_data_for_partition)
// and says which tier served the row, for the per-tier counters (count_local_cache, :171-207).
struct TieredRows {
  PartPtrs parts;
  const uint32_t *nodes;
  const uint32_t *table;
  const char *host;
  const char *replica;
  uint64_t row_bytes;
  uint32_t num_replica;
  Divisor num_part; // d >= 1
  uint32_t my_part;
  uint32_t host_mask; // host tier row = node & host_mask (mock table of SAMGRAPH_EMPTY_FEAT; else all ones)
  static constexpr bool kTiers = true;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    const uint32_t node = nodes[i];
    const uint32_t slot = table ? table[node] : node;
    if (slot == kEmptyKey) {
      tier = kTierHost;
      return host + (uint64_t)(node & host_mask) * row_bytes;
    }
    if (slot < num_replica) {
      tier = kTierReplica;
      return replica + (uint64_t)slot * row_bytes;
    }
    uint32_t part, real;
    num_part.divmod(slot - num_replica, real, part);
    tier = part == my_part ? kTierLocal : kTierRemote;
    return parts.pick(part) + (uint64_t)real * row_bytes;
  }
};

// cache_ratio 1.0, rows kept in NODE order (slot = node id): no table, no miss tier.  The layout of a full cache is
// not observable through the reference's interface (the batch's rows come out in input-node order either way), and
// it removes one dependent random 4-byte read (a 64-byte sector of HBM traffic) per gathered row.
struct IdentRows {
  PartPtrs parts;
  const uint32_t *nodes;
  uint64_t row_bytes;
  Divisor num_part; // d = 1: one array parts[0]
  static constexpr bool kTiers = false;
  __device__ __forceinline__ const char *row(uint64_t i, uint32_t &tier) const {
    tier = 0;
    const uint32_t node = nodes[i];
    if (num_part.d == 1) return parts.p[0] + (uint64_t)node * row_bytes; // uniform
    uint32_t part, real;
    num_part.divmod(node, real, part);
    return parts.pick(part) + (uint64_t)real * row_bytes;
  }
};

// host side: the caller's HOST array of shard base pointers -> kernel argument
static inline bool part_ptrs(const void *const *parts, uint32_t num_part, PartPtrs &out) {
  out = PartPtrs{};
  const uint32_t n = num_part ? num_part : 1;
  if (!parts || n > kMaxParts) {
    set_error("extract: num_part %u (at most %u shards; `parts` is a HOST array of num_part device pointers)", num_part, kMaxParts);
    return false;
  }
  if (!host_readable_table(parts, "`parts`")) return false;
  for (uint32_t p = 0; p < n; ++p) out.p[p] = (const char *)parts[p];
  return true;
}

// U = independent chunk loads in flight per lane (16, or 8 for rows of fewer than 8 chunks)
// Loads and stores are non-temporal: a batch's rows are read once and the gathered batch is a > 100-MB stream that
// nothing re-reads from cache (measured + 3..5 % on MI355X each, profiles/r01-r02).
template <typename Chunk, typename Rows, bool IDENT_DST, int U>
__global__ __launch_bounds__(kBlock) void k_gather_rows(char *__restrict__ out, Rows rows,
                                                        const uint32_t *__restrict__ dst_index, Count n_arg,
                                                        uint32_t rc, uint32_t magic, uint64_t *miss_count) {
  using SV = typename Chunk::Src;
  using DV = typename Chunk::Dst;
  constexpr uint32_t SB = Chunk::kSrcBytes, DB = Chunk::kDstBytes;
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const uint64_t num_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t row_bytes = (uint64_t)rc * DB; // of an OUTPUT row (the locator knows the source's)
  const uint64_t num_tiles = (n + kWave - 1) / kWave;

  // resolve one row per lane for tile `t`: source pointer (+ destination pointer; + the row's scale and bias, the
  // 8-byte trailer behind a Q8ROW row's codes)
  [[maybe_unused]] const uint64_t trailer = q8row_trailer_offset((uint64_t)rc * SB);
  auto resolve = [&](uint64_t t, uint64_t &sp, uint64_t &dp, uint32_t &miss, [[maybe_unused]] u32x2_t &sb) {
    const uint64_t my_row = t * kWave + lane;
    sp = 0; dp = 0; miss = 0;
    if constexpr (Chunk::kScaled) sb = u32x2_t{0u, 0u};
    if (t < num_tiles && my_row < n) {
      sp = (uint64_t)rows.row(my_row, miss);
      if constexpr (Chunk::kScaled) sb = load_chunk<u32x2_t, true>(sp + trailer);
      if constexpr (!IDENT_DST) dp = (uint64_t)(out + (uint64_t)dst_index[my_row] * row_bytes);
    }
  };

  uint64_t sp, dp;
  [[maybe_unused]] u32x2_t sb; // {scale, bias} of my row, as bits (ScaledChunk only)
  uint32_t miss; // tier of my row (kTierHost = a cache miss)
  // rows per tier: counted per wave in registers, combined per workgroup in LDS and added to the caller's counters
  // ONCE per workgroup at the end.  (An atomic per wave and tile -- 46 K tiles x 3 tiers on one line -- is served one
  // at a time at the memory side, 12 ns each: 1.6 ms of counter updates behind a 0.5-ms gather, tools/micro_ticket.hip.)
  uint32_t tier_acc[kTierReplica + 1] = {};
  __shared__ unsigned int s_tier[kTierReplica + 1];
  if (miss_count && threadIdx.x <= kTierReplica) s_tier[threadIdx.x] = 0u;
  resolve(wave, sp, dp, miss, sb);
  for (uint64_t tile = wave; tile < num_tiles; tile += num_waves) {
    // software pipeline: the next tile's index -> table -> pointer chain is in flight while this
    // tile's rows stream
    uint64_t sp_n, dp_n;
    [[maybe_unused]] u32x2_t sb_n;
    uint32_t miss_n;
    resolve(tile + num_waves, sp_n, dp_n, miss_n, sb_n);

    if (miss_count) {
      tier_acc[0] += (uint32_t)__popcll(__ballot(miss == kTierHost));
      if constexpr (Rows::kTiers) {
#pragma unroll
        for (uint32_t k = kTierRemote; k <= kTierReplica; ++k) tier_acc[k - 1] += (uint32_t)__popcll(__ballot(miss == k));
      }
    }
    const uint64_t row0 = tile * kWave;
    const uint32_t rows_here = (n - row0 < (uint64_t)kWave) ? (uint32_t)(n - row0) : (uint32_t)kWave;
    const uint32_t total = rows_here * rc; // chunks in this tile
    const uint64_t out_tile = (uint64_t)(out + row0 * row_bytes);
    for (uint32_t c0 = 0; c0 < total; c0 += kWave * U) {
      SV tmp[U];
      uint32_t cc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t c = c0 + u * kWave + lane;
        cc[u] = c < total ? c : total - 1; // clamp: the load is unconditional, the store is not
        // cc / rc, exact for cc * rc < 2^32; rc == 1 has magic = 0 and takes cc itself
        const uint32_t r = __umulhi(cc[u], magic) + (rc == 1 ? cc[u] : 0u);
        const uint32_t col = cc[u] - r * rc;
        const uint64_t p = shfl_u64(sp, (int)r);
        tmp[u] = load_chunk<SV, true>(p + (uint64_t)col * SB);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t c = c0 + u * kWave + lane;
        uint64_t q;
        if constexpr (IDENT_DST) {
          q = out_tile + (uint64_t)cc[u] * DB;
        } else {
          const uint32_t r = __umulhi(cc[u], magic) + (rc == 1 ? cc[u] : 0u);
          q = shfl_u64(dp, (int)r) + (uint64_t)(cc[u] - r * rc) * DB;
        }
        if constexpr (Chunk::kScaled) {
          // the chunk's row once more (the load loop's `r` is not kept: one multiply-high per chunk instead of U
          // registers held across the loads), for the owner lane's scale and bias
          const uint32_t r = __umulhi(cc[u], magic) + (rc == 1 ? cc[u] : 0u);
          const uint32_t scale = __shfl(sb.x, (int)r, 64), bias = __shfl(sb.y, (int)r, 64);
          if (c < total) store_chunk<DV, true>(q, Chunk::convert(tmp[u], scale, bias));
        } else {
          if (c < total) store_chunk<DV, true>(q, Chunk::convert(tmp[u]));
        }
      }
    }
    sp = sp_n; dp = dp_n; miss = miss_n;
    if constexpr (Chunk::kScaled) sb = sb_n;
  }
  if (miss_count) { // uniform: every wave of the workgroup gets here
    __syncthreads(); // s_tier is zeroed
    if (lane == 0) {
#pragma unroll
      for (uint32_t k = 0; k < (Rows::kTiers ? kTierReplica : 1u); ++k)
        if (tier_acc[k]) atomicAdd(&s_tier[k], tier_acc[k]);
    }
    __syncthreads();
    if (threadIdx.x < (Rows::kTiers ? kTierReplica : 1u) && s_tier[threadIdx.x])
      atomicAdd((unsigned long long *)miss_count + threadIdx.x, (unsigned long long)s_tier[threadIdx.x]);
  }
}

// Rows of 8192 chunks or more (>= 128 KiB at 16-byte chunks; the tile sweep's chunk -> row division is exact only
// below that): every row is a long contiguous stream by itself, so one workgroup copies one row.
template <typename Chunk, typename Rows>
__global__ __launch_bounds__(kBlock) void k_gather_long_rows(char *__restrict__ out, Rows rows,
                                                             const uint32_t *__restrict__ dst_index, Count n_arg,
                                                             uint64_t rc, uint64_t *miss_count) {
  using SV = typename Chunk::Src;
  using DV = typename Chunk::Dst;
  constexpr uint32_t SB = Chunk::kSrcBytes, DB = Chunk::kDstBytes;
  const uint64_t n = n_arg.get();
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint32_t tier = 0;
    const uint64_t sp = (uint64_t)rows.row(i, tier);
    const uint64_t dp = (uint64_t)(out + (dst_index ? (uint64_t)dst_index[i] : i) * rc * DB);
    if (miss_count && threadIdx.x == 0) {
      if (tier == kTierHost) atomicAdd((unsigned long long *)miss_count, 1ull);
      else if (Rows::kTiers && tier >= kTierRemote) atomicAdd((unsigned long long *)miss_count + (tier - 1), 1ull);
    }
    if constexpr (Chunk::kScaled) { // the row's scale and bias: one load, the same for every lane
      const u32x2_t sb = load_chunk<u32x2_t, true>(sp + q8row_trailer_offset(rc * SB));
      for (uint64_t c = threadIdx.x; c < rc; c += kBlock)
        store_chunk<DV, true>(dp + c * DB, Chunk::convert(load_chunk<SV, true>(sp + c * SB), sb.x, sb.y));
    } else {
      for (uint64_t c = threadIdx.x; c < rc; c += kBlock)
        store_chunk<DV, true>(dp + c * DB, Chunk::convert(load_chunk<SV, true>(sp + c * SB)));
    }
  }
}

// identity copy of `n` rows (src_index == dst_index == NULL): plain coalesced stream, count on the device
__global__ __launch_bounds__(kBlock) void k_copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src,
                                                       Count n_arg, uint32_t words_per_row) {
  const uint64_t n = n_arg.get() * words_per_row;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) dst[i] = src[i];
}

} // namespace ggms

// ---- launch timer (include/ggms.h): a pair of events that ride on the next gather's own dispatch packet ------------
struct ggms_launch_timer {
  hipEvent_t start = nullptr, stop = nullptr;
  bool launched = false; // the pair has been attached to a launch (its timestamps mean something)
};

namespace ggms {

static thread_local ggms_launch_timer *tl_armed_timer = nullptr;

bool take_armed_timer(hipEvent_t *start, hipEvent_t *stop) {
  ggms_launch_timer *t = tl_armed_timer;
  if (!t) return false;
  tl_armed_timer = nullptr;
  t->launched = true;
  *start = t->start;
  *stop = t->stop;
  return true;
}

// GGMS_EXTRACT_BLOCKS (default 256): the most workgroups any row gather is launched with (launch_chunks has the story)
int gather_max_blocks() {
  static const int max_blocks = [] { const char *e = getenv("GGMS_EXTRACT_BLOCKS"); int v = e ? atoi(e) : 256; return v > 0 ? v : 256; }();
  return max_blocks;
}

// One row-gather launch: with a timer armed on this thread the kernel goes out through hipExtLaunchKernel carrying
// the timer's events (start = the dispatch's own begin timestamp, stop = its completion signal) -- no marker packet
// before or behind it; otherwise the plain launch.
template <typename F, typename... Args>
static inline void launch_rows(F kernel, int grid, hipStream_t stream, Args... args) {
  hipEvent_t start, stop;
  if (take_armed_timer(&start, &stop))
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, start, stop, 0, args...);
  else
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, args...);
}

// Every row gather goes out through here: `rc` chunks per row, moved as Chunk says.  SCATTER false: the caller never
// has a dst_index (no scatter form of the kernel is built for it).
template <typename Chunk, typename Rows, bool SCATTER = true>
static int launch_chunks(char *out, Rows rows, const uint32_t *dst_index, size_t n_max, Count n, uint64_t rc,
                         uint64_t *miss_count, hipStream_t stream) {
  if (n_max == 0) return GGMS_OK;
  if (rc == 0) {
    set_error("extract: empty rows");
    return GGMS_ERR_INVALID;
  }
  if (!SCATTER && dst_index) {
    set_error("extract: this gather has no scatter form");
    return GGMS_ERR_INVALID;
  }
  if (rc >= 8192) {
    launch_rows(k_gather_long_rows<Chunk, Rows>, grid_for(n_max, 1), stream, out, rows, dst_index, n, rc, miss_count);
    GGMS_LAUNCH_CHECK();
    return GGMS_OK;
  }
  const uint32_t magic = rc == 1 ? 0u : (uint32_t)(((1ull << 32) + rc - 1) / rc);
  // one wave per 64 rows, grid-stride.  The grid is capped at ONE 4-wave block per CU (GGMS_EXTRACT_BLOCKS,
  // default 256 -- the one environment variable the library reads: it moves the memory side's share between the
  // gather and the sampler beside it, profiles/r03_ab_gather_grid.txt): with 16 x 16-B loads per lane in flight that
  // already streams at the rate of a full-occupancy launch, and the free wave slots let the next batch's
  // latency-bound sampling kernels run beside the gather on another stream.
  const int max_blocks = gather_max_blocks();
  int grid = grid_for(n_max, kBlock);
  if (grid > max_blocks) grid = max_blocks;
  // 16 independent chunk loads per lane once a row has >= 8 chunks, else 8 (measured: 0.58 -> 0.60 of peak at 400-B
  // rows, 0.65 -> 0.70 at 512-B rows, and the gather holds its rate when the sampler runs beside it)
  const bool deep = rc >= 8;
#define GGMS_LAUNCH(ID)                                                                                              \
  do {                                                                                                               \
    if (deep)                                                                                                        \
      launch_rows(k_gather_rows<Chunk, Rows, ID, 16>, grid, stream, out, rows, dst_index, n, (uint32_t)rc, magic, miss_count); \
    else                                                                                                             \
      launch_rows(k_gather_rows<Chunk, Rows, ID, 8>, grid, stream, out, rows, dst_index, n, (uint32_t)rc, magic, miss_count); \
  } while (0)
  if (dst_index == nullptr) {
    GGMS_LAUNCH(true);
  } else if constexpr (SCATTER) {
    GGMS_LAUNCH(false);
  }
#undef GGMS_LAUNCH
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

template <typename Rows>
static int launch_gather(char *out, Rows rows, const uint32_t *dst_index, size_t n_max, Count n,
                         size_t row_bytes, int cb, uint64_t *miss_count, hipStream_t stream) {
  const uint64_t rc = row_bytes / cb;
  switch (cb) {
    case 16: return launch_chunks<CopyChunk<16>>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    case 8: return launch_chunks<CopyChunk<8>>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    case 4: return launch_chunks<CopyChunk<4>>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    case 2: return launch_chunks<CopyChunk<2>>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    default: return launch_chunks<CopyChunk<1>>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
  }
}

// ---- how a call's rows are moved -------------------------------------------------------------------------------------
// src_dt == dst_dt (any dtype): as bytes, the plain gather.  Otherwise the output is one of F16 / BF16 / F32, the source
// one of those or an FP8 type (decoded, never produced), and the gather converts (ConvertChunk): the same locators,
// sweep and launch path, chunks of `epc` elements.  A Q8ROW source (row-scaled codes, a source only and never moved
// "plain": it has no element size) goes the same way with ScaledChunk; its element is the one-byte code and its rows
// lie ggms_row_bytes apart.
struct RowMove {
  int src_dt, dst_dt;
  size_t dim, src_es, dst_es, src_stride;
  bool converts() const { return src_dt != dst_dt; }
  size_t src_row_bytes() const { return src_stride; } // the distance between two stored rows
};
static bool row_move(int src_dt, int dst_dt, size_t dim, RowMove &m) {
  const bool q8row = src_dt == GGMS_Q8ROW; // its element is the one-byte code
  if ((q8row || dst_dt == GGMS_Q8ROW) && !(q8row && is_float_dtype(dst_dt))) {
    set_error("extract: invalid argument: no conversion from dtype %d to dtype %d (Q8ROW is the source of a "
              "converting gather into F16, BF16 or F32, nothing else)", src_dt, dst_dt);
    return false;
  }
  m = RowMove{src_dt, dst_dt, dim, q8row ? 1 : ggms_dtype_bytes(src_dt), ggms_dtype_bytes(dst_dt), ggms_row_bytes(src_dt, dim)};
  if (m.src_es == 0 || m.dst_es == 0 || dim == 0) {
    set_error("extract: invalid argument: dtype %d -> %d, dim %zu (unknown dtype or empty rows)", src_dt, dst_dt, dim);
    return false;
  }
  if (m.converts() && !(gather_converts_from(src_dt) && is_float_dtype(dst_dt))) {
    set_error("extract: invalid argument: no conversion from dtype %d to dtype %d (a converting gather takes F16, BF16 "
              "and F32 on either side, F8E4M3 and F8E5M2 as the source only)", src_dt, dst_dt);
    return false;
  }
  return true;
}

// A chunk FAMILY: one converting pair in every chunk width it is built in (kMaxEpc: convert_max_epc, row_chunks.h)
template <int SRC_DT, int DST_DT> struct ConvertFamily {
  static constexpr int kSrcDt = SRC_DT, kDstDt = DST_DT;
  static constexpr int kMaxEpc = convert_max_epc(sizeof(typename Elem<SRC_DT>::bits), sizeof(typename Elem<DST_DT>::bits));
  template <int EPC> using Chunk = ConvertChunk<EPC, SRC_DT, DST_DT>;
};
template <int DST_DT> struct ScaledFamily { // Q8ROW -> DST_DT: a one-byte source element
  static constexpr int kSrcDt = GGMS_Q8ROW, kDstDt = DST_DT;
  static constexpr int kMaxEpc = convert_max_epc(1, sizeof(typename Elem<DST_DT>::bits));
  template <int EPC> using Chunk = ScaledChunk<EPC, DST_DT>;
};

// rows of `dim` elements in the family's chunk of `epc` of them (8-element chunks exist where kMaxEpc allows them only)
template <typename Family, bool SCATTER, typename Rows>
static int launch_family(char *out, Rows rows, const uint32_t *dst_index, size_t n_max, Count n, size_t dim, int epc,
                         uint64_t *miss_count, hipStream_t stream) {
  const uint64_t rc = dim / epc;
  if constexpr (Family::kMaxEpc == 8)
    if (epc == 8)
      return launch_chunks<typename Family::template Chunk<8>, Rows, SCATTER>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
  switch (epc) {
    case 4: return launch_chunks<typename Family::template Chunk<4>, Rows, SCATTER>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    case 2: return launch_chunks<typename Family::template Chunk<2>, Rows, SCATTER>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
    case 1: return launch_chunks<typename Family::template Chunk<1>, Rows, SCATTER>(out, rows, dst_index, n_max, n, rc, miss_count, stream);
  }
  set_error("extract: no %d-element chunk for dtype %d -> %d", epc, Family::kSrcDt, Family::kDstDt);
  return GGMS_ERR_INVALID;
}

// src_bits: every source base pointer the locator may use, ORed (shard bases come from hipMalloc /
// hipIpcOpenMemHandle / hipHostMalloc, >= 256-B aligned, and may be left out)
template <bool SCATTER = true, typename Rows>
static int launch_move(char *out, Rows rows, const uint32_t *dst_index, size_t n_max, Count n, const RowMove &m,
                       uintptr_t src_bits, uint64_t *miss_count, hipStream_t stream) {
  if (!m.converts())
    return launch_gather(out, rows, dst_index, n_max, n, m.src_row_bytes(),
                         pick_chunk(m.src_row_bytes(), (uintptr_t)out | src_bits), miss_count, stream);
  const int epc = pick_chunk(m.dim, convert_max_epc(m.src_es, m.dst_es), m.src_es, src_bits, m.dst_es, (uintptr_t)out);
  if (m.src_dt == GGMS_Q8ROW) {
    // rows lie a multiple of 8 bytes apart, so an 8-byte aligned base puts every row's trailer where one 8-byte load
    // reads it (the callers of a Q8ROW gather put their shard bases into src_bits too)
    if (src_bits % 8 != 0) {
      set_error("extract: invalid argument: a Q8ROW source base is not 8-byte aligned (every row ends in an 8-byte "
                "scale / bias trailer, read by one load)");
      return GGMS_ERR_INVALID;
    }
    switch (m.dst_dt) {
      case GGMS_F32: return launch_family<ScaledFamily<GGMS_F32>, SCATTER>(out, rows, dst_index, n_max, n, m.dim, epc, miss_count, stream);
      case GGMS_F16: return launch_family<ScaledFamily<GGMS_F16>, SCATTER>(out, rows, dst_index, n_max, n, m.dim, epc, miss_count, stream);
      case GGMS_BF16: return launch_family<ScaledFamily<GGMS_BF16>, SCATTER>(out, rows, dst_index, n_max, n, m.dim, epc, miss_count, stream);
    }
  }
#define GGMS_PAIR(S, D)                                                                                              \
  if (m.src_dt == S && m.dst_dt == D)                                                                                \
    return launch_family<ConvertFamily<S, D>, SCATTER>(out, rows, dst_index, n_max, n, m.dim, epc, miss_count, stream);
  GGMS_PAIR(GGMS_F16, GGMS_F32)
  GGMS_PAIR(GGMS_BF16, GGMS_F32)
  GGMS_PAIR(GGMS_F32, GGMS_F16)
  GGMS_PAIR(GGMS_F32, GGMS_BF16)
  GGMS_PAIR(GGMS_F16, GGMS_BF16)
  GGMS_PAIR(GGMS_BF16, GGMS_F16)
  GGMS_PAIR(GGMS_F8E4M3, GGMS_F32)
  GGMS_PAIR(GGMS_F8E4M3, GGMS_F16)
  GGMS_PAIR(GGMS_F8E4M3, GGMS_BF16)
  GGMS_PAIR(GGMS_F8E5M2, GGMS_F32)
  GGMS_PAIR(GGMS_F8E5M2, GGMS_F16)
  GGMS_PAIR(GGMS_F8E5M2, GGMS_BF16)
#undef GGMS_PAIR
  set_error("extract: no conversion from dtype %d to dtype %d", m.src_dt, m.dst_dt);
  return GGMS_ERR_INVALID;
}

} // namespace ggms

using namespace ggms;

// The shard bases of a Q8ROW gather, ORed (launch_move checks their alignment; every other gather leaves them out:
// shard bases come from hipMalloc / hipIpcOpenMemHandle / hipHostMalloc, and its chunk choice is unchanged by this)
static inline uintptr_t part_align_bits(const PartPtrs &pp, uint32_t num_part, const RowMove &m) {
  uintptr_t bits = 0;
  if (m.src_dt == GGMS_Q8ROW)
    for (uint32_t p = 0; p < (num_part ? num_part : 1); ++p) bits |= (uintptr_t)pp.p[p];
  return bits;
}

// The bodies behind the entry points that exist in a plain and a converting form (ggms_*_convert): one dtype is the
// plain call, two are the converting one.
static int gather_scatter_rows(void *out, const void *src, const ggms_id_t *src_index, const ggms_id_t *dst_index,
                               size_t num, const uint64_t *num_dev, size_t dim, int src_dtype, int out_dtype,
                               uint32_t src_row_mask, ggms_stream_t stream) {
  RowMove m;
  if (!row_move(src_dtype, out_dtype, dim, m)) return GGMS_ERR_INVALID;
  if (num == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && src);
  PlainRows rows{(const char *)src, src_index, m.src_row_bytes(), src_row_mask};
  return launch_move((char *)out, rows, dst_index, num, count_of(num, num_dev), m, (uintptr_t)src, nullptr,
                     to_stream(stream));
}

static int extract_cached_rows(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                               const ggms_id_t *table, const void *const *parts, uint32_t num_part,
                               const void *host_feat, size_t dim, int src_dtype, int out_dtype, uint64_t *num_miss_dev,
                               ggms_stream_t stream) {
  RowMove m;
  if (!row_move(src_dtype, out_dtype, dim, m)) return GGMS_ERR_INVALID;
  if (num_nodes == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && nodes && parts);
  PartPtrs pp;
  if (!part_ptrs(parts, num_part, pp)) return GGMS_ERR_INVALID;
  const Divisor div = divisor_of(num_part ? num_part : 1);
  const uintptr_t part_bits = part_align_bits(pp, num_part, m);
  if (!table) { // full cache in node order: slot = node id
    IdentRows rows{pp, nodes, m.src_row_bytes(), div};
    if (num_miss_dev) GGMS_HIP(hipMemsetAsync(num_miss_dev, 0, sizeof(uint64_t), to_stream(stream)));
    return launch_move<false>((char *)out, rows, nullptr, num_nodes, count_of(num_nodes, num_nodes_dev), m, part_bits,
                              nullptr, to_stream(stream));
  }
  CachedRows rows{pp, nodes, table, (const char *)host_feat, m.src_row_bytes(), div};
  return launch_move<false>((char *)out, rows, nullptr, num_nodes, count_of(num_nodes, num_nodes_dev), m,
                            (uintptr_t)host_feat | part_bits, num_miss_dev, to_stream(stream));
}

static int extract_tiered_rows(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                               const ggms_feature_tiers_t *tiers, size_t dim, int src_dtype, int out_dtype,
                               uint64_t *tier_rows_dev, ggms_stream_t stream) {
  RowMove m;
  if (!row_move(src_dtype, out_dtype, dim, m)) return GGMS_ERR_INVALID;
  GGMS_CHECK_ARG(tiers);
  if (num_nodes == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && nodes && tiers->parts && tiers->num_part >= 1 && tiers->my_part < tiers->num_part);
  GGMS_CHECK_ARG(tiers->num_replica == 0 || tiers->replica);
  GGMS_CHECK_ARG(tiers->num_replica < (1ull << 32));
  PartPtrs pp;
  if (!part_ptrs(tiers->parts, tiers->num_part, pp)) return GGMS_ERR_INVALID;
  TieredRows rows{pp, nodes, tiers->table, (const char *)tiers->host_feat,
                  (const char *)tiers->replica, m.src_row_bytes(), (uint32_t)tiers->num_replica,
                  divisor_of(tiers->num_part), tiers->my_part, tiers->host_row_mask ? tiers->host_row_mask : 0xffffffffu};
  return launch_move<false>((char *)out, rows, nullptr, num_nodes, count_of(num_nodes, num_nodes_dev), m,
                            (uintptr_t)tiers->host_feat | (uintptr_t)tiers->replica | part_align_bits(pp, tiers->num_part, m),
                            tier_rows_dev, to_stream(stream));
}

extern "C" {

int ggms_extract(void *dst, const void *src, const ggms_id_t *index, size_t num_index, size_t dim, int dtype,
                 ggms_stream_t stream) {
  const size_t es = ggms_dtype_bytes(dtype);
  GGMS_CHECK_ARG(es != 0 && dim != 0);
  if (num_index == 0) return GGMS_OK;
  GGMS_CHECK_ARG(dst && src && index);
  const size_t row_bytes = dim * es;
  const int cb = pick_chunk(row_bytes, (uintptr_t)dst | (uintptr_t)src);
  PlainRows rows{(const char *)src, index, row_bytes};
  return launch_gather((char *)dst, rows, nullptr, num_index, count_of(num_index), row_bytes, cb, nullptr,
                       to_stream(stream));
}

int ggms_gather_scatter(void *out, const void *src, const ggms_id_t *src_index, const ggms_id_t *dst_index,
                        size_t num, const uint64_t *num_dev, size_t dim, int dtype, ggms_stream_t stream) {
  const size_t es = ggms_dtype_bytes(dtype);
  GGMS_CHECK_ARG(es != 0 && dim != 0);
  if (num == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && src);
  const size_t row_bytes = dim * es;
  if (!src_index && !dst_index && row_bytes % 4 == 0 && (((uintptr_t)out | (uintptr_t)src) & 3) == 0) {
    launch_rows(k_copy_words, grid_for(num * (row_bytes / 4), kBlock * 4), to_stream(stream), (uint32_t *)out,
                (const uint32_t *)src, count_of(num, num_dev), (uint32_t)(row_bytes / 4));
    GGMS_LAUNCH_CHECK();
    return GGMS_OK;
  }
  return gather_scatter_rows(out, src, src_index, dst_index, num, num_dev, dim, dtype, dtype, 0xffffffffu, stream);
}

// ggms_gather_scatter with the source row taken as src_index[i] & src_row_mask: gpu_mock_extract
// (cuda_extraction.cu:51-70) and the mock-table forms of the miss extract (cuda_cache_manager_host.cc:47-48)
int ggms_gather_scatter_masked(void *out, const void *src, const ggms_id_t *src_index, const ggms_id_t *dst_index,
                               size_t num, const uint64_t *num_dev, size_t dim, int dtype, uint32_t src_row_mask,
                               ggms_stream_t stream) {
  GGMS_CHECK_ARG(num == 0 || src_index);
  return gather_scatter_rows(out, src, src_index, dst_index, num, num_dev, dim, dtype, dtype, src_row_mask, stream);
}

int ggms_gather_scatter_convert(void *out, const void *src, const ggms_id_t *src_index, const ggms_id_t *dst_index,
                                size_t num, const uint64_t *num_dev, size_t dim, int src_dtype, int out_dtype,
                                uint32_t src_row_mask, ggms_stream_t stream) {
  return gather_scatter_rows(out, src, src_index, dst_index, num, num_dev, dim, src_dtype, out_dtype, src_row_mask, stream);
}

// GPUMockExtract (cuda_extraction.cu:119-160): dst[i, :] = src[index[i] & (2^mock_bits - 1), :]
int ggms_mock_extract(void *dst, const void *src, const ggms_id_t *index, size_t num_index, size_t dim, int dtype,
                      uint32_t mock_bits, ggms_stream_t stream) {
  GGMS_CHECK_ARG(mock_bits >= 1 && mock_bits <= 32);
  const uint32_t mask = mock_bits == 32 ? 0xffffffffu : ((1u << mock_bits) - 1u);
  return ggms_gather_scatter_masked(dst, src, index, nullptr, num_index, nullptr, dim, dtype, mask, stream);
}

int ggms_gather_scatter_partition(void *out, const void *const *parts, uint32_t num_part,
                                  const ggms_id_t *src_index, const ggms_id_t *dst_index, size_t num,
                                  const uint64_t *num_dev, size_t dim, int dtype, ggms_stream_t stream) {
  const size_t es = ggms_dtype_bytes(dtype);
  GGMS_CHECK_ARG(es != 0 && dim != 0 && num_part != 0);
  if (num == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && parts && src_index);
  const size_t row_bytes = dim * es;
  // shard bases come from hipMalloc / hipIpcOpenMemHandle / hipHostMalloc: >= 256-B aligned
  const int cb = pick_chunk(row_bytes, (uintptr_t)out);
  PartPtrs pp;
  if (!part_ptrs(parts, num_part, pp)) return GGMS_ERR_INVALID;
  PartitionRows rows{pp, src_index, row_bytes, divisor_of(num_part)};
  return launch_gather((char *)out, rows, dst_index, num, count_of(num, num_dev), row_bytes, cb, nullptr,
                       to_stream(stream));
}

int ggms_extract_cached(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                        const ggms_id_t *table, const void *const *parts, uint32_t num_part,
                        const void *host_feat, size_t dim, int dtype, uint64_t *num_miss_dev,
                        ggms_stream_t stream) {
  return extract_cached_rows(out, nodes, num_nodes, num_nodes_dev, table, parts, num_part, host_feat, dim, dtype, dtype,
                             num_miss_dev, stream);
}

int ggms_extract_cached_convert(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                                const ggms_id_t *table, const void *const *parts, uint32_t num_part,
                                const void *host_feat, size_t dim, int src_dtype, int out_dtype,
                                uint64_t *num_miss_dev, ggms_stream_t stream) {
  return extract_cached_rows(out, nodes, num_nodes, num_nodes_dev, table, parts, num_part, host_feat, dim, src_dtype,
                             out_dtype, num_miss_dev, stream);
}

int ggms_extract_tiered(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                        const ggms_feature_tiers_t *tiers, size_t dim, int dtype, uint64_t *tier_rows_dev,
                        ggms_stream_t stream) {
  return extract_tiered_rows(out, nodes, num_nodes, num_nodes_dev, tiers, dim, dtype, dtype, tier_rows_dev, stream);
}

int ggms_extract_tiered_convert(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                                const ggms_feature_tiers_t *tiers, size_t dim, int src_dtype, int out_dtype,
                                uint64_t *tier_rows_dev, ggms_stream_t stream) {
  return extract_tiered_rows(out, nodes, num_nodes, num_nodes_dev, tiers, dim, src_dtype, out_dtype, tier_rows_dev,
                             stream);
}

int ggms_dynamic_cache_reset(uint64_t *stamps, size_t num_node, ggms_stream_t stream) {
  GGMS_CHECK_ARG(stamps || num_node == 0);
  if (num_node) GGMS_HIP(hipMemsetAsync(stamps, 0, num_node * sizeof(uint64_t), to_stream(stream)));
  return GGMS_OK;
}

int ggms_extract_dynamic(void *out, const ggms_id_t *nodes, size_t num_nodes, const uint64_t *num_nodes_dev,
                         const uint64_t *stamps, uint32_t seq, const void *prev_feat, const void *host_feat,
                         size_t dim, int dtype, uint64_t *num_miss_dev, ggms_stream_t stream) {
  const size_t es = ggms_dtype_bytes(dtype);
  GGMS_CHECK_ARG(es != 0 && dim != 0 && seq != 0);
  if (num_nodes == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && nodes && stamps && host_feat && (seq == 1 || prev_feat));
  GGMS_CHECK_ARG(num_nodes < (1ull << 32)); // slots travel in the low half of a stamp word
  const size_t row_bytes = dim * es;
  const int cb = pick_chunk(row_bytes, (uintptr_t)out | (uintptr_t)host_feat | (uintptr_t)prev_feat);
  DynamicRows rows{nodes, (const unsigned long long *)stamps, (const char *)prev_feat, (const char *)host_feat,
                   row_bytes, seq - 1};
  return launch_gather((char *)out, rows, nullptr, num_nodes, count_of(num_nodes, num_nodes_dev), row_bytes, cb,
                       num_miss_dev, to_stream(stream));
}

int ggms_dynamic_cache_publish(uint64_t *stamps, const ggms_id_t *nodes, size_t num_nodes,
                               const uint64_t *num_nodes_dev, uint32_t seq, ggms_stream_t stream) {
  GGMS_CHECK_ARG(seq != 0);
  if (num_nodes == 0) return GGMS_OK;
  GGMS_CHECK_ARG(stamps && nodes && num_nodes < (1ull << 32));
  hipLaunchKernelGGL(k_dynamic_publish, dim3(grid_for(num_nodes, kBlock)), dim3(kBlock), 0, to_stream(stream),
                     (unsigned long long *)stamps, nodes, count_of(num_nodes, num_nodes_dev), seq);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

// ---- launch timer ---------------------------------------------------------------------------------------------------
int ggms_launch_timer_create(ggms_launch_timer_t **timer) {
  GGMS_CHECK_ARG(timer);
  ggms_launch_timer *t = new ggms_launch_timer();
  hipError_t e = hipEventCreate(&t->start);
  if (e == hipSuccess) e = hipEventCreate(&t->stop);
  if (e != hipSuccess) {
    if (t->start) (void)hipEventDestroy(t->start);
    delete t;
    set_error("ggms_launch_timer_create: hipEventCreate -> %s", hipGetErrorString(e));
    return GGMS_ERR_HIP;
  }
  *timer = t;
  return GGMS_OK;
}

int ggms_launch_timer_destroy(ggms_launch_timer_t *timer) {
  if (!timer) return GGMS_OK;
  if (tl_armed_timer == timer) tl_armed_timer = nullptr;
  const hipError_t e0 = hipEventDestroy(timer->start), e1 = hipEventDestroy(timer->stop);
  delete timer;
  GGMS_HIP(e0);
  GGMS_HIP(e1);
  return GGMS_OK;
}

int ggms_launch_timer_arm(ggms_launch_timer_t *timer) {
  GGMS_CHECK_ARG(timer);
  timer->launched = false;
  tl_armed_timer = timer;
  return GGMS_OK;
}

int ggms_launch_timer_wait(ggms_launch_timer_t *timer, ggms_stream_t stream) {
  GGMS_CHECK_ARG(timer);
  if (timer->launched) GGMS_HIP(hipStreamWaitEvent(to_stream(stream), timer->stop, 0));
  return GGMS_OK;
}

int ggms_launch_timer_elapsed_us(ggms_launch_timer_t *timer, double *us) {
  GGMS_CHECK_ARG(timer && us);
  if (!timer->launched) {
    set_error("ggms_launch_timer_elapsed_us: the timer never rode a launch (armed on another thread, or the call had no rows)");
    return GGMS_ERR_INVALID;
  }
  GGMS_HIP(hipEventSynchronize(timer->stop));
  float ms = 0.f;
  GGMS_HIP(hipEventElapsedTime(&ms, timer->start, timer->stop));
  *us = (double)ms * 1e3;
  return GGMS_OK;
}

int ggms_launch_timer_span_us(ggms_launch_timer_t *first, ggms_launch_timer_t *last, double *us) {
  GGMS_CHECK_ARG(first && last && us);
  if (!first->launched || !last->launched) {
    set_error("ggms_launch_timer_span_us: a timer that never rode a launch");
    return GGMS_ERR_INVALID;
  }
  GGMS_HIP(hipEventSynchronize(first->stop));
  GGMS_HIP(hipEventSynchronize(last->stop));
  float ms = 0.f;
  GGMS_HIP(hipEventElapsedTime(&ms, first->start, last->stop));
  *us = (double)ms * 1e3;
  return GGMS_OK;
}

} // extern "C"
