// gather_typed.hip -- ggms_gather_typed: the feature rows of a heterogeneous batch, one table per node type, gathered
// into one buffer of per-type blocks (include/ggms.h has the definition).
//
// The batch's ids arrive grouped by type (ggms_hetero_nodes: typed_nodes + the T + 1 base words), so the work is the
// row gather's (extract.hip) with the row width, the table and the conversion changing a few times along the list.
//   * Every wave first turns the <= 33 base words into what it needs, one group per lane and no LDS: the clamped group
//     starts (a prefix maximum), the blocks' byte offsets (a 64-bit prefix sum of the padded block sizes) and the
//     prefix sum of the group sizes of THIS launch's class.  Workgroup 0 of the first launch writes the offsets out.
//   * A CLASS is what one kernel instance can move: CopyChunk<width> or ConvertChunk<width, src, out>.  The tables of
//     one call fall into a few classes, fixed by the table set; each gets one launch, which sweeps the rows of its own
//     types only -- their groups laid end to end are its dense index space, cut into tiles of 64 rows per wave.
//   * Each lane resolves one row of a tile: its type (compare-and-count over the groups' starts), slot, node, table row,
//     source and destination pointer.  The next tile's chain is in flight while this tile's rows stream, as in
//     k_gather_rows.  A tile holds a few RUNS of equal type; a run is swept as a flat array of chunks with the type's
//     chunks-per-row and multiply-high magic read from the kernel arguments (the run's type is uniform).
//   * A row with no source (an id that is no node, a rank beyond the table) is stored as zero bytes and nothing is
//     loaded for it.  The wave that moves a block's last row also writes the block's zero pad (< 16 bytes).
// Algorithmic bytes per row: 4 (id) [+ 4 (rank)] + source row + output row.  No atomics: a byte's writer is a function
// of its position, so the output does not depend on the grid.
#include <hip/hip_ext.h>

#include "ggms_internal.h"
#include "row_chunks.h"

namespace ggms {

constexpr uint32_t kMaxNodeTypes = GGMS_MAX_NODE_TYPES;

// the table set as the kernel sees it (by value): everything a lane needs about its type
struct TypedTables {
  const char *table[kMaxNodeTypes];
  uint64_t num_rows[kMaxNodeTypes];
  uint32_t src_rb[kMaxNodeTypes];     // bytes from one table row to the next
  uint32_t out_rb[kMaxNodeTypes];     // rb_t: bytes of an output row; 0 for a type without a table
  uint32_t rc[kMaxNodeTypes];         // chunks per row, in the width of the type's class
  uint32_t magic[kMaxNodeTypes];      // ceil(2^32 / rc); 0 for rc == 1
  uint32_t first_node[kMaxNodeTypes];
  uint32_t num_type;
  uint32_t mine;                      // bit t: type t is of this launch's class
  uint32_t write_offsets;             // the first launch of a call
};

__device__ __forceinline__ uint32_t read_lane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t read_lane64(uint64_t v, uint32_t l) {
  return ((uint64_t)read_lane((uint32_t)(v >> 32), l) << 32) | read_lane((uint32_t)v, l);
}

template <typename Chunk, int U>
__global__ __launch_bounds__(kBlock) void k_gather_typed(char *__restrict__ out, TypedTables P,
                                                         const uint32_t *__restrict__ typed_nodes,
                                                         const uint32_t *__restrict__ base_dev, uint32_t max_nodes,
                                                         const uint32_t *__restrict__ row_of_node, uint64_t num_node,
                                                         uint64_t *__restrict__ out_offset) {
  using SV = typename Chunk::Src;
  using DV = typename Chunk::Dst;
  constexpr uint32_t SB = Chunk::kSrcBytes, DB = Chunk::kDstBytes;
  const uint32_t lane = lane_id();
  const uint32_t T = P.num_type; // 1 .. 32

  // ---- the groups, one per lane (lane T: the end) ----------------------------------------------------------------
  // b[t] = max over u <= t of min(base[u], max_nodes): nothing behind max_nodes, and groups that cannot overlap or run
  // backwards whatever the words are -- the sizes add up to at most max_nodes, which is what `out` is sized for
  uint32_t b = 0;
  if (lane <= T) {
    b = base_dev[lane];
    b = b < max_nodes ? b : max_nodes;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(b, o, 64);
    if ((int)lane >= o && y > b) b = y;
  }
  const uint32_t b_next = __shfl_down(b, 1, 64);
  const bool is_type = lane < T;
  const uint32_t cnt = is_type ? b_next - b : 0u;
  const uint32_t rb = is_type ? P.out_rb[lane] : 0u;
  const uint64_t bytes = (uint64_t)cnt * rb;
  const uint64_t padded = (bytes + 15u) & ~(uint64_t)15u;
  uint64_t off = padded; // inclusive scan, then made exclusive: off[t]; every lane >= T ends up with off[T]
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = shfl_u64(off, (int)lane - o);
    if ((int)lane >= o) off += y;
  }
  off -= padded;
  const uint32_t dcnt = (is_type && ((P.mine >> lane) & 1u)) ? cnt : 0u;
  const uint32_t d_end = wave_inclusive_scan(dcnt); // dense index behind my group
  const uint32_t d = d_end - dcnt;                  // ... and of its first row
  const uint32_t total = read_lane(d_end, 63);
  if (P.write_offsets && blockIdx.x == 0 && threadIdx.x <= T) out_offset[threadIdx.x] = off;

  // (the wave's number through readfirstlane: the tile and run loops below are uniform, and the compiler may know it)
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t num_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t num_tiles = ((uint64_t)total + kWave - 1) / kWave;

  // resolve one row per lane for tile `tile`: its type, source pointer (0: a zero row) and destination pointer
  auto resolve = [&](uint64_t tile, uint32_t &ty, uint64_t &sp, uint64_t &dp) {
    const uint64_t i64 = tile * kWave + lane;
    const bool live = tile < num_tiles && i64 < total;
    const uint32_t i = live ? (uint32_t)i64 : 0u;
    // the last group that starts at or before i: the starts ascend, so it is a count; its group is not empty and of
    // this class, because i lies before the next start
    uint32_t t = 0;
#pragma unroll 1
    for (uint32_t k = 1; k < T; ++k) t += (i >= read_lane(d, k)) ? 1u : 0u;
    const uint32_t j = i - __shfl(d, (int)t, 64);
    const uint32_t slot = __shfl(b, (int)t, 64) + j;
    const uint64_t o = shfl_u64(off, (int)t);
    ty = 0xffffffffu; sp = 0; dp = 0;
    if (live) {
      ty = t;
      const uint32_t v = typed_nodes[slot];
      dp = (uint64_t)(out + o + (uint64_t)j * P.out_rb[t]);
      if ((uint64_t)v < num_node) {
        const int64_t row = row_of_node ? (int64_t)row_of_node[v] : (int64_t)v - (int64_t)P.first_node[t];
        if (row >= 0 && (uint64_t)row < P.num_rows[t]) sp = (uint64_t)(P.table[t] + (uint64_t)row * P.src_rb[t]);
      }
    }
  };

  uint32_t ty;
  uint64_t sp, dp;
  resolve(wave, ty, sp, dp);
  for (uint64_t tile = wave; tile < num_tiles; tile += num_waves) {
    uint32_t ty_n;
    uint64_t sp_n, dp_n;
    resolve(tile + num_waves, ty_n, sp_n, dp_n); // in flight while this tile's rows stream

    const uint64_t row0 = tile * kWave;
    const uint32_t rows_here = (total - row0 < (uint64_t)kWave) ? (uint32_t)(total - row0) : (uint32_t)kWave;
    uint32_t l0 = 0;
    while (l0 < rows_here) { // one round per run of equal type; everything about the run is uniform
      const uint32_t t = read_lane(ty, l0);
      const uint32_t n_run = (uint32_t)__popcll(__ballot(ty == t));
      const uint32_t rc = P.rc[t], magic = P.magic[t];
      const uint32_t run_chunks = n_run * rc;
      const uint64_t out_run = read_lane64(dp, l0); // the block's rows are dense: chunk c of the run lies c chunks on
      for (uint32_t c0 = 0; c0 < run_chunks; c0 += kWave * U) {
        SV tmp[U];
        uint32_t cc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t c = c0 + u * kWave + lane;
          cc[u] = c < run_chunks ? c : run_chunks - 1; // clamp: the load does not depend on c, the store does
          // cc / rc, exact for cc * rc < 2^32 (rc < 8192, cc < 64 * rc); rc == 1 has magic = 0 and takes cc itself
          const uint32_t r = __umulhi(cc[u], magic) + (rc == 1 ? cc[u] : 0u);
          const uint32_t col = cc[u] - r * rc;
          const uint64_t p = shfl_u64(sp, (int)(l0 + r));
          SV z{};
          tmp[u] = p ? load_chunk<SV, true>(p + (uint64_t)col * SB) : z;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t c = c0 + u * kWave + lane;
          if (c < run_chunks) store_chunk<DV, true>(out_run + (uint64_t)cc[u] * DB, Chunk::convert(tmp[u]));
        }
      }
      // the run that ends its type's group owns the block's pad: zero bytes up to the next multiple of 16
      if (row0 + l0 + n_run == read_lane(d_end, t)) {
        const uint64_t end = read_lane64(off, t) + read_lane64(bytes, t);
        const uint32_t pad = (uint32_t)(read_lane64(padded, t) - read_lane64(bytes, t));
        if (lane < pad) store_chunk<uint8_t, false>((uint64_t)(out + end + lane), (uint8_t)0);
      }
      l0 += n_run;
    }
    ty = ty_n; sp = sp_n; dp = dp_n;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// how one type's rows are moved: plain (src == out dtype: `width` bytes per chunk) or converting (`width` elements)
struct TypedClass {
  int src_dt, out_dt, width;
  bool same(const TypedClass &o) const {
    if (src_dt == out_dt && o.src_dt == o.out_dt) return width == o.width; // every plain copy of one width is one class
    return src_dt == o.src_dt && out_dt == o.out_dt && width == o.width;
  }
};

static TypedClass class_of(const ggms_typed_table_t &tb, const void *out) {
  const size_t ses = ggms_dtype_bytes(tb.src_dtype), des = ggms_dtype_bytes(tb.out_dtype);
  if (tb.src_dtype == tb.out_dtype)
    return TypedClass{tb.src_dtype, tb.out_dtype, pick_chunk((size_t)tb.dim * ses, (uintptr_t)tb.table | (uintptr_t)out)};
  return TypedClass{tb.src_dtype, tb.out_dtype,
                    pick_chunk(tb.dim, convert_max_epc(ses, des), ses, (uintptr_t)tb.table, des, (uintptr_t)out)};
}
static uint64_t chunks_per_row(const ggms_typed_table_t &tb, const TypedClass &c) {
  return tb.src_dtype == tb.out_dtype ? (uint64_t)tb.dim * ggms_dtype_bytes(tb.src_dtype) / c.width : (uint64_t)tb.dim / c.width;
}

struct TypedLaunch {
  char *out;
  const uint32_t *typed_nodes, *base_dev, *row_of_node;
  uint32_t max_nodes;
  uint64_t num_node;
  uint64_t *out_offset;
  int grid;
  hipStream_t stream;
};

template <typename Chunk>
static void launch_typed_chunk(const TypedLaunch &l, const TypedTables &P, bool deep) {
  hipEvent_t start, stop;
  const bool timed = take_armed_timer(&start, &stop); // rides on the first launch of the call
#define GGMS_TYPED(UU)                                                                                                \
  do {                                                                                                                \
    if (timed)                                                                                                        \
      hipExtLaunchKernelGGL((k_gather_typed<Chunk, UU>), dim3(l.grid), dim3(kBlock), 0, l.stream, start, stop, 0, l.out, \
                            P, l.typed_nodes, l.base_dev, l.max_nodes, l.row_of_node, l.num_node, l.out_offset);       \
    else                                                                                                              \
      hipLaunchKernelGGL((k_gather_typed<Chunk, UU>), dim3(l.grid), dim3(kBlock), 0, l.stream, l.out, P, l.typed_nodes, \
                         l.base_dev, l.max_nodes, l.row_of_node, l.num_node, l.out_offset);                            \
  } while (0)
  if (deep) GGMS_TYPED(16);
  else GGMS_TYPED(8);
#undef GGMS_TYPED
}

template <int S, int D>
static bool launch_typed_pair(const TypedLaunch &l, const TypedTables &P, bool deep, int epc) {
  constexpr int kMaxEpc = convert_max_epc(sizeof(typename Elem<S>::bits), sizeof(typename Elem<D>::bits));
  if constexpr (kMaxEpc == 8)
    if (epc == 8) return launch_typed_chunk<ConvertChunk<8, S, D>>(l, P, deep), true;
  switch (epc) {
    case 4: return launch_typed_chunk<ConvertChunk<4, S, D>>(l, P, deep), true;
    case 2: return launch_typed_chunk<ConvertChunk<2, S, D>>(l, P, deep), true;
    case 1: return launch_typed_chunk<ConvertChunk<1, S, D>>(l, P, deep), true;
  }
  return false;
}

static bool launch_typed_class(const TypedLaunch &l, const TypedTables &P, bool deep, const TypedClass &c) {
  if (c.src_dt == c.out_dt) {
    switch (c.width) {
      case 16: return launch_typed_chunk<CopyChunk<16>>(l, P, deep), true;
      case 8: return launch_typed_chunk<CopyChunk<8>>(l, P, deep), true;
      case 4: return launch_typed_chunk<CopyChunk<4>>(l, P, deep), true;
      case 2: return launch_typed_chunk<CopyChunk<2>>(l, P, deep), true;
    } // (no 1-byte chunk: the elements have 2 or 4 bytes and both sides are aligned to them)
    return false;
  }
#define GGMS_PAIR(S, D) \
  if (c.src_dt == S && c.out_dt == D) return launch_typed_pair<S, D>(l, P, deep, c.width);
  GGMS_PAIR(GGMS_F16, GGMS_F32)
  GGMS_PAIR(GGMS_BF16, GGMS_F32)
  GGMS_PAIR(GGMS_F32, GGMS_F16)
  GGMS_PAIR(GGMS_F32, GGMS_BF16)
  GGMS_PAIR(GGMS_F16, GGMS_BF16)
  GGMS_PAIR(GGMS_BF16, GGMS_F16)
#undef GGMS_PAIR
  return false;
}

constexpr uint64_t kTypedMaxNodes = (1ull << 32) - 1024;

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_gather_typed_out_bytes(const ggms_typed_table_t *tables, uint32_t num_type, size_t max_nodes) {
  if (!tables || num_type == 0 || num_type > kMaxNodeTypes || (uint64_t)max_nodes >= kTypedMaxNodes) return 0;
  uint64_t widest = 0;
  for (uint32_t t = 0; t < num_type; ++t) {
    if (tables[t].dim == 0) continue;
    if (!is_float_dtype(tables[t].src_dtype) || !is_float_dtype(tables[t].out_dtype)) return 0;
    const uint64_t rb = (uint64_t)tables[t].dim * ggms_dtype_bytes(tables[t].out_dtype);
    if (rb > widest) widest = rb;
  }
  size_t need;
  if (__builtin_mul_overflow((size_t)max_nodes, (size_t)widest, &need) || __builtin_add_overflow(need, (size_t)16 * num_type, &need))
    return 0;
  return need;
}

int ggms_gather_typed(void *out, size_t out_bytes, const ggms_typed_table_t *tables, uint32_t num_type,
                      const ggms_id_t *typed_nodes, const uint32_t *base_dev, size_t max_nodes,
                      const uint32_t *row_of_node, size_t num_node, uint64_t *out_offset_dev, ggms_stream_t stream) {
#define GGMS_TYPED_REFUSE(...)                  \
  do {                                          \
    set_error("ggms_gather_typed: " __VA_ARGS__); \
    return GGMS_ERR_INVALID;                    \
  } while (0)
  if (!tables) GGMS_TYPED_REFUSE("invalid argument: tables is NULL (a HOST array of num_type entries)");
  if (num_type == 0 || num_type > kMaxNodeTypes)
    GGMS_TYPED_REFUSE("invalid argument: num_type %u (1 .. %u node types)", num_type, kMaxNodeTypes);
  if (!out) GGMS_TYPED_REFUSE("invalid argument: out is NULL");
  if (!typed_nodes) GGMS_TYPED_REFUSE("invalid argument: typed_nodes is NULL");
  if (!base_dev) GGMS_TYPED_REFUSE("invalid argument: base_dev is NULL (num_type + 1 device words)");
  if (!out_offset_dev) GGMS_TYPED_REFUSE("invalid argument: out_offset_dev is NULL (num_type + 1 device words)");
  if ((uint64_t)max_nodes >= kTypedMaxNodes)
    GGMS_TYPED_REFUSE("invalid argument: max_nodes %zu (below 2^32 - 1024)", max_nodes);
  if ((uintptr_t)out_offset_dev % 8 != 0) GGMS_TYPED_REFUSE("invalid argument: out_offset_dev is not 8-byte aligned");

  TypedTables P = {};
  TypedClass cls[kMaxNodeTypes];
  P.num_type = num_type;
  for (uint32_t t = 0; t < num_type; ++t) {
    const ggms_typed_table_t &tb = tables[t];
    if (tb.dim == 0) continue;
    if (!is_float_dtype(tb.src_dtype))
      GGMS_TYPED_REFUSE("invalid argument: tables[%u].src_dtype %d (GGMS_F32, GGMS_F16 or GGMS_BF16)", t, tb.src_dtype);
    if (!is_float_dtype(tb.out_dtype))
      GGMS_TYPED_REFUSE("invalid argument: tables[%u].out_dtype %d (GGMS_F32, GGMS_F16 or GGMS_BF16)", t, tb.out_dtype);
    if (!tb.table) GGMS_TYPED_REFUSE("invalid argument: tables[%u].table is NULL with dim %u", t, tb.dim);
    const size_t ses = ggms_dtype_bytes(tb.src_dtype), des = ggms_dtype_bytes(tb.out_dtype);
    if ((uintptr_t)tb.table % ses != 0)
      GGMS_TYPED_REFUSE("invalid argument: tables[%u].table is not aligned to its %zu-byte element", t, ses);
    if ((uintptr_t)out % des != 0)
      GGMS_TYPED_REFUSE("invalid argument: out is not aligned to the %zu-byte element of type %u", des, t);
    cls[t] = class_of(tb, out);
    const uint64_t rc = chunks_per_row(tb, cls[t]);
    if (rc >= 8192)
      GGMS_TYPED_REFUSE("invalid argument: tables[%u].dim %u is a row of %llu chunks (below 8192: the tile sweep's "
                        "chunk-to-row division is exact only there)", t, tb.dim, (unsigned long long)rc);
    P.table[t] = (const char *)tb.table;
    P.num_rows[t] = tb.num_rows;
    P.src_rb[t] = (uint32_t)(tb.dim * ses);
    P.out_rb[t] = (uint32_t)(tb.dim * des);
    P.rc[t] = (uint32_t)rc;
    P.magic[t] = rc == 1 ? 0u : (uint32_t)(((1ull << 32) + rc - 1) / rc);
    P.first_node[t] = tb.first_node;
  }
  const size_t need = ggms_gather_typed_out_bytes(tables, num_type, max_nodes);
  if (need == 0 || out_bytes < need)
    GGMS_TYPED_REFUSE("invalid argument: out_bytes %zu is below ggms_gather_typed_out_bytes = %zu", out_bytes, need);
#undef GGMS_TYPED_REFUSE

  // one wave per 64 rows, grid-stride, under the gathers' cap (GGMS_EXTRACT_BLOCKS)
  int grid = grid_for(max_nodes, kBlock);
  if (grid > gather_max_blocks()) grid = gather_max_blocks();
  const TypedLaunch l{(char *)out, typed_nodes, base_dev, row_of_node, (uint32_t)max_nodes, (uint64_t)num_node,
                      out_offset_dev, grid, to_stream(stream)};
  // one launch per class present among the tables; a call without a table still writes its (zero) offsets
  uint32_t todo = 0;
  for (uint32_t t = 0; t < num_type; ++t)
    if (tables[t].dim != 0) todo |= 1u << t;
  P.write_offsets = 1;
  if (todo == 0) {
    launch_typed_chunk<CopyChunk<16>>(l, P, false);
    GGMS_LAUNCH_CHECK();
    return GGMS_OK;
  }
  while (todo) {
    const uint32_t t0 = (uint32_t)__builtin_ctz(todo);
    uint32_t mine = 0, min_rc = 0xffffffffu;
    for (uint32_t t = t0; t < num_type; ++t)
      if (((todo >> t) & 1u) && cls[t].same(cls[t0])) {
        mine |= 1u << t;
        if (P.rc[t] < min_rc) min_rc = P.rc[t];
      }
    P.mine = mine;
    // 16 chunk loads per lane in flight once every row of the class has >= 8 chunks, else 8 (as the row gather)
    if (!launch_typed_class(l, P, min_rc >= 8, cls[t0])) {
      set_error("ggms_gather_typed: no kernel for dtype %d -> %d in chunks of %d", cls[t0].src_dt, cls[t0].out_dt, cls[t0].width);
      return GGMS_ERR_INVALID;
    }
    GGMS_LAUNCH_CHECK();
    P.write_offsets = 0;
    todo &= ~mine;
  }
  return GGMS_OK;
}

} // extern "C"
