// update_rows.hip -- the write side of the row sweep: a learnable F32 feature table takes a batch's gradient.
//
//     for i < count, v = nodes[i] != kEmptyKey:   table[v, :] (and state[v, :]) <- rule(table[v, :], state[v, :], grad[i, :])
//
// The gather's mirror image (extract.hip, k_gather_rows) and HBM-bound like it:
//   * one wave owns 64 consecutive GRADIENT rows; each lane resolves ONE nodes[i] into the byte offset of its table
//     row (the state row lies at the same offset of its own base);
//   * the tile is swept as a flat array of 16-byte chunks: chunk c belongs to row c / chunks_per_row, the owner's
//     offset comes through ds_bpermute (no LDS memory), so the gradient side is one contiguous stream whatever a row's
//     length is;
//   * U chunks per lane have all their loads (gradient, table, state) issued before the first store;
//   * the gradient is read once: non-temporal.  Table and state rows are read and written in place with plain
//     accesses -- the next gather may find them in cache;
//   * the nodes of a call are pairwise distinct (include/ggms.h), so no two chunks alias: no atomics, no workspace.
// Algorithmic bytes per row: 4 (index) + 3 x row_bytes for SGD (gradient in, row in, row out), + 2 x row_bytes for
// Adagrad (state in, state out).
//
// Arithmetic: every operation of a rule is ONE IEEE f32 operation, round to nearest even, subnormals kept; nothing is
// contracted into an FMA (the pragma in update_one; ScaledChunk in extract.hip says why it is needed).  Division and
// square root are the correctly rounded ones: the Makefile passes neither fast-math nor a flush flag, and hipcc's
// default for HIP is -fhip-fp32-correctly-rounded-divide-sqrt.
#include <cmath>

#include "ggms_device.h"
#include "row_formats.h"

namespace ggms {

// one element: w (and s) in, w (and s) out
template <int RULE>
__device__ __forceinline__ void update_one(float &w, [[maybe_unused]] float &s, float g, float lr,
                                           [[maybe_unused]] float eps) {
#pragma clang fp contract(off)
  if constexpr (RULE == GGMS_UPDATE_SGD) {
    const float step = lr * g;
    w = w - step;
  } else {
    const float gg = g * g;
    s = s + gg;
    const float num = lr * g;
    const float root = __builtin_sqrtf(s);
    const float den = root + eps;
    const float step = num / den;
    w = w - step;
  }
}

// a chunk of V f32 elements, as the bits a load delivers
template <int V, int RULE>
__device__ __forceinline__ void update_chunk(typename VecT<uint32_t, V>::type &w, typename VecT<uint32_t, V>::type &s,
                                             const typename VecT<uint32_t, V>::type &g, float lr, float eps) {
  using VT = typename VecT<uint32_t, V>::type;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float we = __builtin_bit_cast(float, (uint32_t)vec_get<VT, V>(w, e));
    float se = __builtin_bit_cast(float, (uint32_t)vec_get<VT, V>(s, e));
    update_one<RULE>(we, se, __builtin_bit_cast(float, (uint32_t)vec_get<VT, V>(g, e)), lr, eps);
    vec_set<VT, V>(w, e, __builtin_bit_cast(uint32_t, we));
    if constexpr (RULE == GGMS_UPDATE_ADAGRAD) vec_set<VT, V>(s, e, __builtin_bit_cast(uint32_t, se));
  }
}

constexpr uint64_t kNoRow = ~0ull; // the offset of a skipped entry (kEmptyKey)

// the count of a call: the device word where there is one, never beyond the bound the launch was sized for
__device__ __forceinline__ uint64_t bounded_count(const Count &n) {
  const uint64_t v = n.get();
  return v < n.imm ? v : n.imm;
}

// V elements per chunk; rc chunks per row (< 8192); magic = ceil(2^32 / rc), 0 for rc == 1
template <int V, int RULE, int U>
__global__ __launch_bounds__(kBlock) void k_update_rows(char *__restrict__ table, char *__restrict__ state,
                                                        const uint32_t *__restrict__ nodes, Count n_arg,
                                                        const char *__restrict__ grad, uint32_t rc, uint32_t magic,
                                                        float lr, float eps) {
  using VT = typename VecT<uint32_t, V>::type;
  constexpr uint32_t CB = V * 4;
  constexpr bool kState = RULE == GGMS_UPDATE_ADAGRAD;
  const uint64_t n = bounded_count(n_arg);
  const uint32_t lane = lane_id();
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const uint64_t num_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t row_bytes = (uint64_t)rc * CB;
  const uint64_t num_tiles = (n + kWave - 1) / kWave;

  // one entry per lane for tile t: the byte offset of its table row
  auto resolve = [&](uint64_t t) -> uint64_t {
    const uint64_t my_row = t * kWave + lane;
    if (t < num_tiles && my_row < n) {
      const uint32_t v = nodes[my_row];
      if (v != kEmptyKey) return (uint64_t)v * row_bytes;
    }
    return kNoRow;
  };

  uint64_t off = resolve(wave);
  for (uint64_t tile = wave; tile < num_tiles; tile += num_waves) {
    const uint64_t off_n = resolve(tile + num_waves); // the next tile's ids are in flight while this tile streams
    const uint64_t row0 = tile * kWave;
    const uint32_t rows_here = (n - row0 < (uint64_t)kWave) ? (uint32_t)(n - row0) : (uint32_t)kWave;
    const uint32_t total = rows_here * rc; // chunks in this tile
    const uint64_t grad_tile = (uint64_t)(grad + row0 * row_bytes);
    for (uint32_t c0 = 0; c0 < total; c0 += kWave * U) {
      VT g[U], w[U];
      [[maybe_unused]] VT s[U];
      uint64_t q[U]; // offset of the chunk in table and state; kNoRow: nothing to do
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t c = c0 + u * kWave + lane;
        const uint32_t cc = c < total ? c : total - 1; // clamp: the shuffle is wave-wide
        // cc / rc, exact for cc * rc < 2^32; rc == 1 has magic = 0 and takes cc itself
        const uint32_t r = __umulhi(cc, magic) + (rc == 1 ? cc : 0u);
        const uint64_t p = shfl_u64(off, (int)r);
        q[u] = (c < total && p != kNoRow) ? p + (uint64_t)(cc - r * rc) * CB : kNoRow;
        g[u] = VT{};
        w[u] = VT{};
        if constexpr (kState) s[u] = VT{};
        if (q[u] != kNoRow) {
          g[u] = load_chunk<VT, true>(grad_tile + (uint64_t)cc * CB);
          w[u] = load_chunk<VT, false>((uint64_t)table + q[u]);
          if constexpr (kState) s[u] = load_chunk<VT, false>((uint64_t)state + q[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (q[u] == kNoRow) continue;
        update_chunk<V, RULE>(w[u], s[u], g[u], lr, eps);
        store_chunk<VT, false>((uint64_t)table + q[u], w[u]);
        if constexpr (kState) store_chunk<VT, false>((uint64_t)state + q[u], s[u]);
      }
    }
    off = off_n;
  }
}

// Rows of 8192 chunks or more (the tile sweep's chunk -> row division is exact only below that): every row is a long
// contiguous stream by itself, so one workgroup updates one row.
template <int V, int RULE>
__global__ __launch_bounds__(kBlock) void k_update_long_rows(char *__restrict__ table, char *__restrict__ state,
                                                             const uint32_t *__restrict__ nodes, Count n_arg,
                                                             const char *__restrict__ grad, uint64_t rc, float lr,
                                                             float eps) {
  using VT = typename VecT<uint32_t, V>::type;
  constexpr uint32_t CB = V * 4;
  constexpr bool kState = RULE == GGMS_UPDATE_ADAGRAD;
  constexpr int U = 4;
  const uint64_t n = bounded_count(n_arg);
  const uint64_t row_bytes = rc * CB;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t v = nodes[i];
    if (v == kEmptyKey) continue; // uniform
    const uint64_t tp = (uint64_t)table + (uint64_t)v * row_bytes, sp = (uint64_t)state + (uint64_t)v * row_bytes;
    const uint64_t gp = (uint64_t)grad + i * row_bytes;
    for (uint64_t c0 = threadIdx.x; c0 < rc; c0 += (uint64_t)kBlock * U) {
      VT g[U], w[U];
      [[maybe_unused]] VT s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t c = c0 + (uint64_t)u * kBlock;
        g[u] = VT{};
        w[u] = VT{};
        if constexpr (kState) s[u] = VT{};
        if (c < rc) {
          g[u] = load_chunk<VT, true>(gp + c * CB);
          w[u] = load_chunk<VT, false>(tp + c * CB);
          if constexpr (kState) s[u] = load_chunk<VT, false>(sp + c * CB);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t c = c0 + (uint64_t)u * kBlock;
        if (c >= rc) continue;
        update_chunk<V, RULE>(w[u], s[u], g[u], lr, eps);
        store_chunk<VT, false>(tp + c * CB, w[u]);
        if constexpr (kState) store_chunk<VT, false>(sp + c * CB, s[u]);
      }
    }
  }
}

// One wave per 64 rows, grid-stride.  At most two 4-wave blocks per CU: a lane holds U chunks of gradient, row (and
// state) between its loads and its first store, so a few waves per SIMD already keep the memory side busy.
constexpr int kUpdateMaxBlocks = 512;

template <int V, int RULE>
static int launch_update(char *table, char *state, const uint32_t *nodes, size_t n_max, Count n, const char *grad,
                         uint64_t rc, float lr, float eps, hipStream_t stream) {
  if (rc >= 8192) {
    hipLaunchKernelGGL((k_update_long_rows<V, RULE>), dim3(grid_for(n_max, 1)), dim3(kBlock), 0, stream, table, state,
                       nodes, n, grad, rc, lr, eps);
    GGMS_LAUNCH_CHECK();
    return GGMS_OK;
  }
  const uint32_t magic = rc == 1 ? 0u : (uint32_t)(((1ull << 32) + rc - 1) / rc);
  int grid = grid_for(n_max, kBlock);
  if (grid > kUpdateMaxBlocks) grid = kUpdateMaxBlocks;
  hipLaunchKernelGGL((k_update_rows<V, RULE, 8>), dim3(grid), dim3(kBlock), 0, stream, table, state, nodes, n, grad,
                     (uint32_t)rc, magic, lr, eps);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

template <int RULE>
static int launch_update_rule(int cb, char *table, char *state, const uint32_t *nodes, size_t n_max, Count n,
                              const char *grad, size_t row_bytes, float lr, float eps, hipStream_t stream) {
  const uint64_t rc = row_bytes / cb;
  switch (cb) {
    case 16: return launch_update<4, RULE>(table, state, nodes, n_max, n, grad, rc, lr, eps, stream);
    case 8: return launch_update<2, RULE>(table, state, nodes, n_max, n, grad, rc, lr, eps, stream);
    default: return launch_update<1, RULE>(table, state, nodes, n_max, n, grad, rc, lr, eps, stream);
  }
}

} // namespace ggms

using namespace ggms;

extern "C" int ggms_update_rows(void *table, void *state, const ggms_id_t *nodes, size_t num_nodes,
                                const uint64_t *num_nodes_dev, const void *grad, size_t dim, int rule, float lr,
                                float eps, ggms_stream_t stream) {
  if (rule != GGMS_UPDATE_SGD && rule != GGMS_UPDATE_ADAGRAD) {
    set_error("update_rows: invalid argument: rule %d (GGMS_UPDATE_SGD = 0 or GGMS_UPDATE_ADAGRAD = 1)", rule);
    return GGMS_ERR_INVALID;
  }
  if (dim == 0) {
    set_error("update_rows: invalid argument: dim 0 (empty rows)");
    return GGMS_ERR_INVALID;
  }
  if (!std::isfinite(lr)) {
    set_error("update_rows: invalid argument: lr is not finite");
    return GGMS_ERR_INVALID;
  }
  if (rule == GGMS_UPDATE_ADAGRAD && !(std::isfinite(eps) && eps > 0.0f)) {
    set_error("update_rows: invalid argument: Adagrad takes a finite eps > 0 (got %g)", (double)eps);
    return GGMS_ERR_INVALID;
  }
  if (num_nodes == 0) return GGMS_OK;
  if (!table || !nodes || !grad) {
    set_error("update_rows: invalid argument: null %s", !table ? "table" : !nodes ? "nodes" : "grad");
    return GGMS_ERR_INVALID;
  }
  if (rule == GGMS_UPDATE_ADAGRAD && !state) {
    set_error("update_rows: invalid argument: Adagrad needs `state` (the accumulator, shaped like the table)");
    return GGMS_ERR_INVALID;
  }
  if (rule == GGMS_UPDATE_SGD) state = nullptr; // not read: it does not bound the chunk width either
  const uintptr_t bits = (uintptr_t)table | (uintptr_t)state | (uintptr_t)grad;
  if (bits % 4 != 0) {
    set_error("update_rows: invalid argument: table, state and grad hold f32 and must be 4-byte aligned");
    return GGMS_ERR_INVALID;
  }
  const size_t row_bytes = dim * 4;
  const int cb = pick_chunk(row_bytes, bits); // 16, 8 or 4: f32 rows and 4-byte aligned bases
  const Count n = count_of(num_nodes, num_nodes_dev);
  if (rule == GGMS_UPDATE_SGD)
    return launch_update_rule<GGMS_UPDATE_SGD>(cb, (char *)table, nullptr, nodes, num_nodes, n, (const char *)grad,
                                               row_bytes, lr, eps, to_stream(stream));
  return launch_update_rule<GGMS_UPDATE_ADAGRAD>(cb, (char *)table, (char *)state, nodes, num_nodes, n,
                                                 (const char *)grad, row_bytes, lr, eps, to_stream(stream));
}
