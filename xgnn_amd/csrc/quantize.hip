// quantize.hip -- the write side of the narrow feature tables: F32 / F16 rows encoded into F16, BF16, the two OCP
// 8-bit floats or the row-scaled GGMS_Q8ROW format (ggms_quantize_rows, include/ggms.h).  The row gather (extract.hip)
// decodes what this file writes; the results are defined bit for bit by the CPU tools of xgnn_amd/datagen.py.
//
// A streaming pass: every source byte is read once (Q8ROW rows beyond kRegDim elements: twice), every output byte
// written once, nothing is reused -- loads and stores are non-temporal.
//   * F16 / BF16 / F8E4M3 / F8E5M2: rows are dense on both sides, so the table is one flat array of elements; a
//     grid-stride loop over chunks of up to 16 source bytes, kElemU chunks per lane in flight.
//   * Q8ROW needs the row's minimum and maximum before its first code.  A row belongs to a power-of-two group of G
//     lanes of one wave (64 / G rows per wave): the lanes load the row once, in chunks of up to 16 bytes, keep it in
//     registers as f32 (at most kRegElems values per lane), reduce min / max / "holds NaN or inf" across the group
//     with lane shuffles (no LDS memory), and encode from the registers.  dim 128 f32: 32 lanes x 16 B, two rows per
//     wave, one pass.  Rows of more than kRegDim elements take k_q8row_long: one wave per row, which reads it twice.
//   * The encode itself is float64, as quantize_q8row computes it: one subtraction, one correctly rounded division and
//     one round-half-even per element.
#include "row_formats.h"
#include "fp8_encode.h"
#include "ggms_device.h"

namespace ggms {

// ---- element encoders: f32 -> the output type's bits --------------------------------------------------------------
template <int DT> struct Encode {
  using bits = typename Elem<DT>::bits;
  static __device__ __forceinline__ bits one(float f) { return Elem<DT>::from_f32(f); }
};
template <> struct Encode<GGMS_F8E4M3> {
  using bits = uint8_t;
  static __device__ __forceinline__ bits one(float f) { return f32_to_fp8_e4m3(f); }
};
template <> struct Encode<GGMS_F8E5M2> {
  using bits = uint8_t;
  static __device__ __forceinline__ bits one(float f) { return f32_to_fp8_e5m2(f); }
};

// ---- the elementwise formats ----------------------------------------------------------------------------------------
constexpr int kElemU = 4; // independent chunk loads per lane before the first store

template <int SRC_DT, int DST_DT, int EPC>
__global__ __launch_bounds__(kBlock) void k_encode_elems(char *__restrict__ out, const char *__restrict__ src, uint64_t n) {
  using S = Elem<SRC_DT>;
  using D = Encode<DST_DT>;
  using SV = typename VecT<typename S::bits, EPC>::type;
  using DV = typename VecT<typename D::bits, EPC>::type;
  constexpr uint64_t SB = EPC * sizeof(typename S::bits), DB = EPC * sizeof(typename D::bits);
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x, threads = (uint64_t)gridDim.x * kBlock;
  const uint64_t chunks = n / EPC;
  for (uint64_t c0 = tid; c0 < chunks; c0 += threads * kElemU) {
    SV v[kElemU];
#pragma unroll
    for (int u = 0; u < kElemU; ++u) {
      const uint64_t c = c0 + u * threads;
      if (c < chunks) v[u] = load_chunk<SV, true>((uint64_t)src + c * SB);
    }
#pragma unroll
    for (int u = 0; u < kElemU; ++u) {
      const uint64_t c = c0 + u * threads;
      if (c < chunks) {
        DV o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) vec_set<DV, EPC>(o, e, D::one(S::to_f32(vec_get<SV, EPC>(v[u], e))));
        store_chunk<DV, true>((uint64_t)out + c * DB, o);
      }
    }
  }
  if constexpr (EPC > 1) { // the n % EPC elements behind the last whole chunk
    const uint64_t e = chunks * EPC + tid;
    if (e < n) {
      const typename S::bits b = load_chunk<typename S::bits, true>((uint64_t)src + e * sizeof(typename S::bits));
      store_chunk<typename D::bits, true>((uint64_t)out + e * sizeof(typename D::bits), D::one(S::to_f32(b)));
    }
  }
}

// ---- Q8ROW -------------------------------------------------------------------------------------------------------------
constexpr int kRegElems = 16;      // row values a lane keeps between the reduction and the encode
constexpr size_t kRegDim = 1024;   // 64 lanes x kRegElems: the longest row k_q8row_rows holds in registers

// Finite f32 bits as unsigned keys in the order of their values, -0 below +0: min and max are integer operations, and
// the minimum of a row whose smallest values are zeros of both signs is -0.0 whatever order the lanes meet them in
// (numpy's min leaves that sign to the order of its reduction).
__device__ __forceinline__ uint32_t order_key(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key_value(uint32_t k) {
  return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k);
}

struct RowRange { // what a lane has seen of its row; `all` folds two lanes' views
  uint32_t kmin = 0xffffffffu, kmax = 0u, bad = 0u;
  __device__ __forceinline__ void see(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f), k = order_key(u);
    bad |= (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; // NaN or +-inf
    kmin = k < kmin ? k : kmin;
    kmax = k > kmax ? k : kmax;
  }
  // across the `group` lanes (a power of two) that share the row: butterfly, every lane ends with the row's range
  __device__ __forceinline__ void all(uint32_t group) {
    for (uint32_t off = 1; off < group; off <<= 1) {
      const uint32_t a = __shfl_xor(kmin, (int)off, 64), b = __shfl_xor(kmax, (int)off, 64), c = __shfl_xor(bad, (int)off, 64);
      kmin = a < kmin ? a : kmin;
      kmax = b > kmax ? b : kmax;
      bad |= c;
    }
  }
};

// quantize_q8row's arithmetic (xgnn_amd/datagen.py), float64: scale = f32((hi - lo) / 255), code = clip(rint((x - lo) /
// scale), 0, 255), every code 0 when the f32 scale is 0; bias = lo.  `/` on doubles is correctly rounded, rint is
// round-half-even, and the f64 -> f32 cast of the scale keeps subnormals.  Nothing here is a multiply-add, and nothing
// may become one.
struct RowScale {
  double lo, scale;
  uint32_t scale_bits, bias_bits;
  bool zero; // bad row or scale 0: every code is 0
  __device__ __forceinline__ RowScale(const RowRange &r) {
#pragma clang fp contract(off)
    const float flo = key_value(r.kmin), fhi = key_value(r.kmax);
    lo = (double)flo;
    const float s = (float)(((double)fhi - lo) / 255.0);
    scale = (double)s;
    zero = r.bad || !(s > 0.0f);
    scale_bits = r.bad ? 0u : __builtin_bit_cast(uint32_t, s);
    bias_bits = r.bad ? 0u : __builtin_bit_cast(uint32_t, flo);
  }
  __device__ __forceinline__ uint8_t code(float x) const {
#pragma clang fp contract(off)
    const double q = __builtin_rint(((double)x - lo) / scale);
    const double c = q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q);
    return zero ? (uint8_t)0 : (uint8_t)(uint32_t)c;
  }
};

// the row's tail, by one lane: zero pad up to the trailer, {scale, bias}, and a bad row's report
__device__ __forceinline__ void q8row_finish(uint64_t out_row, uint32_t dim, const RowScale &rs, bool bad, uint64_t row_id,
                                             unsigned long long *bad_row) {
  const uint32_t trailer = (uint32_t)q8row_trailer_offset(dim);
  for (uint32_t i = dim; i < trailer; ++i) store_chunk<uint8_t, true>(out_row + i, (uint8_t)0);
  store_chunk<u32x2_t, true>(out_row + trailer, u32x2_t{rs.scale_bits, rs.bias_bits});
  if (bad && bad_row) atomicMin(bad_row, (unsigned long long)row_id);
}

template <int SRC_DT, int V>
__device__ __forceinline__ void q8row_store_codes(uint64_t addr, const float *x, const RowScale &rs) {
  using CV = typename VecT<uint8_t, V>::type;
  CV codes;
#pragma unroll
  for (int e = 0; e < V; ++e) vec_set<CV, V>(codes, e, rs.code(x[e]));
  store_chunk<CV, true>(addr, codes);
}

// rows of at most kRegDim elements: `1 << group_log2` lanes per row, the row in registers.  V = elements per load.
template <int SRC_DT, int V>
__global__ __launch_bounds__(kBlock) void k_q8row_rows(char *__restrict__ out, const char *__restrict__ src, uint64_t num_rows,
                                                       uint32_t dim, uint32_t group_log2, uint64_t first_row,
                                                       unsigned long long *bad_row) {
  using S = Elem<SRC_DT>;
  using SV = typename VecT<typename S::bits, V>::type;
  constexpr int P = kRegElems / V; // chunks per lane at most
  constexpr uint64_t ES = sizeof(typename S::bits);
  const uint32_t group = 1u << group_log2, lane = lane_id(), j = lane & (group - 1u), sub = lane >> group_log2;
  const uint32_t rows_per_wave = (uint32_t)kWave >> group_log2;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, num_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t chunks = dim / V; // whole: V divides dim
  const uint64_t out_stride = q8row_stride(dim);
  for (uint64_t r0 = wave * rows_per_wave; r0 < num_rows; r0 += num_waves * rows_per_wave) { // uniform per wave
    const uint64_t row = r0 + sub;
    const bool live = row < num_rows;
    const uint64_t src_row = (uint64_t)src + row * dim * ES, out_row = (uint64_t)out + row * out_stride;
    float x[P * V];
    RowRange range;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if ((uint32_t)p * group >= chunks) break; // uniform
      const uint32_t c = (uint32_t)p * group + j;
      if (live && c < chunks) {
        const SV v = load_chunk<SV, true>(src_row + (uint64_t)c * V * ES);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          x[p * V + e] = S::to_f32(vec_get<SV, V>(v, e));
          range.see(x[p * V + e]);
        }
      }
    }
    range.all(group);
    const RowScale rs(range);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if ((uint32_t)p * group >= chunks) break;
      const uint32_t c = (uint32_t)p * group + j;
      if (live && c < chunks) q8row_store_codes<SRC_DT, V>(out_row + (uint64_t)c * V, &x[p * V], rs);
    }
    if (live && j == 0) q8row_finish(out_row, dim, rs, range.bad != 0, first_row + row, bad_row);
  }
}

// longer rows: one wave per row, read once for the range and once more for the codes
template <int SRC_DT, int V>
__global__ __launch_bounds__(kBlock) void k_q8row_long(char *__restrict__ out, const char *__restrict__ src, uint64_t num_rows,
                                                       uint32_t dim, uint64_t first_row, unsigned long long *bad_row) {
  using S = Elem<SRC_DT>;
  using SV = typename VecT<typename S::bits, V>::type;
  constexpr uint64_t ES = sizeof(typename S::bits);
  const uint32_t lane = lane_id();
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, num_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t chunks = dim / V;
  const uint64_t out_stride = q8row_stride(dim);
  for (uint64_t row = wave; row < num_rows; row += num_waves) {
    const uint64_t src_row = (uint64_t)src + row * dim * ES, out_row = (uint64_t)out + row * out_stride;
    RowRange range;
    for (uint32_t c = lane; c < chunks; c += kWave) {
      const SV v = load_chunk<SV, true>(src_row + (uint64_t)c * V * ES);
#pragma unroll
      for (int e = 0; e < V; ++e) range.see(S::to_f32(vec_get<SV, V>(v, e)));
    }
    range.all(kWave);
    const RowScale rs(range);
    for (uint32_t c = lane; c < chunks; c += kWave) {
      const SV v = load_chunk<SV, false>(src_row + (uint64_t)c * V * ES); // the second read: may still be in cache
      float x[V];
#pragma unroll
      for (int e = 0; e < V; ++e) x[e] = S::to_f32(vec_get<SV, V>(v, e));
      q8row_store_codes<SRC_DT, V>(out_row + (uint64_t)c * V, x, rs);
    }
    if (lane == 0) q8row_finish(out_row, dim, rs, range.bad != 0, first_row + row, bad_row);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <int SRC_DT, int DST_DT>
static int launch_encode(char *out, const char *src, uint64_t n, hipStream_t stream) {
  constexpr size_t SES = sizeof(typename Elem<SRC_DT>::bits), DES = sizeof(typename Encode<DST_DT>::bits);
  const int epc = pick_chunk(0, (int)(16 / SES), SES, (uintptr_t)src, DES, (uintptr_t)out); // flat: whole chunks, then single elements
  const int grid = grid_for(n / epc + 1, (size_t)kBlock * kElemU);
#define GGMS_EPC(E)                                                                                                   \
  case E:                                                                                                            \
    hipLaunchKernelGGL((k_encode_elems<SRC_DT, DST_DT, E>), dim3(grid), dim3(kBlock), 0, stream, out, src, n);       \
    break;
  switch (epc) {
    GGMS_EPC(1)
    GGMS_EPC(2)
    GGMS_EPC(4)
    default:
      if constexpr (SES == 2) hipLaunchKernelGGL((k_encode_elems<SRC_DT, DST_DT, 8>), dim3(grid), dim3(kBlock), 0, stream, out, src, n);
  }
#undef GGMS_EPC
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

template <int SRC_DT, int V>
static int launch_q8row_v(char *out, const char *src, size_t num_rows, size_t dim, uint64_t first_row,
                          unsigned long long *bad_row, hipStream_t stream) {
  if (dim > kRegDim) {
    hipLaunchKernelGGL((k_q8row_long<SRC_DT, V>), dim3(grid_for(num_rows, kBlock / kWave)), dim3(kBlock), 0, stream, out, src,
                       (uint64_t)num_rows, (uint32_t)dim, first_row, bad_row);
  } else {
    uint32_t group_log2 = 0; // the smallest group that has a lane for every chunk, 64 lanes at most
    while (group_log2 < 6 && ((size_t)1 << group_log2) < dim / V) ++group_log2;
    const size_t rows_per_block = (size_t)(kBlock / kWave) * ((size_t)kWave >> group_log2);
    hipLaunchKernelGGL((k_q8row_rows<SRC_DT, V>), dim3(grid_for(num_rows, rows_per_block)), dim3(kBlock), 0, stream, out, src,
                       (uint64_t)num_rows, (uint32_t)dim, group_log2, first_row, bad_row);
  }
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

template <int SRC_DT>
static int launch_q8row(char *out, const char *src, size_t num_rows, size_t dim, uint64_t first_row,
                        unsigned long long *bad_row, hipStream_t stream) {
  constexpr size_t SES = sizeof(typename Elem<SRC_DT>::bits);
  // every row starts dim x SES bytes after the last: a chunk width must divide dim and suit the base.  The codes'
  // side follows: `out` and the row stride are multiples of 8, a chunk of V codes starts at a multiple of V.
  switch (pick_chunk(dim, (int)(16 / SES), SES, (uintptr_t)src, 1, 0)) {
    case 1: return launch_q8row_v<SRC_DT, 1>(out, src, num_rows, dim, first_row, bad_row, stream);
    case 2: return launch_q8row_v<SRC_DT, 2>(out, src, num_rows, dim, first_row, bad_row, stream);
    case 4: return launch_q8row_v<SRC_DT, 4>(out, src, num_rows, dim, first_row, bad_row, stream);
    default:
      if constexpr (SES == 2) return launch_q8row_v<SRC_DT, 8>(out, src, num_rows, dim, first_row, bad_row, stream);
  }
  return GGMS_ERR_INVALID;
}

} // namespace ggms

using namespace ggms;

extern "C" int ggms_quantize_rows(void *out, int out_dtype, const void *src, int src_dtype, size_t num_rows, size_t dim,
                                  uint64_t first_row, uint64_t *bad_row, ggms_stream_t stream) {
  if (!quantiser_reads(src_dtype) || !quantiser_writes(out_dtype) || src_dtype == out_dtype || dim == 0) {
    set_error("quantize_rows: invalid argument: dtype %d -> %d, dim %zu (the source is F32 or F16, the output another "
              "type of F16, BF16, F8E4M3, F8E5M2 and Q8ROW; rows are not empty)", src_dtype, out_dtype, dim);
    return GGMS_ERR_INVALID;
  }
  if (num_rows == 0) return GGMS_OK;
  GGMS_CHECK_ARG(out && src);
  GGMS_CHECK_ARG(dim < (1ull << 32));
  const size_t out_align = out_dtype == GGMS_Q8ROW ? 8 : ggms_dtype_bytes(out_dtype);
  if ((uintptr_t)src % 4 != 0 || (uintptr_t)out % out_align != 0) {
    set_error("quantize_rows: invalid argument: src must be 4-byte aligned and out %zu-byte aligned for dtype %d (a Q8ROW "
              "row ends in an 8-byte scale / bias trailer, written by one store)", out_align, out_dtype);
    return GGMS_ERR_INVALID;
  }
  char *o = (char *)out;
  const char *s = (const char *)src;
  hipStream_t st = to_stream(stream);
  if (out_dtype == GGMS_Q8ROW) {
    unsigned long long *bad = (unsigned long long *)bad_row;
    return src_dtype == GGMS_F32 ? launch_q8row<GGMS_F32>(o, s, num_rows, dim, first_row, bad, st)
                                 : launch_q8row<GGMS_F16>(o, s, num_rows, dim, first_row, bad, st);
  }
  const uint64_t n = (uint64_t)num_rows * dim;
#define GGMS_PAIR(S, D) \
  if (src_dtype == S && out_dtype == D) return launch_encode<S, D>(o, s, n, st);
  GGMS_PAIR(GGMS_F32, GGMS_F16)
  GGMS_PAIR(GGMS_F32, GGMS_BF16)
  GGMS_PAIR(GGMS_F32, GGMS_F8E4M3)
  GGMS_PAIR(GGMS_F32, GGMS_F8E5M2)
  GGMS_PAIR(GGMS_F16, GGMS_BF16)
  GGMS_PAIR(GGMS_F16, GGMS_F8E4M3)
  GGMS_PAIR(GGMS_F16, GGMS_F8E5M2)
#undef GGMS_PAIR
  set_error("quantize_rows: no encoder from dtype %d to dtype %d", src_dtype, out_dtype);
  return GGMS_ERR_INVALID;
}
