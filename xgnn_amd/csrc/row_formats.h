// row_formats.h -- what a stored feature row looks like, for both sides of it: the row gather (extract.hip) reads
// and decodes what the row quantiser (quantize.hip) writes, so the encoder rounds exactly as the gather narrows because
// both use the definitions below.  Element types by ggms_dtype code, the register vectors and streaming accessors
// that move them, the GGMS_Q8ROW and GGMS_MXFP4 row layouts (with MXFP4's decode and rounding), the chunk-width rule, and which dtype may stand on which side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ggms.h"
#include "fp8_decode.h"

namespace ggms {

// ---- which dtype may stand where --------------------------------------------------------------------------------------
// what the converting gather delivers (and reads)
constexpr bool is_float_dtype(int dt) { return dt == GGMS_F16 || dt == GGMS_BF16 || dt == GGMS_F32; }
// the OCP 8-bit floats: decoded by the gather, written by the quantiser, never delivered
constexpr bool is_fp8_dtype(int dt) { return dt == GGMS_F8E4M3 || dt == GGMS_F8E5M2; }
// the ROW formats: codes with per-row (Q8ROW) or per-block (MXFP4) scales, no element size, decoded by the gather only
constexpr bool is_row_format(int dt) { return dt == GGMS_Q8ROW || dt == GGMS_MXFP4; }
// every table type the converting gather reads
constexpr bool gather_converts_from(int dt) { return is_float_dtype(dt) || is_fp8_dtype(dt) || is_row_format(dt); }
constexpr bool quantiser_reads(int dt) { return dt == GGMS_F32 || dt == GGMS_F16; }
constexpr bool quantiser_writes(int dt) { return dt == GGMS_F16 || dt == GGMS_BF16 || is_fp8_dtype(dt) || is_row_format(dt); }

// ---- elements -----------------------------------------------------------------------------------------------------------
// element types by ggms_dtype code: the bits as stored, and the value as f32 (every conversion goes through f32)
template <int DT> struct Elem;
template <> struct Elem<GGMS_F32> {
  using bits = uint32_t;
  static __device__ __forceinline__ float to_f32(bits b) { return __builtin_bit_cast(float, b); }
  static __device__ __forceinline__ bits from_f32(float f) { return __builtin_bit_cast(bits, f); }
};
template <> struct Elem<GGMS_F16> { // the casts are IEEE: widening exact (subnormals included), narrowing
  using bits = uint16_t;            // round-to-nearest-even with overflow to inf and subnormal results kept
  static __device__ __forceinline__ float to_f32(bits b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ bits from_f32(float f) { return __builtin_bit_cast(bits, (_Float16)f); }
};
template <> struct Elem<GGMS_BF16> { // the upper half of an f32
  using bits = uint16_t;
  static __device__ __forceinline__ float to_f32(bits b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
  static __device__ __forceinline__ bits from_f32(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bits)((u >> 16) | 0x40u); // NaN stays NaN (quiet)
    return (bits)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); // nearest even; a carry out of the mantissa ends in inf
  }
};
// the OCP 8-bit floats (fp8_decode.h): SOURCE types only -- no from_f32, so no pair with one of them as output exists
template <> struct Elem<GGMS_F8E4M3> {
  using bits = uint8_t;
  static __device__ __forceinline__ float to_f32(bits b) { return fp8_e4m3_to_f32(b); }
};
template <> struct Elem<GGMS_F8E5M2> {
  using bits = uint8_t;
  static __device__ __forceinline__ float to_f32(bits b) { return fp8_e5m2_to_f32(b); }
};
// N elements of T as one register vector (one load or store instruction); a vector of 1 is the scalar itself
template <typename T, int N> struct VecT { typedef T type __attribute__((ext_vector_type(N))); };
template <typename T> struct VecT<T, 1> { using type = T; };
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

template <typename VT, int N> __device__ __forceinline__ auto vec_get(const VT &v, int e) {
  if constexpr (N == 1) return v;
  else return v[e];
}
template <typename VT, int N, typename T> __device__ __forceinline__ void vec_set(VT &v, int e, T x) {
  if constexpr (N == 1) v = x;
  else v[e] = x;
}

// ---- streaming accessors ------------------------------------------------------------------------------------------------
// chunk loads and stores: plain or non-temporal (a batch's rows, and a table being encoded, are read once)
// The gather's pointers travel through ds_bpermute as integers; tell the compiler they are GLOBAL so it emits
// global_load/global_store (vmcnt only) instead of flat_* (vmcnt + lgkmcnt, aperture check).
template <typename V, bool NT>
__device__ __forceinline__ V load_chunk(uint64_t addr) {
  typedef const V __attribute__((address_space(1))) *gp_t;
  gp_t p = (gp_t)addr;
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <typename V, bool NT>
__device__ __forceinline__ void store_chunk(uint64_t addr, V v) {
  typedef V __attribute__((address_space(1))) *gp_t;
  if constexpr (NT) __builtin_nontemporal_store(v, (gp_t)addr);
  else *(gp_t)addr = v;
}

// ---- the GGMS_Q8ROW row (include/ggms.h) --------------------------------------------------------------------------------
// `dim` one-byte codes, zero bytes up to the next multiple of 8, then the row's f32 scale and f32 bias: where the
// 8-byte trailer of a row of `dim` codes lies, and the distance from one such row to the next
__host__ __device__ constexpr uint64_t q8row_trailer_offset(uint64_t dim) { return (dim + 7u) & ~(uint64_t)7u; }
__host__ __device__ constexpr uint64_t q8row_stride(uint64_t dim) { return q8row_trailer_offset(dim) + 8u; }

// ---- the GGMS_MXFP4 row (include/ggms.h) --------------------------------------------------------------------------------
// nb = ceil(dim / 32) blocks of 16 code bytes (two E2M1 nibbles a byte, low nibble first), then nb E8M0 scale bytes,
// then zero bytes up to a multiple of 8.  dim is even: no byte is shared between two elements' owners.
constexpr uint32_t kMxBlock = 32;            // elements per scale
constexpr uint32_t kMxScaleMin = 2, kMxScaleMax = 252; // the scale bytes the encoder writes (every product a normal f32)
__host__ __device__ constexpr uint64_t mxfp4_blocks(uint64_t dim) { return (dim + kMxBlock - 1) / kMxBlock; }
__host__ __device__ constexpr uint64_t mxfp4_scale_offset(uint64_t dim) { return 16u * mxfp4_blocks(dim); }
__host__ __device__ constexpr uint64_t mxfp4_stride(uint64_t dim) { return (17u * mxfp4_blocks(dim) + 7u) & ~(uint64_t)7u; }

// The f32 bits of E2M1 code `c` (sign in bit 3, magnitude index m in bits 2..0: 0, 0.5, 1, 1.5, 2, 3, 4, 6) times
// 2^(x - 127).  m >= 2 is 2^(e - 1) x (1 + man / 2) with m = 2e + man: exponent field x + e - 1, mantissa man << 22,
// which is ((x - 1) << 23) + (m << 22) -- a shift and an add; 0.5 is the bare 2^(x - 128), 0 is 0.  x = 255: NaN.
__host__ __device__ __forceinline__ uint32_t mxfp4_f32_bits(uint32_t c, uint32_t x) {
  const uint32_t m = c & 7u, base = (x - 1u) << 23;
  const uint32_t mag = m >= 2u ? base + (m << 22) : (m ? base : 0u);
  return x == 255u ? 0x7fc00000u : (mag | ((c & 8u) << 28));
}

// The scale byte of a block whose largest magnitude has the f32 bits `amax_bits` (finite): OCP's floor(log2(amax)) -
// emax_elem read from the exponent field, clamped to the bytes whose products are normal f32 (amax 0 or subnormal: 2).
__host__ __device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t amax_bits) {
  const int32_t x = (int32_t)(amax_bits >> 23) - 2;
  return (uint32_t)(x < (int32_t)kMxScaleMin ? (int32_t)kMxScaleMin : (x > (int32_t)kMxScaleMax ? (int32_t)kMxScaleMax : x));
}

// The E2M1 code of a finite f32 for scale byte x in [kMxScaleMin, kMxScaleMax]: s = |v| x 2^(127 - x) (an exact
// scaling; what underflows is far below 0.25 and rounds to 0 either way) rounded to the nearest magnitude, ties to the
// code with an even low bit, above 6 saturated, the sign kept.  The magnitudes are a grid of step 0.5 below 2, 1 below
// 4 and 2 above: adding 2^(22 + ec), ec = clamp(floor(log2 s), 0, 2), rounds s to its grid in the f32 adder -- nearest,
// ties to the even multiple of the step -- and leaves the multiple k in the low mantissa bits; the code's magnitude
// index is k + 2 ec, whose low bit is k's (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4).
__host__ __device__ __forceinline__ uint32_t mxfp4_code(float v, uint32_t x) {
  const uint32_t vb = __builtin_bit_cast(uint32_t, v);
  float s = __builtin_fabsf(v) * __builtin_bit_cast(float, (254u - x) << 23);
  s = s < 8.0f ? s : 8.0f; // (beyond 8 only for an x below the block's own: saturates all the same)
  const int32_t e = (int32_t)(__builtin_bit_cast(uint32_t, s) >> 23) - 127;
  const uint32_t ec = (uint32_t)(e < 0 ? 0 : (e > 2 ? 2 : e));
  const uint32_t magic = (149u + ec) << 23;
  const uint32_t m = __builtin_bit_cast(uint32_t, s + __builtin_bit_cast(float, magic)) - magic + 2u * ec;
  return ((vb >> 28) & 8u) | (m > 7u ? 7u : m);
}

// ---- chunk width --------------------------------------------------------------------------------------------------------
// The widest chunk, in ELEMENTS (a power of two up to max_epc), that divides a row of `dim` elements and keeps both
// sides aligned to their own chunk size: epc x src_es bytes for every source base, epc x dst_es bytes for `out`
// (*_bits: the addresses ORed together).  dim 0: a flat array with no row ends, any width divides it.
static inline int pick_chunk(size_t dim, int max_epc, size_t src_es, uintptr_t src_bits, size_t dst_es, uintptr_t dst_bits) {
  for (int epc = max_epc; epc > 1; epc >>= 1)
    if (dim % epc == 0 && src_bits % (epc * src_es) == 0 && dst_bits % (epc * dst_es) == 0) return epc;
  return 1;
}
// the plain gather: rows of bytes, chunks of up to 16 of them
static inline int pick_chunk(size_t row_bytes, uintptr_t align_bits) {
  return pick_chunk(row_bytes, 16, 1, align_bits, 1, align_bits);
}

} // namespace ggms
