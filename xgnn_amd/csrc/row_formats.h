// row_formats.h -- what a stored feature row looks like, for both sides of it: the row gather (extract.hip) reads
// and decodes what the row quantiser (quantize.hip) writes, so the encoder rounds exactly as the gather narrows because
// both use the definitions below.  Element types by ggms_dtype code, the register vectors and streaming accessors
// that move them, the GGMS_Q8ROW row layout, the chunk-width rule, and which dtype may stand on which side.
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
// every table type the converting gather reads
constexpr bool gather_converts_from(int dt) { return is_float_dtype(dt) || is_fp8_dtype(dt) || dt == GGMS_Q8ROW; }
constexpr bool quantiser_reads(int dt) { return dt == GGMS_F32 || dt == GGMS_F16; }
constexpr bool quantiser_writes(int dt) { return dt == GGMS_F16 || dt == GGMS_BF16 || is_fp8_dtype(dt) || dt == GGMS_Q8ROW; }

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
