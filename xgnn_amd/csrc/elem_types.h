// elem_types.h -- the element types of a feature table by ggms_dtype code, for the row quantiser (quantize.hip).
// The same definitions, token for token, as the converting gather keeps in extract.hip (which defines its own and
// does not include this header): the encoder rounds exactly as the gather narrows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ggms.h"
#include "fp8_decode.h"

namespace ggms {

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
// N elements of T as one register vector (one load or store instruction)
template <typename T, int N> struct VecT { typedef T type __attribute__((ext_vector_type(N))); };
template <typename T> struct VecT<T, 1> { using type = T; };

} // namespace ggms
