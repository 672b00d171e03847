// fp8_decode.h -- the two OCP 8-bit float formats as SOURCE element types of the converting gather (extract.hip).
//
//   E4M3 ("fn"): 1-4-3, bias 7, no infinities, NaN = 0x7f / 0xff, largest finite 448
//   E5M2:        1-5-2, bias 15, IEEE-like: 0x7c / 0xfc are +-inf, 0x7d..0x7f / 0xfd..0xff NaN
// (not the FNUZ variants: those have another bias and a single NaN at 0x80).
//
// Every finite code of either format is exactly representable in f16, bf16 and f32, so decoding has no rounding mode;
// both routes below go through the f16 that holds the code's bits and the exact f16 -> f32 cast (subnormals included).
// Decode only: an FP8 dtype is never the output of a conversion.
#ifndef GGMS_FP8_DECODE_H
#define GGMS_FP8_DECODE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GGMS_FP8_FN __host__ __device__ __forceinline__
#else
#define GGMS_FP8_FN inline
#endif

namespace ggms {

// E5M2 is the upper byte of the f16 of the same value, inf and NaN included.
GGMS_FP8_FN float fp8_e5m2_to_f32(uint8_t b) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)((uint16_t)b << 8));
}

// E4M3: exponent and mantissa moved into an f16's fields hold the value x 2^-8 (the biases differ by 8; a subnormal
// code becomes an f16 subnormal of the same scale), widened and multiplied by 256 -- exact.  The all-ones pattern is
// NaN, which the shift alone would turn into +-480.
GGMS_FP8_FN float fp8_e4m3_to_f32(uint8_t b) {
  const uint16_t h = (uint16_t)(((uint16_t)(b & 0x80u) << 8) | ((uint16_t)(b & 0x7fu) << 7));
  const float f = (float)__builtin_bit_cast(_Float16, h) * 256.0f;
  const uint32_t nan = 0x7fc00000u | ((uint32_t)(b & 0x80u) << 24); // quiet NaN of the code's sign
  return (b & 0x7fu) == 0x7fu ? __builtin_bit_cast(float, nan) : f;
}

} // namespace ggms

#endif // GGMS_FP8_DECODE_H
