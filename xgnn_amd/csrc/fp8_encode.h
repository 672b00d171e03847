// fp8_encode.h -- f32 -> the two OCP 8-bit float formats of fp8_decode.h, as OUTPUT element types of the row quantiser
// (quantize.hip).  Round to nearest even on the f32's bits; the result is torch's CPU cast bit for bit:
//   E4M3: v.clamp(-448, 448).to(torch.float8_e4m3fn) -- the format has no infinity, so the clamp comes FIRST and
//         +-inf and everything beyond +-448 saturate; NaN stays NaN (0x7f with the sign);
//   E5M2: v.to(torch.float8_e5m2) -- overflow (|v| >= 61440, the tie included) gives +-inf, NaN gives 0x7f with the sign.
// -0 keeps its sign, subnormal codes are produced.
//
// Normal results: add half of the last kept bit (less one, plus the kept bit's parity: nearest even) to the magnitude's
// bits and shift; a carry out of the mantissa moves into the exponent field, which is what rounding up to the next
// binade is.  Subnormal results (below the format's smallest normal): the code is the magnitude in units of the
// subnormal step, rounded to nearest even by ONE f32 addition to the power of two whose ulp is that step.
#ifndef GGMS_FP8_ENCODE_H
#define GGMS_FP8_ENCODE_H

#include "fp8_decode.h"

namespace ggms {

// MANT: mantissa bits of the format, BIAS: its exponent bias; `a` is the magnitude's f32 bits, finite and below the
// format's overflow threshold (or, E5M2, anything up to inf: the caller caps the result)
template <int MANT, int BIAS>
GGMS_FP8_FN uint32_t fp8_round_magnitude(uint32_t a) {
  constexpr int kDrop = 23 - MANT;                          // f32 mantissa bits that go
  constexpr uint32_t kMinNormal = (uint32_t)(127 - BIAS + 1) << 23; // 2^(1 - BIAS)
  if (a < kMinNormal) {
    // step 2^(1 - BIAS - MANT); 2^(1 - BIAS - MANT + 23) has that ulp, and the sum stays in its binade (a < 2^(1-BIAS))
    constexpr uint32_t kMagic = (uint32_t)(127 + 1 - BIAS - MANT + 23) << 23;
    const float sum = __builtin_bit_cast(float, a) + __builtin_bit_cast(float, kMagic);
    return __builtin_bit_cast(uint32_t, sum) - kMagic; // 0 .. 2^MANT: the last one IS the smallest normal's code
  }
  const uint32_t r = a + ((1u << (kDrop - 1)) - 1u) + ((a >> kDrop) & 1u);
  return (r >> kDrop) - ((uint32_t)(127 - BIAS) << MANT);
}

GGMS_FP8_FN uint8_t f32_to_fp8_e5m2(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu); // NaN
  const uint32_t m = fp8_round_magnitude<2, 15>(a);
  return (uint8_t)(sign | (m > 0x7cu ? 0x7cu : m)); // everything from 61440 up, inf included: inf
}

GGMS_FP8_FN uint8_t f32_to_fp8_e4m3(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu); // NaN
  if (a > 0x43e00000u) a = 0x43e00000u;                // clamp to 448 = 1.75 x 2^8 (code 0x7e)
  return (uint8_t)(sign | fp8_round_magnitude<3, 7>(a));
}

} // namespace ggms

#endif // GGMS_FP8_ENCODE_H
