// row_chunks.h -- what a gather's chunk is: the unit the row sweeps of extract.hip and gather_typed.hip move.  One set
// of definitions, so that every gather copies and converts with the same bits.
#pragma once
#include "row_formats.h"

namespace ggms {

template <int BYTES> struct ChunkT;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
template <> struct ChunkT<16> { using type = u32x4_t; };
template <> struct ChunkT<8> { using type = u32x2_t; };
template <> struct ChunkT<4> { using type = uint32_t; };
template <> struct ChunkT<2> { using type = uint16_t; };
template <> struct ChunkT<1> { using type = uint8_t; };

// ---- what a chunk is ----------------------------------------------------------------------------------------------
// The sweep moves CHUNKS: a fixed number of elements of a row, read as Src and written as Dst.  The plain gather's
// chunk is CB bytes on both sides.  A converting gather (ggms_*_convert: an F16 / BF16 / F32 table delivered in
// another of the three types, or an FP8 table delivered in one of them) has chunks of EPC elements: EPC x source element bytes in, EPC x output element bytes
// out, converted at store time -- the registers a lane holds between its loads and its first store are the SOURCE
// chunks only, whichever side is the wider one.
template <int CB> struct CopyChunk {
  static constexpr bool kScaled = false; // (ScaledChunk below)
  static constexpr int kSrcBytes = CB, kDstBytes = CB;
  using Src = typename ChunkT<CB>::type;
  using Dst = Src;
  static __device__ __forceinline__ Dst convert(Src v) { return v; }
};

template <int EPC, int SRC_DT, int DST_DT> struct ConvertChunk {
  using S = Elem<SRC_DT>;
  using D = Elem<DST_DT>;
  static constexpr bool kScaled = false;
  static constexpr int kSrcBytes = EPC * (int)sizeof(typename S::bits), kDstBytes = EPC * (int)sizeof(typename D::bits);
  using Src = typename VecT<typename S::bits, EPC>::type;
  using Dst = typename VecT<typename D::bits, EPC>::type;
  // every FP8 value is a bf16 number (at most 3 mantissa bits): the upper half of its f32, no rounding step
  static constexpr bool kTruncates = (SRC_DT == GGMS_F8E4M3 || SRC_DT == GGMS_F8E5M2) && DST_DT == GGMS_BF16;
  static __device__ __forceinline__ typename D::bits one(typename S::bits b) {
    if constexpr (kTruncates) return (typename D::bits)(__builtin_bit_cast(uint32_t, S::to_f32(b)) >> 16);
    else return D::from_f32(S::to_f32(b));
  }
  static __device__ __forceinline__ Dst convert(Src v) {
    if constexpr (EPC == 1) {
      return one(v);
    } else {
      Dst o;
#pragma unroll
      for (int e = 0; e < EPC; ++e) o[e] = one(v[e]);
      return o;
    }
  }
};

// A row-scaled 8-bit table (GGMS_Q8ROW, include/ggms.h): a row is `dim` unsigned codes, zero bytes up to the next
// multiple of 8, then the row's f32 scale and f32 bias.  The chunk is EPC code bytes; its value needs the two numbers
// that belong to the ROW, so convert takes them beside the chunk's bits: the sweep loads a row's 8-byte trailer with
// the row's pointer (the lane that resolves the row keeps both) and hands scale and bias to the chunk's lane the way
// it hands out the pointer.  value = fl32(fl32(float(code) * scale) + bias), two IEEE operations: NOT an FMA, whose
// single rounding gives other bits (hipcc contracts a * b + c by default, through __fmul_rn / __fadd_rn too, which
// are plain operators in its headers; the pragma takes the licence away for these two operations).
template <int EPC, int DST_DT> struct ScaledChunk {
  using D = Elem<DST_DT>;
  static constexpr bool kScaled = true;
  static constexpr int kSrcBytes = EPC, kDstBytes = EPC * (int)sizeof(typename D::bits);
  using Src = typename VecT<uint8_t, EPC>::type;
  using Dst = typename VecT<typename D::bits, EPC>::type;
  static __device__ __forceinline__ typename D::bits one(uint8_t code, float scale, float bias) {
#pragma clang fp contract(off)
    const float scaled = (float)code * scale;
    const float value = scaled + bias;
    return D::from_f32(value);
  }
  static __device__ __forceinline__ Dst convert(Src v, uint32_t scale_bits, uint32_t bias_bits) {
    const float scale = __builtin_bit_cast(float, scale_bits), bias = __builtin_bit_cast(float, bias_bits);
    if constexpr (EPC == 1) {
      return one(v, scale, bias);
    } else {
      Dst o;
#pragma unroll
      for (int e = 0; e < EPC; ++e) o[e] = one(v[e], scale, bias);
      return o;
    }
  }
};

// A chunk's wider side is at most 16 bytes (one load or store instruction per chunk and side, consecutive lanes on
// consecutive addresses): 8 elements between the 16-bit types, 4 when one side is f32.  Measured against 8-element
// chunks for those (a 16-B load with two 16-B stores, two 16-B loads with a 16-B store): profiles/feat_convert_ab.txt.
// An FP8 source follows the same rule: 8 elements into a 16-bit type (8-B load, 16-B store), 4 into f32 (4-B load,
// 16-B store); profiles/fp8_table_ab.txt.
constexpr int convert_max_epc(size_t src_es, size_t dst_es) { return (int)(16 / (src_es > dst_es ? src_es : dst_es)); }

} // namespace ggms
