// sample_typed.hip -- khop_typed: a fanout per edge type on a type-sorted CSR (include/ggms.h).
//
// Every edge position p of the CSR carries a type edge_type[p] < R; inside a node's list the types are non-decreasing,
// so "the edges of type r" are one contiguous SEGMENT of the list: [b_r, b_{r+1}), b_r = the number of entries with a
// type below r.  A seed is sampled segment by segment: khop_labor's rule on segment r with fanout k_r (labor_select.h:
// the min(k_r, e_r) smallest keys (fmix32(t_p ^ salt) << 32) | p), every segment under the SAME salt -- the variate
// belongs to the node, a node picked under two relations is one row of the batch.  Every edge leaves with its CSR
// position and its type: two relations between the same pair of nodes are two positions.
//
// One layer = a 4-byte memset and four launches (+ the scan's own):
//   k_typed_bounds  a GROUP of G = 2^ceil(log2 R) lanes per seed; lane r finds b_{r+1} by a lower-bound search over the
//                   byte array.  The R - 1 searches of a seed are independent chains of dependent one-byte loads: side
//                   by side they cost log2(d) rounds whatever R is.  Two one-load exits first (type[last] <= r:
//                   b = d; type[first] > r: b = 0), which settle every lane of a one-relation list.  The boundaries
//                   are made monotone by a prefix maximum over the group (a list that is not sorted gets SOME
//                   partition of [0, d]: nothing is read outside the list), written as R words per seed (b_0 = 0 is not
//                   stored), and the group sums the seed's count, sum_r min(k_r, e_r).
//   tile_scan       offset[i] = the sum of the counts of the seeds before i; *num_out = the edge count.  n items, not
//                   n x R.
//   k_typed_select  one WAVE per seed; a seed whose count is 0 costs one 4-byte load.  Else the seed's boundaries are one
//                   coalesced load (lane r holds b_{r+1}) and the wave walks the types with a running offset, routing
//                   every segment by ITS length e_r (not by the degree: 3 edges of a rare relation in a 40 000-entry
//                   hub are a copy): e_r <= k_r a contiguous copy, else labor_wave_select<1 / 4 / 16> up to
//                   kLaborWave1 / 4 / Max.  A seed with a longer segment is listed for
//   k_typed_hub     one WORKGROUP per listed seed: it walks the types again and runs labor_hub_list on the long
//                   segments.  (The list holds seeds, n words, not (seed, type) pairs, n x R: a hub with several long
//                   relations has them done one after the other by its workgroup.)
// The type fanouts travel to the kernels by value, a byte each in eight words of the arguments.
#include "ggms_internal.h"
#include "labor_select.h"
#include "tile_scan.h"

namespace ggms {

// k_r, r < GGMS_MAX_EDGE_TYPES, one byte each
struct TypeFanouts {
  uint32_t w[GGMS_MAX_EDGE_TYPES / 4];
  __device__ __forceinline__ uint32_t get(uint32_t r) const {
    uint32_t v = w[0];
#pragma unroll
    for (uint32_t j = 1; j < GGMS_MAX_EDGE_TYPES / 4; ++j) v = (r >> 2) == j ? w[j] : v;
    return (v >> ((r & 3u) * 8u)) & 0xffu;
  }
};

__global__ __launch_bounds__(kBlock) void k_typed_bounds(const uint32_t *__restrict__ indptr,
                                                         const uint8_t *__restrict__ edge_type,
                                                         const uint32_t *__restrict__ input, Count n_arg, TypeFanouts f,
                                                         uint32_t R, uint32_t gshift, uint32_t *__restrict__ bounds,
                                                         uint32_t *__restrict__ count) {
  const uint64_t n = n_arg.get();
  const int G = 1 << gshift;
  const uint32_t per_block = (uint32_t)kBlock >> gshift;
  const uint32_t r = threadIdx.x & (uint32_t)(G - 1), sub = threadIdx.x >> gshift;
  const uint32_t kr = r < R ? f.get(r) : 0u;
  // the round loop is uniform over the workgroup: every lane of a group takes part in the group's shuffles
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < n; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t i = base + sub;
    uint32_t b = 0;
    if (i < n && r < R) {
      uint32_t b0, end;
      GraphView::bounds(indptr, input[i], b0, end);
      const uint32_t d = end - b0;
      const uint8_t *__restrict__ type = edge_type + b0;
      if (d != 0) {
        if (type[d - 1] <= r) {
          b = d;
        } else if (type[0] <= r) {
          // type[lo] <= r < type[hi] on entry; sorted lists: it holds to the end and b = hi.  Any list: 0 <= lo < hi < d
          uint32_t lo = 0, hi = d - 1;
          while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (type[mid] <= r) lo = mid; else hi = mid;
          }
          b = hi;
        }
      }
    }
    // b_{r+1} = max(b_{r+1}, b_r): an inclusive prefix maximum over the group (its lanes >= R end with b_R)
    for (int off = 1; off < G; off <<= 1) {
      const uint32_t y = __shfl_up(b, off, G);
      b = y > b ? y : b;
    }
    uint32_t prev = __shfl_up(b, 1, G);
    if (r == 0) prev = 0;
    const uint32_t e = b - prev;
    uint32_t c = e < kr ? e : kr;
    for (int off = G >> 1; off > 0; off >>= 1) c += __shfl_xor(c, off, G);
    if (i < n && r < R) bounds[i * R + r] = b;
    if (i < n && r == 0) count[i] = c;
  }
}

struct TypedCount {
  const uint32_t *count;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return count[i]; }
};
struct TypedOffset {
  uint32_t *offset;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { offset[i] = excl; }
};

// an edge of khop_typed: khop_labor's (seed's value, neighbour id), the edge's CSR position and its type
struct TypedEmit {
  uint32_t *__restrict__ src, *__restrict__ dst, *__restrict__ pos; // the outputs + the seed's offset + the segments before
  uint8_t *__restrict__ type;
  uint32_t sv, begin; // begin = indptr[seed] + b_r
  uint32_t r;
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t p, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
    pos[o] = begin + p;
    type[o] = (uint8_t)r;
  }
};

struct TypedArgs {
  const uint32_t *indptr, *indices, *input;
  const uint32_t *bounds, *count, *offset;
  uint32_t *out_src, *out_dst, *out_pos;
  uint8_t *out_type;
  TypeFanouts f;
  uint32_t R, salt;
  SrcMode sm;
  __device__ __forceinline__ TypedEmit emit_of(uint32_t at, uint32_t sv, uint32_t begin, uint32_t r) const {
    return TypedEmit{out_src + at, out_dst + at, out_pos + at, out_type + at, sv, begin, r};
  }
};

__global__ __launch_bounds__(kBlock) void k_typed_select(TypedArgs a, Count n_arg, uint32_t *heavy_count,
                                                         uint32_t *__restrict__ heavy_list) {
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t R = a.R;
  // the count is known without touching the graph: the id, the list head and the boundaries of a seed are only
  // requested where something will be emitted
  uint32_t c = wave < n ? a.count[wave] : 0u;
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t c1 = i + waves < n ? a.count[i + waves] : 0u;
    if (c != 0) {
      const uint32_t bv = lane < R ? a.bounds[i * R + lane] : 0u; // lane r: b_{r+1}
      const uint32_t rid = a.input[i];
      const uint32_t begin = a.indptr[rid];
      const uint32_t sv = a.sm.value(rid, i);
      uint32_t at = a.offset[i];
      uint32_t lo = 0;
      bool heavy = false;
      for (uint32_t r = 0; r < R; ++r) {
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)bv, (int)r);
        const uint32_t e = hi - lo, k = a.f.get(r);
        if (k != 0 && e != 0) { // uniform over the wave: the selection's ballots see all 64 lanes
          const uint32_t *__restrict__ list = a.indices + ((size_t)begin + lo);
          const TypedEmit emit = a.emit_of(at, sv, begin + lo, r);
          if (e <= k) {
            for (uint32_t p = lane; p < e; p += kWave) emit(p, p, list[p]);
          } else if (e <= kLaborWave1) {
            labor_wave_select<1>(list, e, k, a.salt, emit);
          } else if (e <= kLaborWave4) {
            labor_wave_select<4>(list, e, k, a.salt, emit);
          } else if (e <= kLaborWaveMax) {
            labor_wave_select<16>(list, e, k, a.salt, emit);
          } else {
            heavy = true; // a workgroup's segment
          }
          at += e < k ? e : k;
        }
        lo = hi;
      }
      if (heavy && lane == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)i;
    }
    c = c1;
  }
}

__global__ __launch_bounds__(kBlock) void k_typed_hub(TypedArgs a, const uint32_t *heavy_count,
                                                      const uint32_t *__restrict__ heavy_list) {
  const uint32_t nh = *heavy_count;
  const uint32_t R = a.R;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = a.input[i];
    const uint32_t begin = a.indptr[rid];
    const uint32_t sv = a.sm.value(rid, i);
    uint32_t at = a.offset[i];
    uint32_t lo = 0;
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t hi = a.bounds[(uint64_t)i * R + r];
      const uint32_t e = hi - lo, k = a.f.get(r);
      if (k != 0 && e != 0) {
        if (e > k && e > kLaborWaveMax)
          labor_hub_list(a.indices + ((size_t)begin + lo), e, k, a.salt, a.emit_of(at, sv, begin + lo, r));
        at += e < k ? e : k;
      }
      lo = hi;
    }
  }
}

// offset, heavy list, count: n words each; the boundaries: R words per seed; the heavy counter; a private scan area.
// num_type 0 (a caller that does not know it): sized for GGMS_MAX_EDGE_TYPES
size_t typed_ws_words(size_t num_input, size_t num_type) {
  const size_t R = num_type >= 1 && num_type <= GGMS_MAX_EDGE_TYPES ? num_type : GGMS_MAX_EDGE_TYPES;
  return (3 + R) * num_input + tile_scan_words(num_input) + 48;
}

// R in 1 .. 32, every k_r < 128, and their sum (0: nothing is sampled -- the caller refuses it)
int typed_fanout_sum(const uint32_t *type_fanout, uint32_t num_type, size_t *sum) {
  GGMS_CHECK_ARG(num_type >= 1 && num_type <= GGMS_MAX_EDGE_TYPES);
  GGMS_CHECK_ARG(type_fanout);
  size_t K = 0;
  for (uint32_t r = 0; r < num_type; ++r) {
    GGMS_CHECK_ARG(type_fanout[r] <= kLaborMaxFanout);
    K += type_fanout[r];
  }
  *sum = K;
  return GGMS_OK;
}

int sample_khop_typed_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t R = l.num_type;
  uint32_t *offset = l.workspace;
  uint32_t *heavy_list = offset + n_max;
  uint32_t *count = heavy_list + n_max;
  uint32_t *bounds = count + n_max;
  uint32_t *heavy_count = bounds + (size_t)R * n_max;
  uint32_t *scan_scr = heavy_count + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  TypeFanouts f{};
  for (uint32_t r = 0; r < R; ++r) f.w[r >> 2] |= (l.type_fanout[r] & 0xffu) << ((r & 3u) * 8u);
  uint32_t gshift = 0;
  while ((1u << gshift) < R) ++gshift;
  GGMS_HIP(hipMemsetAsync(heavy_count, 0, sizeof(uint32_t), l.s));
  hipLaunchKernelGGL(k_typed_bounds, dim3(grid_for(n_max, (size_t)kBlock >> gshift)), dim3(kBlock), 0, l.s, l.g.indptr,
                     l.edge_type, l.input, l.n, f, R, gshift, bounds, count);
  int rc = tile_scan(TypedCount{count}, TypedOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out, l.s);
  if (rc != GGMS_OK) return rc;
  const TypedArgs a{l.g.indptr, l.g.indices, l.input, bounds, count, offset, l.out_src, l.out_dst, l.out_pos, l.out_type,
                    f, R, l.salt, l.src};
  hipLaunchKernelGGL(k_typed_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, a, l.n, heavy_count,
                     heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device
  hipLaunchKernelGGL(k_typed_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, a, heavy_count, heavy_list);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_sample_khop_typed_workspace_bytes(size_t num_input, uint32_t num_type) {
  if (num_type < 1 || num_type > GGMS_MAX_EDGE_TYPES) return 0;
  return typed_ws_words(num_input, num_type) * sizeof(uint32_t);
}

int ggms_sample_khop_typed(const ggms_graph_t *graph, const uint8_t *edge_type, uint32_t num_type,
                           const uint32_t *type_fanout, const ggms_id_t *input, size_t num_input, uint32_t layer_salt,
                           ggms_id_t *out_src, ggms_id_t *out_dst, ggms_id_t *out_pos, uint8_t *out_type,
                           uint64_t *num_out_dev, void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  size_t K = 0;
  const int rc = typed_fanout_sum(type_fanout, num_type, &K);
  if (rc != GGMS_OK) return rc;
  SampleLayer l{graph, input, num_input, K, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  l.edge_type = edge_type;
  l.num_type = num_type;
  l.type_fanout = type_fanout;
  l.out_pos = out_pos;
  l.out_type = out_type;
  GGMS_CHECK_ARG(num_input == 0 || (edge_type && out_pos && out_type));
  return sample_leaf(GGMS_KHOP_TYPED, l, 0, workspace_bytes);
}

} // extern "C"
