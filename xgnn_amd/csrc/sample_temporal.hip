// sample_temporal.hip -- khop_temporal: time-respecting fixed-fanout neighbour sampling (include/ggms.h).
//
// Every edge position p of the CSR carries a time edge_time[p]; inside a node's list the times are non-decreasing, so
// "the edges before cut-off c" are a PREFIX of the list: its first e positions, e = the number of entries with
// time < c.  A seed comes with its own cut-off and is sampled from that prefix alone -- khop_labor's rule on [0, e)
// (GGMS_PICK_UNIFORM: the min(fanout, e) smallest keys (fmix32(t_p ^ salt) << 32) | p, labor_select.h) or the prefix's
// tail (GGMS_PICK_RECENT).  Every edge leaves with its CSR position: a temporal graph is a multigraph, and the time and
// features of a sampled edge are only recoverable from the position the sampler actually took.
//
// One layer = a 4-byte memset and four launches (+ the scan's own):
//   k_temporal_prefix  a thread per seed: the cut (the caller's array, or the batch's cut table as it stands -- the
//                      layer's snapshot), the list bounds with one 8-byte load, then e.  Two one-load exits first
//                      (time[last] < c: e = d; time[first] >= c: e = 0), else a lower-bound search: a chain of dependent
//                      4-byte loads that only occupancy hides, hence a thread per seed and a launch of its own.  A list
//                      that is not sorted gets SOME e in [0, d]: nothing is read outside the list.
//   tile_scan          offset[i] = sum of min(fanout, e) over the seeds before i; *num_out = the edge count
//   k_temporal_select  one WAVE per seed, routed by e (not by the degree: a 300 000-entry hub with 3 past edges is a
//                      copy).  RECENT, or e <= fanout: a contiguous copy.  e <= kLaborWaveMax: labor_wave_select.
//                      Longer prefixes are listed for
//   k_temporal_hub     one WORKGROUP per listed seed: labor_hub_list over the prefix.
// In a batch (ggms_sample_batch_temporal) every emitted edge f -> t also lowers t's cut-off to f's: one 64-bit atomicMax
// on the cut table per edge, no value returned.  The table is only READ by k_temporal_prefix, which is a launch in front
// of the ones that write it: stream order separates a layer's snapshot from its updates.
#include "ggms_internal.h"
#include "labor_select.h"
#include "tile_scan.h"

namespace ggms {

// a cut-table word: (stamp << 32) | (0xffffffff - cut) under unsigned 64-bit max -- a newer stamp beats a stale word,
// within a stamp the smaller cut wins; a word with another stamp reads as absent (cut = +inf = 0xffffffff)
__device__ __forceinline__ unsigned long long cut_word(uint32_t stamp, uint32_t cut) {
  return ((unsigned long long)stamp << 32) | (0xffffffffu - cut);
}
__device__ __forceinline__ uint32_t cut_of_word(unsigned long long w, uint32_t stamp) {
  return (uint32_t)(w >> 32) == stamp ? 0xffffffffu - (uint32_t)w : 0xffffffffu;
}

__global__ __launch_bounds__(kBlock) void k_temporal_prefix(const uint32_t *__restrict__ indptr,
                                                            const uint32_t *__restrict__ edge_time,
                                                            const uint32_t *__restrict__ input,
                                                            const uint32_t *__restrict__ input_cut,
                                                            const unsigned long long *cut_table, uint32_t stamp,
                                                            Count n_arg, uint32_t *__restrict__ e_out,
                                                            uint32_t *__restrict__ c_out) {
  const uint64_t n = n_arg.get();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t s = input[i];
    const uint32_t c = input_cut ? input_cut[i] : cut_of_word(cut_table[s], stamp);
    uint32_t b, end;
    GraphView::bounds(indptr, s, b, end);
    const uint32_t d = end - b;
    const uint32_t *__restrict__ time = edge_time + b;
    uint32_t e = 0;
    if (d != 0 && c != 0) {
      if (time[d - 1] < c) {
        e = d;
      } else if (time[0] < c) {
        // time[lo] < c <= time[hi] on entry; sorted lists: it holds to the end and e = hi.  Any list: 0 <= lo < hi < d
        uint32_t lo = 0, hi = d - 1;
        while (hi - lo > 1) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (time[mid] < c) lo = mid; else hi = mid;
        }
        e = hi;
      }
    }
    e_out[i] = e;
    c_out[i] = c;
  }
}

struct TemporalCount {
  const uint32_t *e;
  uint32_t fanout;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    const uint32_t v = e[i];
    return v < fanout ? v : fanout;
  }
};
struct TemporalOffset {
  uint32_t *offset;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { offset[i] = excl; }
};

// an edge of khop_temporal: khop_labor's (seed's value, neighbour id), the edge's CSR position, and in a batch the
// neighbour's cut-off lowered to the seed's
struct TemporalEmit {
  uint32_t *__restrict__ src, *__restrict__ dst, *__restrict__ pos; // the outputs + the seed's offset
  uint32_t sv, begin;                                                // begin = indptr[seed]
  unsigned long long *cut_table;                                     // NULL: a leaf call
  unsigned long long word;                                           // cut_word(stamp, the seed's cut)
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t p, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
    pos[o] = begin + p;
    if (cut_table) atomicMax(cut_table + t, word);
  }
};

struct TemporalArgs {
  const uint32_t *indptr, *indices, *input;
  const uint32_t *e, *c, *offset;
  uint32_t *out_src, *out_dst, *out_pos;
  unsigned long long *cut_table;
  uint32_t stamp, fanout, salt, recent;
  SrcMode sm;
  __device__ __forceinline__ TemporalEmit emit_of(uint64_t i, uint32_t rid, uint32_t begin) const {
    const uint32_t off = offset[i];
    return TemporalEmit{out_src + off, out_dst + off, out_pos + off, sm.value(rid, i), begin, cut_table,
                        cut_table ? cut_word(stamp, c[i]) : 0ull};
  }
};

__global__ __launch_bounds__(kBlock) void k_temporal_select(TemporalArgs a, Count n_arg, uint32_t *heavy_count,
                                                            uint32_t *__restrict__ heavy_list) {
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t k = a.fanout;
  // the prefix length is known without touching the graph: the id and the list head of a seed are only requested
  // where something will be emitted (a seed with nothing before its cut costs one 4-byte load)
  uint32_t e = wave < n ? a.e[wave] : 0u;
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t e1 = i + waves < n ? a.e[i + waves] : 0u;
    if (e != 0 && (a.recent || e <= kLaborWaveMax)) {
      const uint32_t rid = a.input[i];
      const uint32_t begin = a.indptr[rid];
      const uint32_t *__restrict__ list = a.indices + begin;
      const TemporalEmit emit = a.emit_of(i, rid, begin);
      if (a.recent || e <= k) { // a contiguous run: the whole prefix, or its last k positions
        const uint32_t m = e < k ? e : k, first = e - m;
        for (uint32_t o = lane; o < m; o += kWave) emit(o, first + o, list[first + o]);
      } else if (e <= kLaborWave1) {
        labor_wave_select<1>(list, e, k, a.salt, emit);
      } else if (e <= kLaborWave4) {
        labor_wave_select<4>(list, e, k, a.salt, emit);
      } else {
        labor_wave_select<16>(list, e, k, a.salt, emit);
      }
    } else if (e != 0) { // a workgroup's prefix
      if (lane == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)i;
    }
    e = e1;
  }
}

__global__ __launch_bounds__(kBlock) void k_temporal_hub(TemporalArgs a, const uint32_t *heavy_count,
                                                         const uint32_t *__restrict__ heavy_list) {
  const uint32_t nh = *heavy_count;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = a.input[i];
    const uint32_t begin = a.indptr[rid];
    labor_hub_list(a.indices + begin, a.e[i], a.fanout, a.salt, a.emit_of(i, rid, begin));
  }
}

// offset, heavy list, e, c: n words each; the heavy counter; a private scan area
size_t temporal_ws_words(size_t num_input) { return 4 * num_input + tile_scan_words(num_input) + 48; }

int sample_khop_temporal_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t fanout = (uint32_t)l.fanout;
  uint32_t *offset = l.workspace;
  uint32_t *heavy_list = offset + n_max;
  uint32_t *e = heavy_list + n_max;
  uint32_t *c = e + n_max;
  uint32_t *heavy_count = c + n_max;
  uint32_t *scan_scr = heavy_count + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  unsigned long long *cut_table = reinterpret_cast<unsigned long long *>(l.cut_table);
  GGMS_HIP(hipMemsetAsync(heavy_count, 0, sizeof(uint32_t), l.s));
  hipLaunchKernelGGL(k_temporal_prefix, dim3(grid_for(n_max, kBlock)), dim3(kBlock), 0, l.s, l.g.indptr, l.edge_time,
                     l.input, l.input_cut, cut_table, l.stamp, l.n, e, c);
  int rc = tile_scan(TemporalCount{e, fanout}, TemporalOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out, l.s);
  if (rc != GGMS_OK) return rc;
  const TemporalArgs a{l.g.indptr, l.g.indices, l.input, e, c, offset, l.out_src, l.out_dst, l.out_pos, cut_table,
                       l.stamp, fanout, l.salt, l.pick == GGMS_PICK_RECENT ? 1u : 0u, l.src};
  hipLaunchKernelGGL(k_temporal_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, a, l.n, heavy_count,
                     heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device (RECENT lists none)
  if (l.pick != GGMS_PICK_RECENT)
    hipLaunchKernelGGL(k_temporal_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, a, heavy_count, heavy_list);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

// ---- the batch's side launches ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_temporal_seed_cut(const uint32_t *__restrict__ seeds,
                                                              const uint32_t *__restrict__ seed_time, uint64_t n,
                                                              unsigned long long *cut_table, uint32_t stamp) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    atomicMax(cut_table + seeds[i], cut_word(stamp, seed_time[i]));
}

__global__ __launch_bounds__(kBlock) void k_temporal_node_cut(const uint32_t *__restrict__ n2o, Count n_arg,
                                                              const unsigned long long *__restrict__ cut_table,
                                                              uint32_t stamp, uint32_t *__restrict__ node_cut) {
  const uint64_t n = n_arg.get();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    node_cut[i] = cut_of_word(cut_table[n2o[i]], stamp);
}

int temporal_seed_cut_impl(const uint32_t *seeds, const uint32_t *seed_time, size_t num_seeds, uint64_t *cut_table,
                           uint32_t stamp, hipStream_t s) {
  if (num_seeds == 0) return GGMS_OK;
  hipLaunchKernelGGL(k_temporal_seed_cut, dim3(grid_for(num_seeds, kBlock)), dim3(kBlock), 0, s, seeds, seed_time,
                     (uint64_t)num_seeds, reinterpret_cast<unsigned long long *>(cut_table), stamp);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

int temporal_node_cut_impl(const uint32_t *n2o, size_t n_max, Count n, const uint64_t *cut_table, uint32_t stamp,
                           uint32_t *node_cut, hipStream_t s) {
  if (n_max == 0) return GGMS_OK;
  hipLaunchKernelGGL(k_temporal_node_cut, dim3(grid_for(n_max, kBlock)), dim3(kBlock), 0, s, n2o, n,
                     reinterpret_cast<const unsigned long long *>(cut_table), stamp, node_cut);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

// ggms_link_seed_times: position q of ggms_link_seeds' endpoint layout belongs to positive q (sources), q - B
// (destinations) or (q - 2 B) / K (negatives)
__global__ __launch_bounds__(kBlock) void k_link_seed_times(const uint32_t *__restrict__ edge_time,
                                                            const uint32_t *__restrict__ edge_ids, uint64_t num_edge,
                                                            uint64_t B, Divisor K, uint32_t *__restrict__ out_time) {
  const uint64_t total = B * (2 + K.d);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < total; q += stride) {
    uint64_t i = q < B ? q : q - B;
    if (q >= 2 * B) {
      uint32_t quo, rem;
      K.divmod((uint32_t)(q - 2 * B), quo, rem);
      i = quo;
    }
    const uint32_t eid = edge_ids[i];
    out_time[q] = eid < num_edge ? edge_time[eid] : 0u;
  }
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_sample_khop_temporal(const ggms_graph_t *graph, const uint32_t *edge_time, const ggms_id_t *input,
                              const uint32_t *input_cut, size_t num_input, size_t fanout, int pick, uint32_t layer_salt,
                              ggms_id_t *out_src, ggms_id_t *out_dst, ggms_id_t *out_pos, uint64_t *num_out_dev,
                              void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  SampleLayer l{graph, input, num_input, fanout, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  l.edge_time = edge_time;
  l.input_cut = input_cut;
  l.out_pos = out_pos;
  l.pick = pick;
  GGMS_CHECK_ARG(pick == GGMS_PICK_UNIFORM || pick == GGMS_PICK_RECENT);
  GGMS_CHECK_ARG(num_input == 0 || (edge_time && input_cut && out_pos));
  return sample_leaf(GGMS_KHOP_TEMPORAL, l, 0, workspace_bytes);
}

int ggms_link_seed_times(const uint32_t *edge_time, uint64_t num_edge, const ggms_id_t *edge_ids, size_t num_pos,
                         uint32_t num_negative, uint32_t *out_time, ggms_stream_t stream) {
  GGMS_CHECK_ARG(num_negative >= 1 && num_negative <= 64);
  if (num_pos == 0) return GGMS_OK;
  GGMS_CHECK_ARG(edge_time && edge_ids && out_time);
  GGMS_CHECK_ARG((uint64_t)num_pos * num_negative < (1ull << 32));
  hipLaunchKernelGGL(k_link_seed_times, dim3(grid_for(num_pos * (2 + num_negative), kBlock)), dim3(kBlock), 0,
                     to_stream(stream), edge_time, edge_ids, num_edge, (uint64_t)num_pos, divisor_of(num_negative),
                     out_time);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // extern "C"
