// sample_labor_weighted.hip -- khop_labor_weighted: fixed-fanout WEIGHTED sampling without replacement, with khop_labor's
// per-node shared randomness (include/ggms.h).
//
// Efraimidis-Spirakis / exponential clocks: edge p of a seed's list gets the key E(t_p) / w_p, E an Exp(1) variate that
// belongs to the NODE t_p (a function of fmix32(t_p ^ layer_salt)), w_p the edge's weight; the min(fanout, d) smallest
// keys are a sample without replacement in which an edge's chance grows with its weight, and seeds that share a
// neighbour share its variate (khop_labor's batch-shrinking effect).  The key is integer arithmetic plus ONE IEEE
// division, so the numpy statement reproduces it bit for bit:
//   h = fmix32(t ^ salt); v = 2 h + 1 (33 bits); e = floor(log2 v); the 32 fraction bits f of v below its top bit;
//   L = (e << 32) + T[f >> 24] + (((T[(f >> 24) + 1] - T[f >> 24]) * (f & 0xffffff)) >> 24)   (labor_log2_table.h)
//   E = (33 << 32) - L >= 1;  key32 = bits(float(E) / clamp(w, 2^-40, 2^40));  key = (key32 << 32) | p
// Positive floats order like their bit patterns: the selection is khop_labor's bottom-k over another 32-bit number.
//
// One layer = khop_labor's chain: a 4-byte memset, tile_scan (counts min(fanout, d): LaborCount), and
//   k_weighted_select  one WAVE per seed.  d <= fanout: the list is copied.  d <= kLaborWaveMax: a lane holds 1, 4 or
//                      16 (id, weight) pairs -- both loads of a pair are issued before anything is computed -- turns
//                      them into key32 in registers, and the k-th smallest is found by the 32-round ballot / popcount
//                      threshold search; ties (equal ids with equal weights) break by position.  The log table is
//                      copied into LDS once per workgroup: 64 lanes index it with 64 different hashes.  Longer lists are
//                      listed for
//   k_weighted_hub     one WORKGROUP per listed seed.  khop_labor predicts its pre-filter threshold from k / d; with
//                      weights the expected number of keys under tau (Exp(1) units) is sum(1 - exp(-w_i tau)) <= W tau,
//                      W = the sum of the clamped weights.  So pass 1 streams the weights alone and block-reduces W,
//                      pass 2 streams ids and weights and keeps the keys under tau = (2 k + 64) / W in LDS (kLaborCand
//                      slots), and the bitwise search for the k-th smallest 64-bit key runs over LDS.  Fewer than k
//                      survivors (a few weights carry W) or more than the buffer holds (equal ids with equal weights):
//                      the exact route -- the 32-round search over the list itself, keys recomputed per round, and an
//                      ordered emit with block scans.  W and tau are floating-point sums whose rounding depends on the
//                      reduction order; they only choose the ROUTE, never the edges.
// Output positions come from the scan and from ranks inside a seed; the one atomic is the heavy list's counter.
#include "ggms_internal.h"
#include "labor_log2_table.h"
#include "labor_select.h"
#include "tile_scan.h"

namespace ggms {

constexpr float kWeightMin = 0x1p-40f, kWeightMax = 0x1p40f;
constexpr float kExpScale = 6196328018.6f; // 2^32 / ln 2: an Exp(1) value in the units of E

// fminf(fmaxf(w, 2^-40), 2^40) with the NaN case spelled out: a NaN fails the first comparison and becomes 2^-40
__device__ __forceinline__ float weight_clamp(float w) {
  const float lo = w > kWeightMin ? w : kWeightMin;
  return lo < kWeightMax ? lo : kWeightMax;
}

// key32 of (neighbour id, weight); T = the log table in LDS
__device__ __forceinline__ uint32_t weighted_key32(uint32_t t, float w, uint32_t salt, const uint64_t *T) {
  return __float_as_uint((float)labor_exp_units(t, salt, T) / weight_clamp(w));
}

// an edge of khop_labor_weighted: khop_labor's (seed's value, neighbour id) and the edge's CSR position
struct WeightedEmit {
  uint32_t *__restrict__ src, *__restrict__ dst, *__restrict__ pos; // the outputs + the seed's offset
  uint32_t sv, begin;                                                // begin = indptr[seed]
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t p, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
    pos[o] = begin + p;
  }
};

struct WeightedArgs {
  GraphView g; // one CSR: a list's first position is list - g.indices
  const float *edge_weight;
  const uint32_t *input, *offset;
  uint32_t *out_src, *out_dst, *out_pos;
  uint32_t fanout, salt;
  SrcMode sm;
  __device__ __forceinline__ WeightedEmit emit_of(uint64_t i, uint32_t rid, uint32_t begin) const {
    const uint32_t off = offset[i];
    return WeightedEmit{out_src + off, out_dst + off, out_pos + off, sm.value(rid, i), begin};
  }
};

// fanout < d <= 64 R: the whole list's keys in the wave's registers, position p = 64 r + lane (labor_wave_select's
// search over key32 instead of the hash).  A COPY of labor_select.h's search, tie logic and emit, as weighted_hub_list's
// LDS search and exact route are of labor_hub_list's: a fix to the selection there belongs here too
template <int R>
__device__ __forceinline__ void weighted_wave_select(const uint32_t *__restrict__ list, const float *__restrict__ wl,
                                                     uint32_t d, uint32_t k, uint32_t salt, const uint64_t *T,
                                                     const WeightedEmit &emit) {
  const uint32_t lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t t[R], key[R];
  float w[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = 64u * r + lane;
    t[r] = p < d ? list[p] : 0u;
    w[r] = p < d ? wl[p] : 1.0f;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) key[r] = weighted_key32(t[r], w[r], salt, T);
  // V = the k-th smallest key32: the largest V with fewer than k keys below it
  uint32_t V = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t X = V | (1u << bit);
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) c += (uint32_t)__popcll(__ballot(64u * r + lane < d && key[r] < X));
    if (c < k) V = X;
  }
  uint32_t less = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) less += (uint32_t)__popcll(__ballot(64u * r + lane < d && key[r] < V));
  const uint32_t need = k - less; // of the positions whose key32 IS V, the first `need`
  uint32_t ties = 0, out = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool in = 64u * r + lane < d;
    const uint64_t eq = __ballot(in && key[r] == V);
    const bool sel = in && (key[r] < V || (key[r] == V && ties + (uint32_t)__popcll(eq & below) < need));
    const uint64_t sm = __ballot(sel);
    if (sel) emit(out + (uint32_t)__popcll(sm & below), 64u * r + lane, t[r]);
    ties += (uint32_t)__popcll(eq);
    out += (uint32_t)__popcll(sm);
  }
}

__global__ __launch_bounds__(kBlock) void k_weighted_select(WeightedArgs a, Count n_arg, uint32_t *heavy_count,
                                                            uint32_t *__restrict__ heavy_list) {
  __shared__ uint64_t s_T[kLaborLogEntries];
  load_log_table(s_T);
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t k = a.fanout;
  // k_labor_select's prefetch: the id of the seed two rounds ahead and the head of the next one are requested before
  // this round's list is touched
  uint32_t rid = wave < n ? a.input[wave] : 0u;
  uint32_t rid1 = wave + waves < n ? a.input[wave + waves] : 0u;
  uint32_t d = 0;
  const uint32_t *list = nullptr;
  if (wave < n) list = a.g.neighbours(rid, d);
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t rid2 = i + 2 * waves < n ? a.input[i + 2 * waves] : 0u;
    uint32_t d1 = 0;
    const uint32_t *list1 = nullptr;
    if (i + waves < n) list1 = a.g.neighbours(rid1, d1);
    if (d > kLaborWaveMax) { // a workgroup's list
      if (lane == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)i;
    } else if (d != 0) {
      const uint32_t begin = (uint32_t)(list - a.g.indices);
      const float *__restrict__ wl = a.edge_weight + begin;
      const WeightedEmit emit = a.emit_of(i, rid, begin);
      if (d <= k) {
        for (uint32_t p = lane; p < d; p += kWave) emit(p, p, list[p]);
      } else if (d <= kLaborWave1) {
        weighted_wave_select<1>(list, wl, d, k, a.salt, s_T, emit);
      } else if (d <= kLaborWave4) {
        weighted_wave_select<4>(list, wl, d, k, a.salt, s_T, emit);
      } else {
        weighted_wave_select<16>(list, wl, d, k, a.salt, s_T, emit);
      }
    }
    rid = rid1;
    rid1 = rid2;
    d = d1;
    list = list1;
  }
}

// key32 of list[0, d) below X, counted by the workgroup's lanes (U pairs in flight each); the caller sums
template <uint32_t U = 8>
__device__ __forceinline__ uint32_t weighted_count_below(const uint32_t *__restrict__ list, const float *__restrict__ wl,
                                                         uint32_t d, uint32_t salt, const uint64_t *T, uint32_t X) {
  uint32_t c = 0;
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
    float w[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + threadIdx.x;
      v[u] = p < d ? list[p] : 0u;
      w[u] = p < d ? wl[p] : 1.0f;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u)
      c += (base + u * kBlock + threadIdx.x < d && weighted_key32(v[u], w[u], salt, T) < X) ? 1u : 0u;
  }
  return c;
}

// One list by the whole workgroup (every thread calls it with the same arguments; d > kLaborWaveMax >= 2 k + 64).
// Ends with a barrier: the next call may rewrite the LDS at once.
__device__ __forceinline__ void weighted_hub_list(const uint32_t *__restrict__ list, const float *__restrict__ wl,
                                                  uint32_t d, uint32_t k, uint32_t salt, const uint64_t *T,
                                                  const WeightedEmit &emit) {
  constexpr uint32_t U = 16; // (id, weight) pairs a lane has in flight: one workgroup streams the whole list
  __shared__ unsigned long long s_key[kLaborCand];
  __shared__ uint32_t s_sel[kLaborMaxFanout + 1];
  __shared__ uint32_t s_sum[2][kBlock / kWave];
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ float s_w[kBlock / kWave];
  __shared__ uint32_t s_cnt, s_nsel;
  const uint32_t tid = threadIdx.x;
  // ---- pass 1: W = the sum of the clamped weights (every term >= 2^-40, at most 2^32 terms of at most 2^40: finite)
  float wsum = 0.0f;
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    float w[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + tid;
      w[u] = p < d ? weight_clamp(wl[p]) : 0.0f;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) wsum += w[u];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) wsum += __shfl_xor(wsum, off, 64);
  if (lane_id() == 0) s_w[tid >> 6] = wsum;
  if (tid == 0) {
    s_cnt = 0;
    s_nsel = 0;
  }
  __syncthreads();
  static_assert(kBlock / kWave == 4, "the sum of W below (and labor_block_sum) adds four waves' partial sums");
  const float W = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]); // the same value in every thread
  // tau = (2 k + 64) / W in Exp(1) units, as a key32: a positive normal float (W in [2^-30, 2^72])
  const uint32_t T0 = __float_as_uint((float)(2u * k + 64u) * kExpScale / W);
  // ---- pass 2: the keys under the threshold
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
    float w[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + tid;
      v[u] = p < d ? list[p] : 0u;
      w[u] = p < d ? wl[p] : 1.0f;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + tid;
      const uint32_t key = weighted_key32(v[u], w[u], salt, T);
      if (p < d && key < T0) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        if (slot < kLaborCand) s_key[slot] = ((unsigned long long)key << 32) | (uint32_t)p;
      }
    }
  }
  __syncthreads();
  const uint32_t m = s_cnt;
  uint32_t turn = 0;
  if (m >= k && m <= kLaborCand) {
    // ---- the k-th smallest key among the survivors: key32 is below T0 and positions below d, the bits above either
    // are zero in every key
    unsigned long long K = 0;
    const int key_top = 63 - __clzll((long long)(((unsigned long long)T0 << 32) | 0xffffffffull));
    const int pos_top = 31 - __clz((int)(d - 1u));
    for (int bit = key_top; bit >= 0; --bit) {
      if (bit < 32 && bit > pos_top) continue;
      const unsigned long long X = K | (1ull << bit);
      uint32_t c = 0;
      for (uint32_t j = tid; j < m; j += kBlock) c += s_key[j] < X ? 1u : 0u;
      if (labor_block_sum(c, s_sum, turn++) < k) K = X;
    }
    for (uint32_t j = tid; j < m; j += kBlock)
      if (s_key[j] <= K) { // exactly k of them: keys are distinct
        const uint32_t slot = atomicAdd(&s_nsel, 1u);
        if (slot <= kLaborMaxFanout) s_sel[slot] = (uint32_t)s_key[j];
      }
    __syncthreads();
    if (tid < k) {
      const uint32_t p = s_sel[tid];
      uint32_t rank = 0;
      for (uint32_t x = 0; x < k; ++x) rank += s_sel[x] < p ? 1u : 0u;
      emit(rank, p, list[p]);
    }
  } else {
    // ---- the exact route: the k-th smallest key32 over the list itself, then an emit in position order
    uint32_t V = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t X = V | (1u << bit);
      if (labor_block_sum(weighted_count_below(list, wl, d, salt, T, X), s_sum, turn++) < k) V = X;
    }
    const uint32_t need = k - labor_block_sum(weighted_count_below(list, wl, d, salt, T, V), s_sum, turn++);
    uint32_t ties = 0, out = 0;
    for (uint64_t base = 0; base < d && out < k; base += kBlock) {
      const uint64_t p = base + tid;
      const uint32_t t = p < d ? list[p] : 0u;
      const uint32_t key = weighted_key32(t, p < d ? wl[p] : 1.0f, salt, T);
      const bool lt = p < d && key < V, eq = p < d && key == V;
      if (!__syncthreads_or(lt || eq)) continue;
      uint32_t tie_total, sel_total;
      const uint32_t tie_rank = ties + block_exclusive_scan(eq ? 1u : 0u, s_scan, tie_total);
      const bool sel = lt || (eq && tie_rank < need);
      const uint32_t o = out + block_exclusive_scan(sel ? 1u : 0u, s_scan, sel_total);
      if (sel) emit(o, (uint32_t)p, t);
      ties += tie_total;
      out += sel_total;
    }
  }
  __syncthreads(); // s_key / s_sel / s_w / the counters are rewritten by the next list
}

__global__ __launch_bounds__(kBlock) void k_weighted_hub(WeightedArgs a, const uint32_t *heavy_count,
                                                         const uint32_t *__restrict__ heavy_list) {
  __shared__ uint64_t s_T[kLaborLogEntries];
  const uint32_t nh = *heavy_count;
  if (blockIdx.x >= nh) return; // uniform over the workgroup: no barrier is left behind
  load_log_table(s_T);
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = a.input[i];
    uint32_t d;
    const uint32_t *__restrict__ list = a.g.neighbours(rid, d);
    const uint32_t begin = (uint32_t)(list - a.g.indices);
    weighted_hub_list(list, a.edge_weight + begin, d, a.fanout, a.salt, s_T, a.emit_of(i, rid, begin));
  }
}

int sample_khop_labor_weighted_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t fanout = (uint32_t)l.fanout;
  uint32_t *offset = l.workspace; // labor_ws_words' layout
  uint32_t *heavy_list = offset + n_max;
  uint32_t *heavy_count = heavy_list + n_max;
  uint32_t *scan_scr = heavy_count + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  GGMS_HIP(hipMemsetAsync(heavy_count, 0, sizeof(uint32_t), l.s));
  int rc = tile_scan(LaborCount{l.g, l.input, fanout}, LaborOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out,
                     l.s);
  if (rc != GGMS_OK) return rc;
  const WeightedArgs a{l.g, l.edge_weight, l.input, offset, l.out_src, l.out_dst, l.out_pos, fanout, l.salt, l.src};
  hipLaunchKernelGGL(k_weighted_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, a, l.n, heavy_count,
                     heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device
  hipLaunchKernelGGL(k_weighted_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, a, heavy_count, heavy_list);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_sample_khop_labor_weighted(const ggms_graph_t *graph, const float *edge_weight, const ggms_id_t *input,
                                    size_t num_input, size_t fanout, uint32_t layer_salt, ggms_id_t *out_src,
                                    ggms_id_t *out_dst, ggms_id_t *out_pos, uint64_t *num_out_dev, void *workspace,
                                    size_t workspace_bytes, ggms_stream_t stream) {
  SampleLayer l{graph, input, num_input, fanout, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  l.edge_weight = edge_weight;
  l.out_pos = out_pos;
  GGMS_CHECK_ARG(num_input == 0 || (edge_weight && out_pos));
  return sample_leaf(GGMS_KHOP_LABOR_WEIGHTED, l, 0, workspace_bytes);
}

} // extern "C"
