// sample_labor.hip -- khop_labor: fixed-fanout neighbour sampling with per-node shared randomness.
//
// LABOR (layer-neighbour sampling) in its fixed-size form, bottom-k / sequential Poisson sampling: the random variate
// belongs to the NODE, not to the (seed, neighbour) pair, so every seed of a layer that could pick neighbour t sees
// the same number for t and seeds with overlapping lists pick overlapping neighbours -- fewer distinct nodes per
// batch, hence fewer table inserts and fewer feature rows (DESIGN.md "khop_labor").  There is no reference
// counterpart; the definition (include/ggms.h):
//   position p of the seed's list t_0 .. t_{d-1} has the key (fmix32(t_p ^ layer_salt) << 32) | p;
//   selected are the min(fanout, d) positions with the smallest keys, emitted in ascending position.
// The variate is a hash: no RNG pool, no order between batches, the output is a pure function of the inputs.
//
// One layer = a 4-byte memset and three launches:
//   tile_scan       offset[i] = sum of min(fanout, d) over the seeds before i; *num_out = the edge count
//   k_labor_select  one WAVE per seed.  d <= fanout: the list is copied.  d <= kLaborWaveMax: the hashes of the whole
//                   list sit in registers (1, 4 or 16 per lane: kLaborWave1 / kLaborWave4 / kLaborWaveMax), the k-th
//                   smallest hash is found by a bitwise threshold search -- 32 rounds of ballot + popcount, no LDS, no
//                   sort -- equal hashes (multi-edges) are broken by position, and the selected positions leave in
//                   order at ranks counted with the same ballots.  Longer lists are listed (heavy_list) for
//   k_labor_hub     one WORKGROUP per listed seed.  A first pass over the list keeps the keys whose hash is under the
//                   threshold that fanout / d predicts with slack ((2 fanout + 64) / d of the hash range: 66 .. 318
//                   expected survivors) in an LDS buffer of kLaborCand keys; the k-th smallest KEY among the survivors
//                   is found by the same bitwise search over LDS, and the k selected positions are ranked by position.
//                   Fewer than fanout survivors, or more than the buffer holds (an adversarial or multi-edge list):
//                   the exact route -- the bitwise search over the list itself (32 more passes, L2-resident for any
//                   list that matters) and an ordered emit with block scans.
// Output positions come from the scan and from ranks inside a seed: no atomic touches the output.  The one atomic of
// the layer is the heavy list's counter (which hub goes to which workgroup is not observable).
#include "ggms_internal.h"
#include "labor_hash.h"
#include "tile_scan.h"

namespace ggms {

constexpr uint32_t kLaborWave1 = 64;     // list lengths up to which a lane of the seed's wave holds 1 key,
constexpr uint32_t kLaborWave4 = 256;    // 4 keys,
constexpr uint32_t kLaborWaveMax = 1024; // 16 keys; longer lists take a workgroup (k_labor_hub)
constexpr uint32_t kLaborCand = 1024;    // keys the hub pre-filter's LDS buffer holds (8 KB)
constexpr uint32_t kLaborMaxFanout = 127;

struct LaborCount {
  GraphView g;
  const uint32_t *input;
  uint32_t fanout;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    uint32_t len;
    g.neighbours(input[i], len);
    return len < fanout ? len : fanout;
  }
};
struct LaborOffset {
  uint32_t *offset;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { offset[i] = excl; }
};

// fanout < d <= 64 R: the whole list in the wave's registers, position p = 64 r + lane
template <int R>
__device__ __forceinline__ void labor_wave_select(const uint32_t *__restrict__ list, uint32_t d, uint32_t k, uint32_t salt,
                                                  uint32_t sv, uint32_t *__restrict__ out_src,
                                                  uint32_t *__restrict__ out_dst) {
  const uint32_t lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t t[R], h[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = 64u * r + lane;
    t[r] = p < d ? list[p] : 0u;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) h[r] = fmix32(t[r] ^ salt);
  // V = the k-th smallest hash: the largest V with fewer than k hashes below it
  uint32_t V = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t T = V | (1u << bit);
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) c += (uint32_t)__popcll(__ballot(64u * r + lane < d && h[r] < T));
    if (c < k) V = T;
  }
  uint32_t less = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) less += (uint32_t)__popcll(__ballot(64u * r + lane < d && h[r] < V));
  const uint32_t need = k - less; // of the positions whose hash IS V, the first `need`
  uint32_t ties = 0, out = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool in = 64u * r + lane < d;
    const uint64_t eq = __ballot(in && h[r] == V);
    const bool sel = in && (h[r] < V || (h[r] == V && ties + (uint32_t)__popcll(eq & below) < need));
    const uint64_t sm = __ballot(sel);
    if (sel) {
      const uint32_t o = out + (uint32_t)__popcll(sm & below);
      out_src[o] = sv;
      out_dst[o] = t[r];
    }
    ties += (uint32_t)__popcll(eq);
    out += (uint32_t)__popcll(sm);
  }
}

__global__ __launch_bounds__(kBlock) void k_labor_select(GraphView g, const uint32_t *__restrict__ input, Count n_arg,
                                                         uint32_t fanout, uint32_t salt,
                                                         const uint32_t *__restrict__ offset,
                                                         uint32_t *__restrict__ out_src, uint32_t *__restrict__ out_dst,
                                                         SrcMode sm, uint32_t *heavy_count,
                                                         uint32_t *__restrict__ heavy_list) {
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  // The chain seed id -> list head -> list is three dependent round trips and a wave has one seed in flight: the id
  // of the seed two rounds ahead and the head of the next one are requested before this round's list is touched
  uint32_t rid = wave < n ? input[wave] : 0u;
  uint32_t rid1 = wave + waves < n ? input[wave + waves] : 0u;
  uint32_t d = 0;
  const uint32_t *list = nullptr;
  if (wave < n) list = g.neighbours(rid, d);
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t rid2 = i + 2 * waves < n ? input[i + 2 * waves] : 0u;
    uint32_t d1 = 0;
    const uint32_t *list1 = nullptr;
    if (i + waves < n) list1 = g.neighbours(rid1, d1);
    if (d > kLaborWaveMax) { // a workgroup's list
      if (lane == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)i;
    } else if (d != 0) {
      const uint32_t off = offset[i];
      const uint32_t sv = sm.value(rid, i);
      if (d <= fanout) {
        for (uint32_t p = lane; p < d; p += kWave) {
          out_src[off + p] = sv;
          out_dst[off + p] = list[p];
        }
      } else if (d <= kLaborWave1) {
        labor_wave_select<1>(list, d, fanout, salt, sv, out_src + off, out_dst + off);
      } else if (d <= kLaborWave4) {
        labor_wave_select<4>(list, d, fanout, salt, sv, out_src + off, out_dst + off);
      } else {
        labor_wave_select<16>(list, d, fanout, salt, sv, out_src + off, out_dst + off);
      }
    }
    rid = rid1;
    rid1 = rid2;
    d = d1;
    list = list1;
  }
}

// sum of x over the workgroup; buf: 2 x 4 words, `turn` alternates between calls (one barrier per call)
__device__ __forceinline__ uint32_t labor_block_sum(uint32_t x, uint32_t (*buf)[kBlock / kWave], uint32_t turn) {
  x = wave_reduce_sum(x);
  if (lane_id() == 0) buf[turn & 1u][threadIdx.x >> 6] = x;
  __syncthreads();
  return buf[turn & 1u][0] + buf[turn & 1u][1] + buf[turn & 1u][2] + buf[turn & 1u][3];
}

// hashes of list[0, d) below T, counted by the workgroup's lanes (U loads in flight each); the caller sums
template <uint32_t U = 8>
__device__ __forceinline__ uint32_t labor_count_below(const uint32_t *__restrict__ list, uint32_t d, uint32_t salt,
                                                      uint32_t T) {
  uint32_t c = 0;
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + threadIdx.x;
      v[u] = p < d ? list[p] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) c += (base + u * kBlock + threadIdx.x < d && fmix32(v[u] ^ salt) < T) ? 1u : 0u;
  }
  return c;
}

__global__ __launch_bounds__(kBlock) void k_labor_hub(GraphView g, const uint32_t *__restrict__ input, uint32_t fanout,
                                                      uint32_t salt, const uint32_t *__restrict__ offset,
                                                      uint32_t *__restrict__ out_src, uint32_t *__restrict__ out_dst,
                                                      SrcMode sm, const uint32_t *heavy_count,
                                                      const uint32_t *__restrict__ heavy_list) {
  constexpr uint32_t U = 32; // list entries a lane has in flight in the first pass: one workgroup streams the whole list
  __shared__ unsigned long long s_key[kLaborCand];
  __shared__ uint32_t s_sel[kLaborMaxFanout + 1];
  __shared__ uint32_t s_sum[2][kBlock / kWave];
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ uint32_t s_cnt, s_nsel;
  const uint32_t nh = *heavy_count;
  const uint32_t k = fanout;
  const uint32_t tid = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = input[i];
    uint32_t d;
    const uint32_t *__restrict__ list = g.neighbours(rid, d);
    const uint32_t off = offset[i];
    const uint32_t sv = sm.value(rid, i);
    // ---- first pass: the keys under the predicted threshold (d > kLaborWaveMax >= 2 k + 64, so T0 < 2^32)
    const uint32_t T0 = (uint32_t)(((uint64_t)(2u * k + 64u) << 32) / d);
    if (tid == 0) {
      s_cnt = 0;
      s_nsel = 0;
    }
    __syncthreads();
    for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
      uint32_t v[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint64_t p = base + u * kBlock + tid;
        v[u] = p < d ? list[p] : 0u;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint64_t p = base + u * kBlock + tid;
        const uint32_t h = fmix32(v[u] ^ salt);
        if (p < d && h < T0) {
          const uint32_t slot = atomicAdd(&s_cnt, 1u);
          if (slot < kLaborCand) s_key[slot] = ((unsigned long long)h << 32) | (uint32_t)p;
        }
      }
    }
    __syncthreads();
    const uint32_t m = s_cnt;
    uint32_t turn = 0;
    if (m >= k && m <= kLaborCand) {
      // ---- the k-th smallest key among the survivors: hashes are below T0 and positions below d, the bits above
      // either are zero in every key
      unsigned long long K = 0;
      const int hash_top = 63 - __clzll(((unsigned long long)T0 << 32) | 0xffffffffull);
      const int pos_top = 31 - __clz((int)(d - 1u));
      for (int bit = hash_top; bit >= 0; --bit) {
        if (bit < 32 && bit > pos_top) continue;
        const unsigned long long T = K | (1ull << bit);
        uint32_t c = 0;
        for (uint32_t j = tid; j < m; j += kBlock) c += s_key[j] < T ? 1u : 0u;
        if (labor_block_sum(c, s_sum, turn++) < k) K = T;
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
        out_src[off + rank] = sv;
        out_dst[off + rank] = list[p];
      }
    } else {
      // ---- the exact route: the k-th smallest hash over the list itself, then an emit in position order
      uint32_t V = 0;
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t T = V | (1u << bit);
        if (labor_block_sum(labor_count_below(list, d, salt, T), s_sum, turn++) < k) V = T;
      }
      const uint32_t need = k - labor_block_sum(labor_count_below(list, d, salt, V), s_sum, turn++);
      uint32_t ties = 0, out = 0;
      for (uint64_t base = 0; base < d && out < k; base += kBlock) {
        const uint64_t p = base + tid;
        const uint32_t t = p < d ? list[p] : 0u;
        const uint32_t h = fmix32(t ^ salt);
        const bool lt = p < d && h < V, eq = p < d && h == V;
        if (!__syncthreads_or(lt || eq)) continue;
        uint32_t tie_total, sel_total;
        const uint32_t tie_rank = ties + block_exclusive_scan(eq ? 1u : 0u, s_scan, tie_total);
        const bool sel = lt || (eq && tie_rank < need);
        const uint32_t o = out + block_exclusive_scan(sel ? 1u : 0u, s_scan, sel_total);
        if (sel) {
          out_src[off + o] = sv;
          out_dst[off + o] = t;
        }
        ties += tie_total;
        out += sel_total;
      }
    }
    __syncthreads(); // s_key / s_sel / the counters are rewritten by the next list
  }
}

size_t labor_ws_words(size_t num_input) { return 2 * num_input + tile_scan_words(num_input) + 48; }

int sample_khop_labor_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t fanout = (uint32_t)l.fanout;
  uint32_t *offset = l.workspace;
  uint32_t *heavy_list = offset + n_max;
  uint32_t *heavy_count = heavy_list + n_max;
  uint32_t *scan_scr = heavy_count + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  GGMS_HIP(hipMemsetAsync(heavy_count, 0, sizeof(uint32_t), l.s));
  int rc = tile_scan(LaborCount{l.g, l.input, fanout}, LaborOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out,
                     l.s);
  if (rc != GGMS_OK) return rc;
  hipLaunchKernelGGL(k_labor_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, l.g, l.input, l.n,
                     fanout, l.salt, offset, l.out_src, l.out_dst, l.src, heavy_count, heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device
  hipLaunchKernelGGL(k_labor_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, l.g, l.input, fanout, l.salt, offset,
                     l.out_src, l.out_dst, l.src, heavy_count, heavy_list);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_sample_khop_labor(const ggms_graph_t *graph, const ggms_id_t *input, size_t num_input, size_t fanout,
                           uint32_t layer_salt, ggms_id_t *out_src, ggms_id_t *out_dst, uint64_t *num_out_dev,
                           void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  SampleLayer l{graph, input, num_input, fanout, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  return sample_leaf(GGMS_KHOP_LABOR, l, 0, workspace_bytes);
}

} // extern "C"
