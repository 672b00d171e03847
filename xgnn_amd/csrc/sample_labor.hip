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
#include "labor_select.h"
#include "tile_scan.h"

namespace ggms {

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

// an edge of khop_labor: (seed's value, neighbour id) at the seed's offset + the rank inside the seed
struct LaborEmit {
  uint32_t *__restrict__ src, *__restrict__ dst; // out_src / out_dst + the seed's offset
  uint32_t sv;
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
  }
};

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
        labor_wave_select<1>(list, d, fanout, salt, LaborEmit{out_src + off, out_dst + off, sv});
      } else if (d <= kLaborWave4) {
        labor_wave_select<4>(list, d, fanout, salt, LaborEmit{out_src + off, out_dst + off, sv});
      } else {
        labor_wave_select<16>(list, d, fanout, salt, LaborEmit{out_src + off, out_dst + off, sv});
      }
    }
    rid = rid1;
    rid1 = rid2;
    d = d1;
    list = list1;
  }
}

__global__ __launch_bounds__(kBlock) void k_labor_hub(GraphView g, const uint32_t *__restrict__ input, uint32_t fanout,
                                                      uint32_t salt, const uint32_t *__restrict__ offset,
                                                      uint32_t *__restrict__ out_src, uint32_t *__restrict__ out_dst,
                                                      SrcMode sm, const uint32_t *heavy_count,
                                                      const uint32_t *__restrict__ heavy_list) {
  const uint32_t nh = *heavy_count;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = input[i];
    uint32_t d;
    const uint32_t *__restrict__ list = g.neighbours(rid, d);
    const uint32_t off = offset[i];
    labor_hub_list(list, d, fanout, salt, LaborEmit{out_src + off, out_dst + off, sm.value(rid, i)});
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
