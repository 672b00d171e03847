// sample_typed_temporal.hip -- khop_typed_temporal: a fanout per edge type, among the edges before a per-seed cut-off
// time, on a (type, time)-sorted CSR (include/ggms.h).
//
// Every edge position p carries a type edge_type[p] < R and a time edge_time[p].  Inside a node's list the types are
// non-decreasing and, inside a type's segment, the times: the list is sorted by the pair (type, time).  For a seed with
// cut c, "the edges of type r before c" are then a PREFIX of r's segment:
//   A_r = the first position with type >= r                          (khop_typed's b_r)
//   Z_r = the first position with (type, time) >= (r, c), lexicographically
//   e_r = Z_r - A_r, and the eligible positions are [A_r, Z_r).
// Each prefix is sampled with fanout k_r: khop_labor's rule on it (GGMS_PICK_UNIFORM: the min(k_r, e_r) smallest keys
// (fmix32(t_p ^ salt) << 32) | p, every segment under the same salt as in khop_typed) or its tail (GGMS_PICK_RECENT).
// Every edge leaves with its CSR position and its type.  R = 1 is khop_temporal, every cut = 0xffffffff is khop_typed.
//
// One layer = a 4-byte memset and four launches (+ the scan's own), as in sample_typed.hip and sample_temporal.hip:
//   k_tt_bounds  a GROUP of G = 2^ceil(log2 R) lanes per seed, lane r owns relation r.  d = 0 or c = 0 ends a seed before
//                its list is touched.  Else the four END loads go out together (type[0], type[d-1], time[0], time[d-1]:
//                the same four addresses for every lane of the group, one round trip) and settle what can be settled
//                without a search: an empty segment (type[d-1] < r or type[0] > r), a segment at the head (A_r = 0) or
//                the tail of the list, a list that lies wholly before or wholly behind (r, c) -- a one-relation list is
//                exactly khop_temporal's two time exits.  What is left runs TWO lower-bound searches advanced in the same
//                round: chain A over the type bytes, chain Z over the pairs, whose probe loads type[m] and time[m]
//                together.  Three independent loads per round, log2(d) round trips in all -- not log2(d) for the
//                segment and then log2(e) for its times.  At most 32 rounds.  Both chains only ever probe [1, d - 2].
//                A is made monotone by a prefix maximum over the group and Z_r is clamped into [A_r, A_{r+1}] (A_R = d):
//                a list that is not sorted gets SOME disjoint ranges inside [0, d).
//                Out: the record of the seed, 2 R consecutive words A_0 .. A_{R-1}, e_0 .. e_{R-1}; its cut; its count,
//                sum_r min(k_r, e_r), summed over the group.
//   tile_scan    offset[i] = the sum of the counts of the seeds before i; *num_out = the edge count.
//   k_tt_select  one WAVE per seed; a seed whose count is 0 costs one 4-byte load.  Else the record is ONE coalesced load
//                (lane r: A_r, lane 32 + r: e_r) and the wave walks the relations with a running offset, routing each by
//                e_r (3 past edges of a rare relation in a 40 000-entry hub are a copy): RECENT or e_r <= k_r a
//                contiguous copy, else labor_wave_select<1 / 4 / 16>.  A seed with a longer prefix is listed for
//   k_tt_hub     one WORKGROUP per listed seed: labor_hub_list on its long prefixes, one after the other.  Not launched
//                for RECENT, which lists nothing.
// In a batch (ggms_sample_batch_typed_temporal) every emitted edge f -> t lowers t's cut to f's, khop_temporal's 64-bit
// atomicMax on the cut table; k_tt_bounds is the only reader of the table and runs in front of the launches that write.
#include "cut_word.h"
#include "ggms_internal.h"
#include "labor_select.h"
#include "tile_scan.h"
#include "type_fanouts.h"

namespace ggms {

__global__ __launch_bounds__(kBlock) void k_tt_bounds(const uint32_t *__restrict__ indptr,
                                                      const uint8_t *__restrict__ edge_type,
                                                      const uint32_t *__restrict__ edge_time,
                                                      const uint32_t *__restrict__ input,
                                                      const uint32_t *__restrict__ input_cut,
                                                      const unsigned long long *cut_table, uint32_t stamp, Count n_arg,
                                                      TypeFanouts f, uint32_t R, uint32_t gshift,
                                                      uint32_t *__restrict__ record, uint32_t *__restrict__ c_out,
                                                      uint32_t *__restrict__ count) {
  const uint64_t n = n_arg.get();
  const int G = 1 << gshift;
  const uint32_t per_block = (uint32_t)kBlock >> gshift;
  const uint32_t r = threadIdx.x & (uint32_t)(G - 1), sub = threadIdx.x >> gshift;
  const uint32_t kr = r < R ? f.get(r) : 0u;
  // the round loop is uniform over the workgroup: every lane of a group takes part in the group's shuffles
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < n; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t i = base + sub;
    uint32_t c = 0, d = 0, b0 = 0;
    if (i < n) {
      const uint32_t s = input[i];
      c = input_cut ? input_cut[i] : cut_of_word(cut_table[s], stamp);
      uint32_t end;
      GraphView::bounds(indptr, s, b0, end);
      d = end - b0;
    }
    // the lanes behind R hold A = Z = d: the prefix maximum leaves them there, and lane R - 1 reads A_R = d from them
    uint32_t A = r < R ? 0u : d, Z = A;
    if (r < R && d != 0 && c != 0) {
      const uint8_t *__restrict__ type = edge_type + b0;
      const uint32_t *__restrict__ time = edge_time + b0;
      const uint32_t t0 = type[0], tl = type[d - 1], m0 = time[0], ml = time[d - 1]; // in flight together
      const bool less0 = t0 < r || (t0 == r && m0 < c); // (type, time)[0] < (r, c)
      const bool lessl = tl < r || (tl == r && ml < c);
      // chain A: the first p with type[p] >= r, in [lo1, hi1]; chain Z: the first p with (type, time)[p] >= (r, c), in
      // [lo2, hi2].  Searched: type[0] < r <= type[d-1], resp. pair[0] < (r, c) <= pair[d-1] -- sorted lists keep that
      // to the end; any list: 1 <= lo <= hi <= d - 1 and every probe m has lo <= m < hi
      uint32_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
      if (tl < r) lo1 = hi1 = d;
      else if (t0 < r) lo1 = 1u, hi1 = d - 1u;
      if (lessl) lo2 = hi2 = d;
      else if (less0) lo2 = 1u, hi2 = d - 1u;
      for (uint32_t round = 0; round < 32u; ++round) {
        const bool a1 = lo1 < hi1, a2 = lo2 < hi2;
        if (!a1 && !a2) break;
        const uint32_t p1 = lo1 + ((hi1 - lo1) >> 1), p2 = lo2 + ((hi2 - lo2) >> 1);
        const uint32_t y1 = a1 ? type[p1] : 0u, y2 = a2 ? type[p2] : 0u, x2 = a2 ? time[p2] : 0u; // three loads together
        if (a1) { if (y1 < r) lo1 = p1 + 1u; else hi1 = p1; }
        if (a2) { if (y2 < r || (y2 == r && x2 < c)) lo2 = p2 + 1u; else hi2 = p2; }
      }
      A = lo1;
      Z = lo2;
    }
    // A_r = max(A_r, A_{r-1}): an inclusive prefix maximum over the group
    for (int off = 1; off < G; off <<= 1) {
      const uint32_t y = __shfl_up(A, off, G);
      A = y > A ? y : A;
    }
    uint32_t nextA = __shfl_down(A, 1, G);
    if (r + 1u >= (uint32_t)G) nextA = d;
    Z = Z < A ? A : (Z > nextA ? nextA : Z); // A_r <= Z_r <= A_{r+1} <= d
    const uint32_t e = Z - A;
    uint32_t cnt = e < kr ? e : kr;
    for (int off = G >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, G);
    if (i < n && r < R) {
      uint32_t *__restrict__ rec = record + (size_t)i * (2u * R);
      rec[r] = A;
      rec[R + r] = e;
    }
    if (i < n && r == 0) {
      c_out[i] = c;
      count[i] = cnt;
    }
  }
}

struct TTCount {
  const uint32_t *count;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return count[i]; }
};
struct TTOffset {
  uint32_t *offset;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t, uint32_t excl) const { offset[i] = excl; }
};

// an edge of khop_typed_temporal: khop_typed's four words, and in a batch khop_temporal's lowering of the neighbour's cut
struct TTEmit {
  uint32_t *__restrict__ src, *__restrict__ dst, *__restrict__ pos; // the outputs + the seed's offset + the relations before
  uint8_t *__restrict__ type;
  uint32_t sv, begin; // begin = indptr[seed] + A_r
  uint32_t r;
  unsigned long long *cut_table; // NULL: a leaf call
  unsigned long long word;       // cut_word(stamp, the seed's cut)
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t p, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
    pos[o] = begin + p;
    type[o] = (uint8_t)r;
    if (cut_table) atomicMax(cut_table + t, word);
  }
};

struct TTArgs {
  const uint32_t *indptr, *indices, *input;
  const uint32_t *record, *count, *c, *offset;
  uint32_t *out_src, *out_dst, *out_pos;
  uint8_t *out_type;
  unsigned long long *cut_table;
  TypeFanouts f;
  uint32_t R, salt, stamp, recent;
  SrcMode sm;
  __device__ __forceinline__ TTEmit emit_of(uint32_t at, uint32_t sv, uint32_t begin, uint32_t r,
                                            unsigned long long word) const {
    return TTEmit{out_src + at, out_dst + at, out_pos + at, out_type + at, sv, begin, r, cut_table, word};
  }
  __device__ __forceinline__ unsigned long long word_of(uint64_t i) const {
    return cut_table ? cut_word(stamp, c[i]) : 0ull;
  }
};

__global__ __launch_bounds__(kBlock) void k_tt_select(TTArgs a, Count n_arg, uint32_t *heavy_count,
                                                      uint32_t *__restrict__ heavy_list) {
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t R = a.R;
  // lane r reads word r of the record (A_r), lane 32 + r word R + r (e_r): 2 R consecutive words, one request
  const uint32_t slot = lane & 31u, word_at = lane < 32u ? slot : R + slot;
  // the count is known without touching the graph: the id, the list head and the record of a seed are only requested
  // where something will be emitted
  uint32_t cnt = wave < n ? a.count[wave] : 0u;
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t cnt1 = i + waves < n ? a.count[i + waves] : 0u;
    if (cnt != 0) {
      const uint32_t rv = slot < R ? a.record[(size_t)i * (2u * R) + word_at] : 0u;
      const uint32_t rid = a.input[i];
      const uint32_t begin = a.indptr[rid];
      const uint32_t sv = a.sm.value(rid, i);
      const unsigned long long word = a.word_of(i);
      uint32_t at = a.offset[i];
      bool heavy = false;
      for (uint32_t r = 0; r < R; ++r) {
        const uint32_t A = (uint32_t)__builtin_amdgcn_readlane((int)rv, (int)r);
        const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)rv, (int)(32u + r));
        const uint32_t k = a.f.get(r);
        if (k != 0 && e != 0) { // uniform over the wave: the selection's ballots see all 64 lanes
          const uint32_t *__restrict__ list = a.indices + ((size_t)begin + A);
          const TTEmit emit = a.emit_of(at, sv, begin + A, r, word);
          if (a.recent || e <= k) { // a contiguous run: the whole prefix, or its last k positions
            const uint32_t m = e < k ? e : k, first = e - m;
            for (uint32_t o = lane; o < m; o += kWave) emit(o, first + o, list[first + o]);
          } else if (e <= kLaborWave1) {
            labor_wave_select<1>(list, e, k, a.salt, emit);
          } else if (e <= kLaborWave4) {
            labor_wave_select<4>(list, e, k, a.salt, emit);
          } else if (e <= kLaborWaveMax) {
            labor_wave_select<16>(list, e, k, a.salt, emit);
          } else {
            heavy = true; // a workgroup's prefix
          }
          at += e < k ? e : k;
        }
      }
      if (heavy && lane == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)i;
    }
    cnt = cnt1;
  }
}

__global__ __launch_bounds__(kBlock) void k_tt_hub(TTArgs a, const uint32_t *heavy_count,
                                                   const uint32_t *__restrict__ heavy_list) {
  const uint32_t nh = *heavy_count;
  const uint32_t R = a.R;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t *__restrict__ rec = a.record + (size_t)i * (2u * R);
    const uint32_t rid = a.input[i];
    const uint32_t begin = a.indptr[rid];
    const uint32_t sv = a.sm.value(rid, i);
    const unsigned long long word = a.word_of(i);
    uint32_t at = a.offset[i];
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t A = rec[r], e = rec[R + r], k = a.f.get(r);
      if (k != 0 && e != 0) {
        if (e > k && e > kLaborWaveMax)
          labor_hub_list(a.indices + ((size_t)begin + A), e, k, a.salt, a.emit_of(at, sv, begin + A, r, word));
        at += e < k ? e : k;
      }
    }
  }
}

// offset, heavy list, count, cut: n words each; the records: 2 R words per seed; the heavy counter; a private scan area.
// num_type 0 (a caller that does not know it): sized for GGMS_MAX_EDGE_TYPES
size_t typed_temporal_ws_words(size_t num_input, size_t num_type) {
  const size_t R = num_type >= 1 && num_type <= GGMS_MAX_EDGE_TYPES ? num_type : GGMS_MAX_EDGE_TYPES;
  return (4 + 2 * R) * num_input + tile_scan_words(num_input) + 48;
}

int sample_khop_typed_temporal_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t R = l.num_type;
  uint32_t *offset = l.workspace;
  uint32_t *heavy_list = offset + n_max;
  uint32_t *count = heavy_list + n_max;
  uint32_t *c = count + n_max;
  uint32_t *record = c + n_max;
  uint32_t *heavy_count = record + 2 * (size_t)R * n_max;
  uint32_t *scan_scr = heavy_count + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  const TypeFanouts f = type_fanouts_of(l.type_fanout, R);
  uint32_t gshift = 0;
  while ((1u << gshift) < R) ++gshift;
  unsigned long long *cut_table = reinterpret_cast<unsigned long long *>(l.cut_table);
  const bool recent = l.pick == GGMS_PICK_RECENT;
  GGMS_HIP(hipMemsetAsync(heavy_count, 0, sizeof(uint32_t), l.s));
  hipLaunchKernelGGL(k_tt_bounds, dim3(grid_for(n_max, (size_t)kBlock >> gshift)), dim3(kBlock), 0, l.s, l.g.indptr,
                     l.edge_type, l.edge_time, l.input, l.input_cut, cut_table, l.stamp, l.n, f, R, gshift, record, c, count);
  int rc = tile_scan(TTCount{count}, TTOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out, l.s);
  if (rc != GGMS_OK) return rc;
  const TTArgs a{l.g.indptr, l.g.indices, l.input, record, count, c, offset, l.out_src, l.out_dst, l.out_pos, l.out_type,
                 cut_table, f, R, l.salt, l.stamp, recent ? 1u : 0u, l.src};
  hipLaunchKernelGGL(k_tt_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, a, l.n, heavy_count,
                     heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device (RECENT lists none)
  if (!recent) hipLaunchKernelGGL(k_tt_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, a, heavy_count, heavy_list);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_sample_khop_typed_temporal_workspace_bytes(size_t num_input, uint32_t num_type) {
  if (num_type < 1 || num_type > GGMS_MAX_EDGE_TYPES) return 0;
  return typed_temporal_ws_words(num_input, num_type) * sizeof(uint32_t);
}

int ggms_sample_khop_typed_temporal(const ggms_graph_t *graph, const uint8_t *edge_type, const uint32_t *edge_time,
                                    uint32_t num_type, const uint32_t *type_fanout, const ggms_id_t *input,
                                    const uint32_t *input_cut, size_t num_input, int pick, uint32_t layer_salt,
                                    ggms_id_t *out_src, ggms_id_t *out_dst, ggms_id_t *out_pos, uint8_t *out_type,
                                    uint64_t *num_out_dev, void *workspace, size_t workspace_bytes,
                                    ggms_stream_t stream) {
  size_t K = 0;
  const int rc = typed_fanout_sum(type_fanout, num_type, &K);
  if (rc != GGMS_OK) return rc;
  SampleLayer l{graph, input, num_input, K, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  l.edge_type = edge_type;
  l.edge_time = edge_time;
  l.input_cut = input_cut;
  l.num_type = num_type;
  l.type_fanout = type_fanout;
  l.pick = pick;
  l.out_pos = out_pos;
  l.out_type = out_type;
  GGMS_CHECK_ARG(pick == GGMS_PICK_UNIFORM || pick == GGMS_PICK_RECENT);
  GGMS_CHECK_ARG(num_input == 0 || (edge_type && edge_time && input_cut && out_pos && out_type));
  return sample_leaf(GGMS_KHOP_TYPED_TEMPORAL, l, 0, workspace_bytes);
}

} // extern "C"
