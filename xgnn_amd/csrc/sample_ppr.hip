// sample_ppr.hip -- ppr_topk: per seed, the top-K nodes of an approximate personalised PageRank vector, by forward push
// (Andersen-Chung-Lang) in integer arithmetic (include/ggms.h; tests/ppr_ref.py restates the definition in numpy).
//
// There is no reference counterpart (PyG: torch_geometric.utils.ppr.get_ppr, numba on the CPU; ShaDow-GNN's PPR
// extractor; PPRGo).  random_walk's visit counts estimate the same vector by Monte Carlo with ~12 samples per seed; here
// the vector itself is pushed to a residual bound, synchronously: a round pushes every node whose residual is at or over
// eps * degree, with the values it had when the round began.  All arithmetic is uint32 / uint64 and every sum is a sum of
// integers, so no order of lanes, waves or atomics can change a bit of the result.
//
// One layer = two launches:
//   k_ppr_push   ONE WORKGROUP per seed, grid-stride under grid_for.  The seed's whole state lives in LDS: an
//                open-addressed table of 2C slots {key, r, p, list start, degree} (slot = fmix32(node) & (2C - 1), linear
//                probing) and the round's push list {slot, q, prefix of the active degrees}.  A round is
//                  scan    every lane reads its slots, finds the active ones, and two block scans give each its place in
//                          the push list and the exclusive prefix of its degree: the active lists laid end to end;
//                  insert  only if |map| + sum of active degrees > C (else the round surely fits): the positions of the
//                          lists, one per lane and tile, enter their keys; the count of new keys decides truncation.  A
//                          hub is cut by edge over the 256 lanes, not left to one (edge_tiles.h's idea in a workgroup);
//                  own     p += a, r = r - a - q d for every entry of the push list;
//                  add     the same walk over the positions: find (or, in a round that surely fits, enter) the key and
//                          add q to its r with an LDS integer atomic.
//                The degree and list start of a node are read from HBM once, by the lane that enters it.
//                Then the top K of {(p << 32) | ~node} over the table: the candidates are compacted over the (now dead)
//                start / degree words, the K-th largest key is found by a bitwise threshold search (62 block counts), the
//                <= 127 selected keys are ranked by counting and written K-strided to the staging, with the seed's count.
//   tile_scan    offsets of the counts in seed order, *num_out; its emit copies a seed's picks to their dense place.
// Every loop is bounded: max_rounds rounds, 2C probe steps, sum of degrees / 256 tiles.  No HBM atomic, no host round
// trip, no allocation.
#include "ggms_internal.h"
#include "labor_hash.h"
#include "tile_scan.h"

#include <cmath>

namespace ggms {

constexpr uint32_t kPprOne = 1u << 30;
constexpr uint32_t kPprMaxK = 127;

// LDS words of one workgroup: 5 table arrays of 2C, 3 push-list arrays of C (+ the prefix's end), kept even
static size_t ppr_lds_words(uint32_t C) { return 13 * (size_t)C + 2; }

struct PprParams {
  uint32_t A, E, C, max_rounds, K;
};

struct PprTable {
  uint32_t *start, *deg, *key, *r, *p; // 2C words each; start / deg first: the candidates' 64-bit keys reuse them
  uint32_t S;                          // 2C
};

// the slot of node v, entered if it is not there (its list bounds read by the lane that wins the slot).  kEmptyKey: the
// table is physically full -- more than C distinct nodes -- and *stop is raised
__device__ __forceinline__ uint32_t ppr_slot(const PprTable &t, const uint32_t *__restrict__ indptr, uint32_t v,
                                             uint32_t *num_new, uint32_t *stop) {
  uint32_t h = fmix32(v) & (t.S - 1u);
  for (uint32_t step = 0; step < t.S; ++step) {
    uint32_t k = __hip_atomic_load(t.key + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == kEmptyKey) {
      k = atomicCAS(t.key + h, kEmptyKey, v);
      if (k == kEmptyKey) {
        uint32_t b, e;
        GraphView::bounds(indptr, v, b, e);
        t.start[h] = b;
        t.deg[h] = e - b;
        atomicAdd(num_new, 1u);
        return h;
      }
    }
    if (k == v) return h;
    h = (h + 1u) & (t.S - 1u);
  }
  __hip_atomic_store(stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return kEmptyKey;
}

// the entry of the push list that position x of the concatenated active lists belongs to: the last e with pre[e] <= x
// (an entry of degree 0 has no position and is never the last one)
__device__ __forceinline__ uint32_t ppr_entry(const uint32_t *pre, uint32_t num, uint32_t x) {
  uint32_t lo = 0, hi = num; // pre[lo] <= x < pre[hi]  (pre[0] = 0, pre[num] = the total)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pre[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_ppr_push(const uint32_t *__restrict__ indptr,
                                                     const uint32_t *__restrict__ indices,
                                                     const uint32_t *__restrict__ input, Count n_arg, PprParams P,
                                                     uint32_t *__restrict__ stage_dst, uint32_t *__restrict__ stage_data,
                                                     uint32_t *__restrict__ count, uint32_t *__restrict__ out_stat) {
  extern __shared__ uint32_t lds[];
  __shared__ uint32_t s_scan[4], s_new, s_stop, s_ncand, s_nsel, s_sump, s_cnt[2][kBlock / kWave];
  __shared__ uint64_t s_sel[kPprMaxK + 1];
  const uint32_t C = P.C, S = 2u * C, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const PprTable t{lds, lds + S, lds + 2 * S, lds + 3 * S, lds + 4 * S, S};
  uint32_t *const pl_slot = lds + 5 * S, *const pl_q = pl_slot + C, *const pl_pre = pl_q + C; // pl_pre: C + 1 words
  uint64_t *const cand = reinterpret_cast<uint64_t *>(lds);                                   // 2C keys over start / deg
  const uint64_t n = n_arg.get();
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t seed = input[i];
    if (seed == kEmptyKey) { // yields nothing (uniform over the workgroup)
      if (tid == 0) {
        count[i] = 0;
        if (out_stat) { out_stat[2 * i] = 0; out_stat[2 * i + 1] = 0; }
      }
      continue;
    }
    for (uint32_t s = tid; s < S; s += kBlock) {
      t.key[s] = kEmptyKey;
      t.r[s] = 0;
      t.p[s] = 0;
    }
    if (tid == 0) s_ncand = s_nsel = s_sump = s_new = s_stop = 0;
    __syncthreads();
    if (tid == 0) {
      const uint32_t h = fmix32(seed) & (S - 1u);
      uint32_t b, e;
      GraphView::bounds(indptr, seed, b, e);
      t.key[h] = seed;
      t.r[h] = kPprOne;
      t.start[h] = b;
      t.deg[h] = e - b;
    }
    __syncthreads();
    uint32_t nmap = 1, rounds = 0, truncated = 0; // uniform
    for (uint32_t round = 0; round < P.max_rounds; ++round) {
      // ---- scan: who is active, where its entry and its list go
      uint32_t c = 0, ds = 0;
      for (uint32_t s = tid; s < S; s += kBlock) {
        if (t.key[s] == kEmptyKey) continue;
        const uint32_t r = t.r[s], d = t.deg[s];
        const bool act = d ? (uint64_t)r >= (uint64_t)P.E * d : r > 0u;
        c += act ? 1u : 0u;
        ds += act ? d : 0u;
      }
      uint32_t num_act, sum_deg; // active lists are disjoint ranges of `indices`: their sum fits 32 bits
      uint32_t at = block_exclusive_scan(c, s_scan, num_act);
      uint32_t pre = block_exclusive_scan(ds, s_scan, sum_deg);
      if (num_act == 0) break;
      for (uint32_t s = tid; s < S; s += kBlock) {
        if (t.key[s] == kEmptyKey) continue;
        const uint32_t r = t.r[s], d = t.deg[s];
        if (!(d ? (uint64_t)r >= (uint64_t)P.E * d : r > 0u)) continue;
        const uint32_t a = (uint32_t)(((uint64_t)P.A * r) >> 16);
        pl_slot[at] = s;
        pl_q[at] = d ? (r - a) / d : 0u;
        pl_pre[at] = pre;
        ++at;
        pre += d;
      }
      if (tid == 0) {
        pl_pre[num_act] = sum_deg;
        s_new = 0;
      }
      __syncthreads();
      // ---- insert: only a round that might not fit counts its new keys first
      const uint32_t room = C - nmap;
      if (sum_deg > room) {
        for (uint32_t x0 = 0; x0 < sum_deg; x0 += kBlock) {
          // enough is known: leaving early changes no decision (the count only grows)
          if (__hip_atomic_load(&s_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u ||
              __hip_atomic_load(&s_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > room)
            break;
          const uint32_t x = x0 + tid;
          if (x < sum_deg) {
            const uint32_t e = ppr_entry(pl_pre, num_act, x);
            const uint32_t v = indices[(uint64_t)t.start[pl_slot[e]] + (x - pl_pre[e])];
            ppr_slot(t, indptr, v, &s_new, &s_stop);
          }
        }
        __syncthreads();
        if (s_stop != 0u || s_new > room) { // the round does not happen (keys it entered hold r = p = 0: no effect)
          truncated = 1;
          break;
        }
      }
      // ---- own: the pushed nodes' side, from the values the round began with
      for (uint32_t e = tid; e < num_act; e += kBlock) {
        const uint32_t s = pl_slot[e], r = t.r[s], d = t.deg[s];
        const uint32_t a = d ? (uint32_t)(((uint64_t)P.A * r) >> 16) : r;
        t.p[s] += a;
        t.r[s] = r - a - pl_q[e] * d;
      }
      __syncthreads();
      // ---- add: q onto every position's node
      for (uint32_t x = tid; x < sum_deg; x += kBlock) {
        const uint32_t e = ppr_entry(pl_pre, num_act, x);
        const uint32_t v = indices[(uint64_t)t.start[pl_slot[e]] + (x - pl_pre[e])];
        const uint32_t h = ppr_slot(t, indptr, v, &s_new, &s_stop);
        if (h != kEmptyKey) atomicAdd(t.r + h, pl_q[e]); // (never full here: |map| + new <= C < 2C)
      }
      __syncthreads();
      nmap += s_new; // (s_new is cleared again behind the next round's scan barriers)
      ++rounds;
    }
    // ---- the candidates: every scored node but the seed, as (p << 32) | ~node, over the dead start / deg words
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t s = tid; s < S; s += kBlock) { // at most C scored nodes; the words written are not the ones read
      const uint32_t k = t.key[s], p = t.p[s];
      sum += p;
      if (k != kEmptyKey && k != seed && p != 0u) cand[atomicAdd(&s_ncand, 1u)] = ((uint64_t)p << 32) | (uint32_t)~k;
    }
    sum = wave_reduce_sum(sum);
    if (lane == 0) atomicAdd(&s_sump, sum);
    __syncthreads();
    const uint32_t ncand = s_ncand;
    uint64_t thr = 0; // the K-th largest key (keys are distinct), 0 = take all
    if (ncand > P.K) {
      for (int bit = 61; bit >= 0; --bit) { // p < 2^30: bits 62, 63 are clear
        const uint64_t trial = thr | (1ull << bit);
        uint32_t cc = 0;
        for (uint32_t j = tid; j < ncand; j += kBlock) cc += cand[j] >= trial ? 1u : 0u;
        cc = wave_reduce_sum(cc);
        if (lane == 0) s_cnt[bit & 1][wv] = cc;
        __syncthreads();
        uint32_t tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBlock / kWave; ++w) tot += s_cnt[bit & 1][w];
        if (tot >= P.K) thr = trial;
      }
    }
    for (uint32_t j = tid; j < ncand; j += kBlock) {
      const uint64_t key = cand[j];
      if (key >= thr) {
        const uint32_t o = atomicAdd(&s_nsel, 1u);
        if (o <= kPprMaxK) s_sel[o] = key;
      }
    }
    __syncthreads();
    const uint32_t take = s_nsel < P.K ? s_nsel : P.K;
    if (tid < take) {
      const uint64_t mine = s_sel[tid];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < take; ++j) rank += s_sel[j] > mine ? 1u : 0u;
      stage_dst[i * P.K + rank] = ~(uint32_t)mine;
      stage_data[i * P.K + rank] = (uint32_t)(mine >> 32);
    }
    if (tid == 0) {
      count[i] = take;
      if (out_stat) {
        out_stat[2 * i] = rounds | (truncated << 31);
        out_stat[2 * i + 1] = s_sump;
      }
    }
    __syncthreads(); // LDS is rewritten by the next seed
  }
}

struct PprCount {
  const uint32_t *count;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return count[i]; }
};
// a seed's picks, K-strided in the staging, to their dense place
struct PprEmit {
  const uint32_t *stage_dst, *stage_data, *input;
  uint32_t K;
  SrcMode sm;
  uint32_t *out_src, *out_dst, *out_data;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t v, uint32_t excl) const {
    if (v == 0u) return;
    const uint32_t sv = sm.local ? sm.value(0u, i) : input[i];
    for (uint32_t k = 0; k < v; ++k) {
      out_src[excl + k] = sv;
      out_dst[excl + k] = stage_dst[i * K + k];
      out_data[excl + k] = stage_data[i * K + k];
    }
  }
};

// staging (dst, data: n K each), the counts, a private scan area
size_t ppr_ws_words(size_t num_input, size_t K) { return 2 * num_input * K + num_input + tile_scan_words(num_input) + 48; }

// what include/ggms.h says ggms_sample_ppr refuses about the push itself; host arithmetic only
int ppr_check(double alpha, double eps, size_t max_nodes, size_t max_rounds, size_t K, const char *who) {
  if (!(alpha >= 0.05 && alpha <= 0.95)) {
    set_error("%s: alpha %g (0.05 .. 0.95)", who, alpha);
    return GGMS_ERR_INVALID;
  }
  if (!(eps >= 1.0 / 1048576.0 && eps <= 1.0)) {
    set_error("%s: eps %g (2^-20 .. 1)", who, eps);
    return GGMS_ERR_INVALID;
  }
  if (max_nodes < 64 || max_nodes > GGMS_PPR_MAX_NODES || (max_nodes & (max_nodes - 1)) != 0) {
    set_error("%s: max_nodes %zu (a power of two, 64 .. %u = GGMS_PPR_MAX_NODES: a seed's state is one workgroup's LDS)", who,
              max_nodes, (unsigned)GGMS_PPR_MAX_NODES);
    return GGMS_ERR_INVALID;
  }
  if (max_rounds < 1 || max_rounds > 255) {
    set_error("%s: max_rounds %zu (1 .. 255)", who, max_rounds);
    return GGMS_ERR_INVALID;
  }
  if (K < 1 || K > kPprMaxK || K >= max_nodes) {
    set_error("%s: K %zu (1 .. %u, below max_nodes)", who, K, (unsigned)kPprMaxK);
    return GGMS_ERR_INVALID;
  }
  return GGMS_OK;
}

void ppr_set(SampleLayer &l, double alpha, double eps, size_t max_nodes, size_t max_rounds) {
  l.ppr_a = (uint32_t)std::floor(alpha * 65536.0 + 0.5);
  l.ppr_e = (uint32_t)std::floor(eps * 1073741824.0);
  l.ppr_nodes = (uint32_t)max_nodes;
  l.ppr_rounds = (uint32_t)max_rounds;
}

int sample_ppr_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t K = (uint32_t)l.fanout;
  uint32_t *stage_dst = l.workspace;
  uint32_t *stage_data = stage_dst + n_max * K;
  uint32_t *count = stage_data + n_max * K;
  uint32_t *scan_scr = count + n_max + 16;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  static const int raised = raise_dynamic_lds(reinterpret_cast<const void *>(&k_ppr_push),
                                              ppr_lds_words(GGMS_PPR_MAX_NODES) * sizeof(uint32_t), "k_ppr_push");
  if (raised != GGMS_OK) return raised;
  const PprParams P{l.ppr_a, l.ppr_e, l.ppr_nodes, l.ppr_rounds, K};
  hipLaunchKernelGGL(k_ppr_push, dim3(grid_for(n_max, 1)), dim3(kBlock), ppr_lds_words(P.C) * sizeof(uint32_t), l.s,
                     l.g.indptr, l.g.indices, l.input, l.n, P, stage_dst, stage_data, count, l.out_stat);
  GGMS_LAUNCH_CHECK();
  return tile_scan(PprCount{count}, PprEmit{stage_dst, stage_data, l.input, K, l.src, l.out_src, l.out_dst, l.out_data},
                   n_max, l.n, sa, nullptr, nullptr, l.num_out, l.s);
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_sample_ppr_workspace_bytes(size_t num_input, size_t K) { return ppr_ws_words(num_input, K) * sizeof(uint32_t); }

int ggms_sample_ppr(const ggms_graph_t *graph, const ggms_id_t *input, size_t num_input, double alpha, double eps,
                    size_t max_nodes, size_t max_rounds, size_t K, ggms_id_t *out_src, ggms_id_t *out_dst,
                    ggms_id_t *out_data, uint64_t *num_out_dev, uint32_t *out_stat, void *workspace,
                    size_t workspace_bytes, ggms_stream_t stream) {
  static const char *const who = "ggms_sample_ppr";
  GGMS_CHECK_ARG(graph && num_out_dev);
  if (graph->num_part != 0) {
    set_error("%s: num_part %u: a seed's push reads ONE CSR, the call takes unsharded graphs only", who, graph->num_part);
    return GGMS_ERR_INVALID;
  }
  const int rc = ppr_check(alpha, eps, max_nodes, max_rounds, K, who);
  if (rc != GGMS_OK) return rc;
  if (num_input != 0 && workspace_bytes < ggms_sample_ppr_workspace_bytes(num_input, K)) {
    set_error("%s: workspace_bytes %zu, ggms_sample_ppr_workspace_bytes gives %zu", who, workspace_bytes,
              ggms_sample_ppr_workspace_bytes(num_input, K));
    return GGMS_ERR_INVALID;
  }
  SampleLayer l{graph, input, num_input, K, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.out_data = out_data;
  l.out_stat = out_stat;
  ppr_set(l, alpha, eps, max_nodes, max_rounds);
  return sample_leaf(GGMS_PPR_TOPK, l, 0, workspace_bytes);
}

} // extern "C"
