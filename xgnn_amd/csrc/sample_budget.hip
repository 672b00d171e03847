// sample_budget.hip -- khop_budget: layer-wise importance sampling under a hard node budget per layer (include/ggms.h).
//
// FastGCN / LADIES / HGSampling: a layer draws S nodes for the WHOLE frontier, a candidate's chance grows with how much
// of the frontier points at it, and the frontier keeps its edges into the chosen set (a seed at most `fanout` of them,
// so the batch chain's capacities hold).  There is no reference counterpart; tests/khop_budget_ref.py restates the
// definition in numpy and the result equals it bit for bit: weights are 64-bit integer sums, the variate is
// khop_labor_weighted's integer E(t), the key one IEEE division, and every choice is a comparison of distinct keys.
//
// One layer is a fixed chain of launches (their number depends on num_node alone); every count stays on the device:
//   memset               the control block, the digit histograms, the per-seed counts (one contiguous piece)
//   tile_scan            pre[i] = list entries of the seeds before i, cw[i] = the seed's contribution c_i (one 64-bit
//                        division per SEED, in the scan's emit); the total E stays on the device
//   k_budget_accumulate  the edge-tiled walk (edge_tiles.h).  A round's 2048 entries first meet in an LDS table of
//                        kCombSlots (tag, 64-bit sum) slots -- ds_cmpst + ds_add_u64 -- so that a hub candidate hit by
//                        many seeds of a tile costs ONE memory-side atomic per round instead of one per hit WHERE it
//                        holds its slot (atomics on one address are served one after the other); no probing: an entry
//                        whose slot is taken by another id goes to memory directly.  The returning 64-bit add on map[t] tells the first toucher (old == 0: every
//                        contribution is >= 1), first touchers are gathered in LDS and appended to the candidate list
//                        with one counter atomic per round, not one per candidate
//   k_budget_keys        key32 of every candidate (log table in LDS) + the histogram of the first digit
//   k_budget_hist x (P-1) MSB-first selection of the S-th smallest key: 11-bit digits of (key32 << tb) | t, tb = the bits
//                        of a node id.  Every workgroup derives the previous pass's digit and remaining rank from the
//                        global histogram itself (2048 counters, one block scan) instead of a single-workgroup launch
//                        between two passes; workgroup 0 records the state for the pass after.  Histograms are per
//                        workgroup in LDS, flushed with integer adds.  M <= S: every pass falls through
//   k_budget_mark        the last digit; map[t] = {chosen, key32} or "rejected": the per-seed stage reads ONE word per entry
//   k_budget_count       the walk again: eligible entries per seed.  Owners run in order inside a wave, so a run of equal
//                        owners adds once (two ballots); a hub spread over many tiles costs an atomic per wave
//   tile_scan            offset[i] = sum of min(fanout, eligible) before i; the edge count
//   k_budget_select      one WAVE per seed up to kLaborWaveMax entries: map words of the whole list in registers,
//                        labor_select.h's ballot / popcount threshold search over key32 with ineligible entries masked
//   k_budget_hub         one WORKGROUP per longer list: the eligible (key32, position) pairs are staged in LDS
//                        (kHubCand), the k-th smallest found by the bitwise search there; more eligible entries than the
//                        buffer holds: the exact route over the list itself, as labor_hub_list's
//   k_budget_restore     map[t] = 0 through the candidate list: the map is clean again at the cost of the layer
// The candidate list's order depends on the run (who touches a word first); nothing else does: keys are distinct and
// every output position comes from a scan or a rank.
#include "edge_tiles.h"
#include "ggms_internal.h"
#include "labor_log2_table.h"
#include "labor_select.h"

namespace ggms {

namespace {

constexpr uint32_t kDigitBits = 11, kRadix = 1u << kDigitBits;
constexpr uint32_t kMaxPass = 6;       // ceil(64 / 11)
constexpr uint32_t kSelTile = 2048;    // candidates per workgroup round of the selection passes
constexpr uint32_t kCombSlots = 2048;  // LDS combining table of the accumulate walk: a slot per entry of a round
constexpr uint32_t kHubCand = 4096;    // eligible (key32, position) pairs the hub's LDS buffer holds (32 KB)
constexpr unsigned long long kChosen = 1ull << 32, kRejected = 2ull << 32; // map word after the mark: flag | key32

struct BudgetState {
  uint64_t prefix; // the digits picked so far
  uint32_t rank;   // the rank still looked for among the keys under that prefix (1-based)
  uint32_t all;    // M <= S: every candidate is chosen
};
struct BudgetCtl {
  uint64_t E;    // list entries of the frontier
  uint32_t M;    // candidates appended (may exceed the capacity: readers clamp)
  uint32_t heavy;
  uint32_t over; // the frontier's list entries total 2^32 or more: nothing is walked, GGMS_STATUS_TABLE_FULL is set
  uint32_t _pad[3];
  BudgetState st[kMaxPass]; // st[p] = after the picks of passes 0 .. p
};

// the selection's key: (key32 << tb) | t, `bits` = 32 + tb significant bits, cut MSB-first into `passes` digits
struct KeyPlan {
  uint32_t tb, bits, passes;
  __host__ __device__ __forceinline__ uint32_t hi(uint32_t p) const { return bits - kDigitBits * p; }
  __host__ __device__ __forceinline__ uint32_t lo(uint32_t p) const { return hi(p) > kDigitBits ? hi(p) - kDigitBits : 0u; }
  __device__ __forceinline__ uint64_t key(uint32_t key32, uint32_t t) const { return ((uint64_t)key32 << tb) | t; }
  __device__ __forceinline__ uint32_t digit(uint64_t key, uint32_t p) const {
    return (uint32_t)(key >> lo(p)) & ((1u << (hi(p) - lo(p))) - 1u);
  }
};
KeyPlan key_plan(uint32_t num_node) {
  uint32_t tb = 1;
  while (tb < 32 && (((uint64_t)num_node - 1) >> tb) != 0) ++tb;
  return KeyPlan{tb, 32 + tb, (32 + tb + kDigitBits - 1) / kDigitBits};
}

// scan pieces: degree of seed i -> pre[i], cw[i]
struct BudgetPrefix {
  uint32_t *pre;
  uint64_t *cw; // NULL: uniform
  uint32_t *over;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t d, uint32_t excl) const {
    pre[i] = excl;
    // the first seed at which the running total passes 2^32 still sees an exact prefix: its 32-bit sum wraps
    if ((uint32_t)(excl + d) < excl) *over = 1u;
    if (cw) {
      uint64_t c = 1;
      if (d != 0 && d < (1u << 20)) {
        c = (1ull << 40) / ((uint64_t)d * d);
        c = c ? c : 1;
      }
      cw[i] = c;
    }
  }
};
struct BudgetCount {
  const uint32_t *cnt;
  uint32_t fanout;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return cnt[i] < fanout ? cnt[i] : fanout; }
};

__device__ __forceinline__ uint32_t cand_count(const BudgetCtl *ctl, uint32_t cap) { return ctl->M < cap ? ctl->M : cap; }

// The state after the picks of passes 0 .. done - 1, by the whole workgroup (the same value in every thread): the
// recorded state of the pass before + the global histogram of pass done - 1.  s_scan: 4 words
__device__ __forceinline__ BudgetState budget_state(const BudgetCtl *ctl, const uint32_t *__restrict__ hist, uint32_t done,
                                                    uint64_t S, uint32_t cap, const KeyPlan &kp, uint32_t *s_scan,
                                                    BudgetState *s_st) {
  const uint32_t M = cand_count(ctl, cap);
  BudgetState st{0, (uint32_t)(S < 0xffffffffull ? S : 0xffffffffull), M <= S ? 1u : 0u};
  if (done == 0 || st.all) return st;
  if (done >= 2) st = ctl->st[done - 2];
  const uint32_t p = done - 1;
  const uint32_t *h = hist + (size_t)p * kRadix + threadIdx.x * 8u;
  uint32_t c[8], sum = 0;
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    c[b] = h[b];
    sum += c[b];
  }
  if (threadIdx.x == 0) *s_st = st; // (kept if no bin holds the rank: cannot happen with consistent counts)
  uint32_t total;
  uint32_t run = block_exclusive_scan(sum, s_scan, total);
  if (run < st.rank && st.rank <= run + sum) {
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      if (run < st.rank && st.rank <= run + c[b])
        *s_st = BudgetState{(st.prefix << (kp.hi(p) - kp.lo(p))) | (threadIdx.x * 8u + b), st.rank - run, 0u};
      run += c[b];
    }
  }
  __syncthreads();
  return *s_st;
}

__global__ __launch_bounds__(kBlock) void k_budget_accumulate(GraphView g, const uint32_t *__restrict__ input, Count n_arg,
                                                              const uint32_t *__restrict__ pre,
                                                              const uint64_t *__restrict__ cw, BudgetCtl *ctl,
                                                              unsigned long long *map, uint32_t num_node,
                                                              uint32_t *__restrict__ cand, uint32_t cap) {
  __shared__ uint32_t s_tag[kCombSlots];
  __shared__ unsigned long long s_sum[kCombSlots];
  __shared__ uint32_t s_first[kEdgeTile];
  __shared__ uint32_t s_nfirst, s_base;
  for (uint32_t s = threadIdx.x; s < kCombSlots; s += kBlock) {
    s_tag[s] = kEmptyKey;
    s_sum[s] = 0;
  }
  if (threadIdx.x == 0) s_nfirst = 0;
  __syncthreads();
  const uint64_t F = n_arg.get();
  const uint64_t E = ctl->over ? 0ull : ctl->E;
  walk_edge_tiles_where(
      g, input, F, pre, E, num_node,
      [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t, const uint32_t (&own)[kPerThread],
          const uint32_t *const (&)[kPerThread]) {
        uint64_t c[kPerThread];
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; ++k) c[k] = (cw && ((have >> k) & 1u)) ? cw[own[k]] : 1ull;
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; ++k) {
          if (!((have >> k) & 1u) || v[k] >= num_node) continue;
          const uint32_t slot = (v[k] * 0x9e3779b1u) >> 21; // 11 bits: kCombSlots
          const uint32_t old = atomicCAS(&s_tag[slot], kEmptyKey, v[k]);
          if (old == kEmptyKey || old == v[k]) {
            atomicAdd(&s_sum[slot], (unsigned long long)c[k]);
          } else if (atomicAdd(map + v[k], (unsigned long long)c[k]) == 0ull) {
            s_first[atomicAdd(&s_nfirst, 1u)] = v[k];
          }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < kCombSlots; s += kBlock) {
          const uint32_t t = s_tag[s];
          if (t == kEmptyKey) continue;
          if (atomicAdd(map + t, s_sum[s]) == 0ull) s_first[atomicAdd(&s_nfirst, 1u)] = t;
          s_tag[s] = kEmptyKey;
          s_sum[s] = 0;
        }
        __syncthreads();
        const uint32_t nf = s_nfirst; // at most one per entry of the round: <= kEdgeTile
        if (threadIdx.x == 0 && nf != 0) s_base = atomicAdd(&ctl->M, nf);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nf; j += kBlock) {
          const uint64_t at = (uint64_t)s_base + j;
          if (at < cap) cand[at] = s_first[j];
        }
        if (threadIdx.x == 0) s_nfirst = 0; // (read by every thread before the barrier above; the walk's own barrier
                                            // stands between this round's reads of s_first and the next round's writes)
      });
}
static_assert(kCombSlots == 1u << 11, "the slot hash keeps 11 bits");

__global__ __launch_bounds__(kBlock) void k_budget_keys(BudgetCtl *ctl, uint32_t *hist, const uint32_t *__restrict__ cand,
                                                        uint32_t *__restrict__ cand_key, uint32_t cap,
                                                        const unsigned long long *__restrict__ map, uint64_t S,
                                                        uint32_t salt, KeyPlan kp, uint32_t *status) {
  __shared__ uint64_t s_T[kLaborLogEntries];
  __shared__ uint32_t s_h[kRadix];
  for (uint32_t d = threadIdx.x; d < kRadix; d += kBlock) s_h[d] = 0;
  load_log_table(s_T);
  const uint32_t M = cand_count(ctl, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0 && (ctl->M > cap || ctl->over)) atomicOr(status, kErrTableFull);
  const bool all = M <= S;
  for (uint64_t base = (uint64_t)blockIdx.x * kSelTile; base < M; base += (uint64_t)gridDim.x * kSelTile) {
    uint32_t t[kSelTile / kBlock];
    unsigned long long W[kSelTile / kBlock];
#pragma unroll
    for (uint32_t u = 0; u < kSelTile / kBlock; ++u) {
      const uint64_t j = base + u * kBlock + threadIdx.x;
      t[u] = j < M ? cand[j] : 0u;
      W[u] = j < M ? map[t[u]] : 1ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < kSelTile / kBlock; ++u) {
      const uint64_t j = base + u * kBlock + threadIdx.x;
      if (j >= M) continue;
      const uint32_t key32 = __float_as_uint((float)labor_exp_units(t[u], salt, s_T) / (float)W[u]);
      cand_key[j] = key32;
      if (!all) atomicAdd(&s_h[kp.digit(kp.key(key32, t[u]), 0)], 1u);
    }
  }
  __syncthreads();
  if (all) return;
  for (uint32_t d = threadIdx.x; d < kRadix; d += kBlock)
    if (s_h[d]) atomicAdd(hist + d, s_h[d]);
}

// pass p >= 1: the digit p of the candidates under the prefix of passes 0 .. p - 1
__global__ __launch_bounds__(kBlock) void k_budget_hist(BudgetCtl *ctl, uint32_t *hist, const uint32_t *__restrict__ cand,
                                                        const uint32_t *__restrict__ cand_key, uint32_t cap, uint64_t S,
                                                        KeyPlan kp, uint32_t p) {
  __shared__ uint32_t s_h[kRadix];
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ BudgetState s_st;
  for (uint32_t d = threadIdx.x; d < kRadix; d += kBlock) s_h[d] = 0;
  const BudgetState st = budget_state(ctl, hist, p, S, cap, kp, s_scan, &s_st);
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->st[p - 1] = st;
  if (st.all) return; // uniform
  __syncthreads();
  const uint32_t M = cand_count(ctl, cap);
  const uint32_t hi = kp.hi(p); // < 64: p >= 1
  for (uint64_t base = (uint64_t)blockIdx.x * kSelTile; base < M; base += (uint64_t)gridDim.x * kSelTile) {
#pragma unroll
    for (uint32_t u = 0; u < kSelTile / kBlock; ++u) {
      const uint64_t j = base + u * kBlock + threadIdx.x;
      if (j >= M) continue;
      const uint64_t key = kp.key(cand_key[j], cand[j]);
      if ((key >> hi) == st.prefix) atomicAdd(&s_h[kp.digit(key, p)], 1u);
    }
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < kRadix; d += kBlock)
    if (s_h[d]) atomicAdd(hist + (size_t)p * kRadix + d, s_h[d]);
}

__global__ __launch_bounds__(kBlock) void k_budget_mark(BudgetCtl *ctl, const uint32_t *hist,
                                                        const uint32_t *__restrict__ cand,
                                                        const uint32_t *__restrict__ cand_key, uint32_t cap,
                                                        unsigned long long *__restrict__ map, uint64_t S, KeyPlan kp,
                                                        uint64_t *stat) {
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ BudgetState s_st;
  const BudgetState st = budget_state(ctl, hist, kp.passes, S, cap, kp, s_scan, &s_st); // prefix = the S-th smallest key
  const uint32_t M = cand_count(ctl, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0 && stat) {
    stat[0] = M;
    stat[1] = st.all ? (uint64_t)M : S;
  }
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < M; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t t = cand[j], key32 = cand_key[j];
    map[t] = (st.all || kp.key(key32, t) <= st.prefix) ? (kChosen | key32) : kRejected;
  }
}

__global__ __launch_bounds__(kBlock) void k_budget_restore(const BudgetCtl *ctl, const uint32_t *__restrict__ cand,
                                                           uint32_t cap, unsigned long long *__restrict__ map) {
  const uint32_t M = cand_count(ctl, cap);
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < M; j += (uint64_t)gridDim.x * kBlock) map[cand[j]] = 0ull;
}

__global__ __launch_bounds__(kBlock) void k_budget_count(GraphView g, const uint32_t *__restrict__ input, Count n_arg,
                                                         const uint32_t *__restrict__ pre, const BudgetCtl *ctl,
                                                         const unsigned long long *__restrict__ map, uint32_t num_node,
                                                         uint32_t *cnt) {
  const uint64_t F = n_arg.get();
  const uint64_t E = ctl->over ? 0ull : ctl->E;
  const uint32_t lane = lane_id();
  walk_edge_tiles_where(g, input, F, pre, E, num_node,
                        [&](const uint32_t (&v)[kPerThread], uint32_t have, uint64_t, const uint32_t (&own)[kPerThread],
                            const uint32_t *const (&)[kPerThread]) {
                          unsigned long long m[kPerThread];
#pragma unroll
                          for (uint32_t k = 0; k < kPerThread; ++k)
                            m[k] = (((have >> k) & 1u) && v[k] < num_node) ? map[v[k]] : 0ull;
#pragma unroll
                          for (uint32_t k = 0; k < kPerThread; ++k) {
                            const uint64_t eb = __ballot((m[k] & kChosen) != 0ull);
                            if (eb == 0ull) continue; // uniform over the wave
                            // the lanes that hold entries are a prefix of the wave and their owners ascend: a lane
                            // heads a run if its owner differs from the lane before
                            const bool valid = (have >> k) & 1u;
                            const uint32_t prev = __shfl_up(own[k], 1, 64);
                            const bool head = valid && (lane == 0 || prev != own[k]);
                            const uint64_t hb = __ballot(head);
                            const uint64_t above = hb & ~((2ull << lane) - 1ull); // heads past this lane
                            const uint64_t upto = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull;
                            const uint32_t c = (uint32_t)__popcll(eb & upto & ~((1ull << lane) - 1ull));
                            if (head && c != 0) atomicAdd(cnt + own[k], c);
                          }
                        });
}

// an edge of khop_budget: khop_labor's (seed's value, neighbour id) and the edge's CSR position
struct BudgetEmit {
  uint32_t *__restrict__ src, *__restrict__ dst, *__restrict__ pos; // the outputs + the seed's offset
  uint32_t sv, begin;                                                // begin = indptr[seed]
  __device__ __forceinline__ void operator()(uint32_t o, uint32_t p, uint32_t t) const {
    src[o] = sv;
    dst[o] = t;
    pos[o] = begin + p;
  }
};

struct BudgetArgs {
  GraphView g; // one CSR: a list's first position is list - g.indices
  const unsigned long long *map;
  const uint32_t *input, *offset, *cnt;
  uint32_t *out_src, *out_dst, *out_pos;
  uint32_t fanout, num_node;
  SrcMode sm;
  __device__ __forceinline__ BudgetEmit emit_of(uint64_t i, uint32_t rid, uint32_t begin) const {
    const uint32_t off = offset[i];
    return BudgetEmit{out_src + off, out_dst + off, out_pos + off, sm.value(rid, i), begin};
  }
  // the map word of a list entry: 0 for an id out of range (never eligible)
  __device__ __forceinline__ unsigned long long word(uint32_t t) const { return t < num_node ? map[t] : 0ull; }
};

// 0 < d <= 64 R, e = the list's eligible entries: the map words of the whole list in the wave's registers, position
// p = 64 r + lane.  e <= k: the eligible entries in order; else labor_wave_select's search over key32 with the
// ineligible entries masked (a copy of its search, tie logic and emit: a fix there belongs here too)
template <int R>
__device__ __forceinline__ void budget_wave_select(const BudgetArgs &a, const uint32_t *__restrict__ list, uint32_t d,
                                                   uint32_t k, uint32_t e, const BudgetEmit &emit) {
  const uint32_t lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t t[R], key[R], in = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = 64u * r + lane;
    t[r] = p < d ? list[p] : kEmptyKey;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const unsigned long long m = a.word(t[r]); // kEmptyKey is no node id
    key[r] = (uint32_t)m;
    in |= (m & kChosen) ? 1u << r : 0u;
  }
  const bool all = e <= k;
  uint32_t V = 0, need = 0;
  if (!all) { // V = the k-th smallest key32: the largest V with fewer than k keys below it
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t X = V | (1u << bit);
      uint32_t c = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) c += (uint32_t)__popcll(__ballot(((in >> r) & 1u) && key[r] < X));
      if (c < k) V = X;
    }
    uint32_t less = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) less += (uint32_t)__popcll(__ballot(((in >> r) & 1u) && key[r] < V));
    need = k - less; // of the positions whose key32 IS V, the first `need`
  }
  uint32_t ties = 0, out = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool el = (in >> r) & 1u;
    const uint64_t eq = __ballot(el && !all && key[r] == V);
    const bool sel = el && (all || key[r] < V || (key[r] == V && ties + (uint32_t)__popcll(eq & below) < need));
    const uint64_t sm = __ballot(sel);
    if (sel) emit(out + (uint32_t)__popcll(sm & below), 64u * r + lane, t[r]);
    ties += (uint32_t)__popcll(eq);
    out += (uint32_t)__popcll(sm);
  }
}

__global__ __launch_bounds__(kBlock) void k_budget_select(BudgetArgs a, Count n_arg, BudgetCtl *ctl,
                                                          uint32_t *__restrict__ heavy_list) {
  const uint64_t n = n_arg.get();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  for (uint64_t i = wave; i < n; i += waves) {
    const uint32_t e = a.cnt[i];
    if (e == 0) continue; // no edge into the chosen set (a seed of degree 0 among them)
    const uint32_t rid = a.input[i];
    uint32_t d;
    const uint32_t *list = a.g.neighbours(rid, d);
    if (d > kLaborWaveMax) { // a workgroup's list
      if (lane_id() == 0) heavy_list[atomicAdd(&ctl->heavy, 1u)] = (uint32_t)i;
      continue;
    }
    const BudgetEmit emit = a.emit_of(i, rid, (uint32_t)(list - a.g.indices));
    if (d <= kLaborWave1) budget_wave_select<1>(a, list, d, a.fanout, e, emit);
    else if (d <= kLaborWave4) budget_wave_select<4>(a, list, d, a.fanout, e, emit);
    else budget_wave_select<16>(a, list, d, a.fanout, e, emit);
  }
}

// eligible entries of list[0, d) whose key32 is below X, counted by the workgroup's lanes; the caller sums
__device__ __forceinline__ uint32_t budget_count_below(const BudgetArgs &a, const uint32_t *__restrict__ list, uint32_t d,
                                                       uint32_t X) {
  constexpr uint32_t U = 4;
  uint32_t c = 0;
  for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
    uint32_t v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t p = base + u * kBlock + threadIdx.x;
      v[u] = p < d ? list[p] : kEmptyKey;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const unsigned long long m = a.word(v[u]);
      c += ((m & kChosen) && (uint32_t)m < X) ? 1u : 0u;
    }
  }
  return c;
}

// One list by the whole workgroup (every thread calls it with the same arguments; d > kLaborWaveMax, e >= 1 eligible
// entries).  Ends with a barrier: the next call may rewrite the LDS at once.
__device__ __forceinline__ void budget_hub_list(const BudgetArgs &a, const uint32_t *__restrict__ list, uint32_t d,
                                                uint32_t k, uint32_t e, const BudgetEmit &emit) {
  constexpr uint32_t U = 4;
  __shared__ unsigned long long s_key[kHubCand];
  __shared__ uint32_t s_sel[kLaborMaxFanout + 1];
  __shared__ uint32_t s_sum[2][kBlock / kWave];
  __shared__ uint32_t s_scan[kBlock / kWave];
  __shared__ uint32_t s_cnt, s_nsel;
  const uint32_t tid = threadIdx.x;
  uint32_t turn = 0;
  if (tid == 0) {
    s_cnt = 0;
    s_nsel = 0;
  }
  __syncthreads();
  if (e <= kHubCand) {
    // ---- the eligible (key32, position) pairs, in any order: the key carries the position
    for (uint64_t base = 0; base < d; base += (uint64_t)kBlock * U) {
      uint32_t v[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint64_t p = base + u * kBlock + tid;
        v[u] = p < d ? list[p] : kEmptyKey;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const unsigned long long m = a.word(v[u]);
        if (m & kChosen) {
          const uint32_t slot = atomicAdd(&s_cnt, 1u);
          if (slot < kHubCand) s_key[slot] = (m << 32) | (uint32_t)(base + u * kBlock + tid);
        }
      }
    }
    __syncthreads();
    const uint32_t m = s_cnt < kHubCand ? s_cnt : kHubCand; // == e
    uint32_t nsel = m;
    if (m > k) {
      // ---- the k-th smallest key: positions are below d, the bits between are zero in every key
      unsigned long long K = 0;
      const int pos_top = 31 - __clz((int)(d - 1u));
      for (int bit = 63; bit >= 0; --bit) {
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
      nsel = k;
    } else if (tid < m) {
      s_sel[tid] = (uint32_t)s_key[tid];
    }
    __syncthreads();
    if (tid < nsel) { // ranked by position
      const uint32_t p = s_sel[tid];
      uint32_t rank = 0;
      for (uint32_t x = 0; x < nsel; ++x) rank += s_sel[x] < p ? 1u : 0u;
      emit(rank, p, list[p]);
    }
  } else {
    // ---- the exact route (e > kHubCand > k): the k-th smallest key32 over the list itself, an emit in position order
    uint32_t V = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t X = V | (1u << bit);
      if (labor_block_sum(budget_count_below(a, list, d, X), s_sum, turn++) < k) V = X;
    }
    const uint32_t need = k - labor_block_sum(budget_count_below(a, list, d, V), s_sum, turn++);
    uint32_t ties = 0, out = 0;
    for (uint64_t base = 0; base < d && out < k; base += kBlock) {
      const uint64_t p = base + tid;
      const uint32_t t = p < d ? list[p] : kEmptyKey;
      const unsigned long long m = a.word(t);
      const bool el = (m & kChosen) != 0ull;
      const bool lt = el && (uint32_t)m < V, eq = el && (uint32_t)m == V;
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
  __syncthreads(); // s_key / s_sel / the counters are rewritten by the next list
}

__global__ __launch_bounds__(kBlock) void k_budget_hub(BudgetArgs a, const BudgetCtl *ctl,
                                                       const uint32_t *__restrict__ heavy_list) {
  const uint32_t nh = ctl->heavy;
  for (uint32_t q = blockIdx.x; q < nh; q += gridDim.x) {
    const uint32_t i = heavy_list[q];
    const uint32_t rid = a.input[i];
    uint32_t d;
    const uint32_t *__restrict__ list = a.g.neighbours(rid, d);
    budget_hub_list(a, list, d, a.fanout, a.cnt[i], a.emit_of(i, rid, (uint32_t)(list - a.g.indices)));
  }
}

inline size_t up2(size_t w) { return (w + 1) & ~(size_t)1; }
constexpr size_t kCtlWords = sizeof(BudgetCtl) / sizeof(uint32_t);
static_assert(sizeof(BudgetCtl) % 8 == 0, "the histograms behind it stay 8-byte aligned");

// candidate words behind a workspace of `bytes` whose first `fixed` bytes are the layer's own: ids, then keys
size_t cand_capacity(size_t bytes, size_t fixed, uint32_t num_node) {
  const size_t room = bytes > fixed + 16 ? (bytes - fixed - 16) / 8 : 0;
  return room < num_node ? room : num_node;
}

} // namespace

// words: 2 of slack for the 8-byte alignment, then ctl | hist | cnt (zeroed together) | pre | offset | heavy | cw | scan
size_t budget_ws_words(size_t n) {
  return 2 + kCtlWords + (size_t)kMaxPass * kRadix + 4 * up2(n) + 2 * n + tile_scan_words(n) + 16;
}

int sample_khop_budget_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t fanout = (uint32_t)l.fanout;
  const uint32_t N = l.graph->num_node;
  const uint32_t cap = (uint32_t)l.budget_cap;
  uint32_t *w = (uint32_t *)(((uintptr_t)l.workspace + 7) & ~(uintptr_t)7);
  BudgetCtl *ctl = (BudgetCtl *)w;
  uint32_t *hist = w + kCtlWords;
  uint32_t *cnt = hist + (size_t)kMaxPass * kRadix;
  uint32_t *pre = cnt + up2(n_max);
  uint32_t *offset = pre + up2(n_max);
  uint32_t *heavy_list = offset + up2(n_max);
  uint64_t *cw = (uint64_t *)(heavy_list + up2(n_max));
  uint32_t *scan_scr = (uint32_t *)(cw + n_max);
  uint32_t *cand = l.budget_cand, *cand_key = cand + cap;
  const ScanArea sa = l.scan ? *l.scan : ScanArea{scan_scr, false};
  const KeyPlan kp = key_plan(N);
  const uint64_t S = l.budget_nodes;
  GGMS_HIP(hipMemsetAsync(ctl, 0, (size_t)((char *)pre - (char *)ctl), l.s));
  int rc = tile_scan(ListDegree{l.g, l.input, nullptr},
                     BudgetPrefix{pre, l.budget_mode == GGMS_BUDGET_LADIES ? cw : nullptr, &ctl->over}, n_max, l.n, sa, nullptr,
                     nullptr, &ctl->E, l.s);
  if (rc != GGMS_OK) return rc;
  // persistent grids: the walked total and the candidate count are only known on the device
  hipLaunchKernelGGL(k_budget_accumulate, dim3(grid_cap()), dim3(kBlock), 0, l.s, l.g, l.input, l.n,
                     (const uint32_t *)pre, l.budget_mode == GGMS_BUDGET_LADIES ? (const uint64_t *)cw : nullptr, ctl,
                     l.budget_map, N, cand, cap);
  const int sel_grid = grid_for(cap, kSelTile);
  hipLaunchKernelGGL(k_budget_keys, dim3(sel_grid), dim3(kBlock), 0, l.s, ctl, hist, (const uint32_t *)cand, cand_key, cap,
                     (const unsigned long long *)l.budget_map, S, l.salt, kp, sa.status_word());
  for (uint32_t p = 1; p < kp.passes; ++p)
    hipLaunchKernelGGL(k_budget_hist, dim3(sel_grid), dim3(kBlock), 0, l.s, ctl, hist, (const uint32_t *)cand,
                       (const uint32_t *)cand_key, cap, S, kp, p);
  hipLaunchKernelGGL(k_budget_mark, dim3(grid_for(cap, kBlock)), dim3(kBlock), 0, l.s, ctl, (const uint32_t *)hist,
                     (const uint32_t *)cand, (const uint32_t *)cand_key, cap, l.budget_map, S, kp, l.budget_stat);
  hipLaunchKernelGGL(k_budget_count, dim3(grid_cap()), dim3(kBlock), 0, l.s, l.g, l.input, l.n, (const uint32_t *)pre,
                     (const BudgetCtl *)ctl, (const unsigned long long *)l.budget_map, N, cnt);
  GGMS_LAUNCH_CHECK();
  rc = tile_scan(BudgetCount{cnt, fanout}, LaborOffset{offset}, n_max, l.n, sa, nullptr, nullptr, l.num_out, l.s);
  if (rc != GGMS_OK) return rc;
  const BudgetArgs a{l.g,       (const unsigned long long *)l.budget_map, l.input, offset, cnt, l.out_src, l.out_dst,
                     l.out_pos, fanout, N, l.src};
  hipLaunchKernelGGL(k_budget_select, dim3(grid_for(n_max, kBlock / kWave)), dim3(kBlock), 0, l.s, a, l.n, ctl, heavy_list);
  // a workgroup per listed seed; how many there are is only known on the device
  hipLaunchKernelGGL(k_budget_hub, dim3(grid_for(n_max, 1)), dim3(kBlock), 0, l.s, a, (const BudgetCtl *)ctl,
                     (const uint32_t *)heavy_list);
  hipLaunchKernelGGL(k_budget_restore, dim3(grid_for(cap, kBlock)), dim3(kBlock), 0, l.s, (const BudgetCtl *)ctl,
                     (const uint32_t *)cand, cap, l.budget_map);
  GGMS_LAUNCH_CHECK();
  return GGMS_OK;
}

// the refusals of include/ggms.h that need no device call; `who` names the entry point
int budget_check(const ggms_graph_t *graph, size_t n_max, const size_t *budgets, const size_t *fanouts, uint32_t num,
                 int mode, const void *map, const char *who) {
  if (graph->num_part != 0) {
    set_error("%s: num_part %u: the weights are summed over the lists of ONE CSR and positions are its own, the call takes "
              "unsharded graphs only", who, graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (mode != GGMS_BUDGET_UNIFORM && mode != GGMS_BUDGET_LADIES) {
    set_error("%s: mode %d (GGMS_BUDGET_UNIFORM or GGMS_BUDGET_LADIES)", who, mode);
    return GGMS_ERR_INVALID;
  }
  if (n_max >= ((size_t)1 << 22)) {
    set_error("%s: %zu seeds in a layer: at most 2^22 - 1, so that a candidate's 64-bit weight cannot overflow", who, n_max);
    return GGMS_ERR_INVALID;
  }
  for (uint32_t i = 0; i < num; ++i) {
    if (budgets[i] < 1) {
      set_error("%s: a node budget of 0 (layer %u): every layer draws at least one node", who, i);
      return GGMS_ERR_INVALID;
    }
    if (fanouts[i] < 1 || fanouts[i] > kLaborMaxFanout) {
      set_error("%s: fanout %zu (layer %u): a seed keeps 1 .. %u of its eligible edges", who, fanouts[i], i, kLaborMaxFanout);
      return GGMS_ERR_INVALID;
    }
  }
  if (n_max != 0 && !map) {
    set_error("%s: map is null (8 bytes per node, ggms_budget_map_init)", who);
    return GGMS_ERR_INVALID;
  }
  return GGMS_OK;
}

size_t budget_cand_bytes(uint64_t num_edge) { return 8 * (size_t)num_edge + 16; }

bool budget_set_cand(SampleLayer &l, void *workspace, size_t workspace_bytes, size_t fixed_bytes, const char *who) {
  const size_t cap = cand_capacity(workspace_bytes, fixed_bytes, l.graph->num_node);
  if (cap == 0 && l.graph->num_node != 0) {
    set_error("%s: workspace_bytes %zu leaves no room for the candidate list behind the first %zu bytes", who, workspace_bytes,
              fixed_bytes);
    return false;
  }
  l.budget_cand = (uint32_t *)(((uintptr_t)workspace + fixed_bytes + 15) & ~(uintptr_t)15);
  l.budget_cap = cap;
  return true;
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_budget_map_init(uint64_t *map, size_t num_node, ggms_stream_t stream) {
  if (num_node == 0) return GGMS_OK;
  if (!map) {
    set_error("ggms_budget_map_init: map is null");
    return GGMS_ERR_INVALID;
  }
  GGMS_HIP(hipMemsetAsync(map, 0, num_node * sizeof(uint64_t), to_stream(stream)));
  return GGMS_OK;
}

size_t ggms_sample_khop_budget_workspace_bytes(size_t num_input, size_t fanout, uint64_t num_edge) {
  if (num_edge >= 0xffffffffull) {
    set_error("ggms_sample_khop_budget_workspace_bytes: %llu edges: positions are 32-bit (at most 2^32 - 2)",
              (unsigned long long)num_edge);
    return 0;
  }
  return layer_ws_words(GGMS_KHOP_BUDGET, num_input, fanout, 0, 0) * sizeof(uint32_t) + budget_cand_bytes(num_edge);
}

int ggms_sample_khop_budget(const ggms_graph_t *graph, const ggms_id_t *input, size_t num_input, size_t budget,
                            size_t fanout, int mode, uint32_t layer_salt, uint64_t *map, ggms_id_t *out_src,
                            ggms_id_t *out_dst, ggms_id_t *out_pos, uint64_t *num_out_dev, uint64_t *stat_dev,
                            void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  static const char *const who = "ggms_sample_khop_budget";
  GGMS_CHECK_ARG(graph && num_out_dev);
  int rc = budget_check(graph, num_input, &budget, &fanout, 1, mode, map, who);
  if (rc != GGMS_OK) return rc;
  SampleLayer l{graph, input, num_input, fanout, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.salt = layer_salt;
  l.out_pos = out_pos;
  l.budget_map = (unsigned long long *)map;
  l.budget_nodes = budget;
  l.budget_mode = mode;
  l.budget_stat = stat_dev;
  if (num_input == 0) {
    if (stat_dev) GGMS_HIP(hipMemsetAsync(stat_dev, 0, 2 * sizeof(uint64_t), l.s));
  } else {
    GGMS_CHECK_ARG(workspace && out_pos);
    if (!budget_set_cand(l, workspace, workspace_bytes, layer_ws_words(GGMS_KHOP_BUDGET, num_input, fanout, 0, 0) * 4, who))
      return GGMS_ERR_INVALID;
  }
  return sample_leaf(GGMS_KHOP_BUDGET, l, 0, workspace_bytes);
}

} // extern "C"
