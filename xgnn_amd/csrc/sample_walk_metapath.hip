// sample_walk_metapath.hip -- random_walk_metapath: PinSAGE's walks along a relation path on a type-sorted CSR
// (include/ggms.h; tests/walk_metapath_ref.py restates the definition in numpy).
//
// There is no reference counterpart (DGL: RandomWalkNeighborSampler(metapath=...) / PinSAGESampler).  A walk follows
// metapath[0 .. M) over and over; only the node at the end of a full traversal is a visit.  Step j leaves node u through
// the edges of relation r = metapath[j]: inside u's list the type bytes are non-decreasing, so those edges are one
// contiguous SEGMENT, and the step is "find the segment, pick one of its e entries with one hash".  The walk is stateless
// (khop_labor's fmix32 of the seed's id, the walk and the step): no RNG pool, nothing to order between batches.
//
// ONE kernel writes the visit scratch (tmp_src / tmp_dst, visit-major, stride n_max) exactly as k_random_walk lays it
// out; ranking, scan, compaction and the table insert are sample_random_walk.hip's k_walk_topk_emit, unchanged
// (walk_topk_impl).  DESIGN.md 8r:
//   items      an item is a (walk, seed) pair, walk-major: a wave holds 64 consecutive seeds of one walk, so every visit
//              is one coalesced 256-byte store per array, and the ids / list heads of a wave's first step are those of
//              consecutive frontier entries.  W walks of a seed run in W different waves, side by side.
//   ordinary   a lane finds both ends of r's segment itself: two one-load exits (type[0] > r or type[d-1] < r: empty;
//              type[0] == r: the segment starts the list; type[d-1] == r: it ends it -- a one-relation list is settled by
//              these two loads), else two lower-bound searches over the bytes, independent chains advanced in the same
//              round so that their loads travel together: log2(d) round trips, not 2 log2(d).
//   hubs       a list of more than kWalkHubMin entries is searched by the whole wave, 64 probes per round
//              (wave_type_bound, type_bound.h): the wave ballots its hub lanes and serves them one after the other.  A
//              million-entry hub costs 2 x 4 rounds of one probe per lane instead of 40 dependent byte loads in one lane
//              while 63 wait.
//   bounds     every loop is bounded: M x T steps, 32 search rounds, 64 hub turns of log64 rounds.  No atomics, no LDS,
//              no scratch; grid-stride under grid_for.  A list whose bytes are not sorted gets SOME [L, U) inside
//              [0, d): every probe and the pick lie inside the list.
#include "ggms_internal.h"
#include "labor_hash.h"
#include "type_bound.h"

#include <cmath>

namespace ggms {

// lists longer than this are searched by the wave together.  At 2048: 11 rounds of two byte loads in one lane, the 64
// lanes' chains overlapping, against 2 x 2 rounds of the whole wave per hub lane, one hub after the other.  The only
// value tried (profiles/walk_metapath.txt)
constexpr uint32_t kWalkHubMin = 2048;

// metapath[j], j < GGMS_MAX_METAPATH, one byte each
struct Metapath {
  uint32_t w[GGMS_MAX_METAPATH / 4];
  __device__ __forceinline__ uint32_t get(uint32_t j) const { return ((j < 4u ? w[0] : w[1]) >> ((j & 3u) * 8u)) & 0xffu; }
};

__global__ __launch_bounds__(kBlock) void k_walk_metapath(const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ indices,
                                                          const uint8_t *__restrict__ edge_type,
                                                          const uint32_t *__restrict__ input, Count n_arg,
                                                          uint64_t stride, Metapath mp, uint32_t M, uint32_t T, uint32_t W,
                                                          uint64_t thr, uint32_t salt, uint32_t *__restrict__ tmp_src,
                                                          uint32_t *__restrict__ tmp_dst) {
  const uint64_t n = n_arg.get();
  const uint32_t lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t chunks = (n + kWave - 1) / kWave; // 64 seeds of one walk
  const uint64_t items = chunks * W;
  // the loop and everything in it that ballots is uniform over the wave: a lane without a seed or with a finished walk
  // stays in step and takes part in the hub searches of the others
  for (uint64_t c = wave; c < items; c += waves) {
    const uint32_t w = (uint32_t)(c / chunks);
    const uint64_t i = (c - (uint64_t)w * chunks) * kWave + lane;
    const bool in = i < n;
    const uint32_t seed = in ? input[i] : kEmptyKey;
    const uint32_t wk = fmix32(fmix32(seed ^ salt) + 0x9E3779B9u * (w + 1u));
    const auto draw = [wk](uint32_t x) -> uint32_t { return fmix32(wk + 0x85EBCA6Bu * (x + 1u)); };
    bool alive = seed != kEmptyKey;
    uint32_t u = seed;
    for (uint32_t t = 0; t < T; ++t) {
      for (uint32_t j = 0; j < M; ++j) {
        if (__ballot(alive) == 0ull) break; // nothing left to walk in this wave
        const uint32_t r = mp.get(j);
        uint32_t b0 = 0, d = 0;
        if (alive) {
          uint32_t end;
          GraphView::bounds(indptr, u, b0, end);
          d = end - b0;
        }
        const bool hub = d > kWalkHubMin;
        uint32_t lb = 0, ub = 0; // r's segment of the list: [lb, ub)
        if (d != 0u && !hub) {
          const uint8_t *__restrict__ type = edge_type + b0;
          const uint32_t t0 = type[0], tl = type[d - 1u];
          if (t0 <= r && tl >= r) {
            // L = the first p with type[p] >= r, in [lo1, hi1]; U = the first p with type[p] > r, in [lo2, hi2]
            uint32_t lo1 = t0 == r ? 0u : 1u, hi1 = t0 == r ? 0u : d - 1u;
            uint32_t lo2 = tl == r ? d : 1u, hi2 = tl == r ? d : d - 1u;
            for (uint32_t round = 0; round < 32u; ++round) {
              const bool a1 = lo1 < hi1, a2 = lo2 < hi2;
              if (!a1 && !a2) break;
              const uint32_t m1 = lo1 + ((hi1 - lo1) >> 1), m2 = lo2 + ((hi2 - lo2) >> 1);
              const uint32_t y1 = a1 ? type[m1] : 0u, y2 = a2 ? type[m2] : 0u; // both in flight together
              if (a1) { if (y1 < r) lo1 = m1 + 1u; else hi1 = m1; }
              if (a2) { if (y2 <= r) lo2 = m2 + 1u; else hi2 = m2; }
            }
            lb = lo1;
            ub = lo2;
          }
        }
        uint64_t hubs = __ballot(hub);
        for (uint32_t turn = 0; turn < (uint32_t)kWave && hubs != 0ull; ++turn) {
          const int leader = __ffsll((long long)hubs) - 1;
          hubs &= hubs - 1ull;
          const uint64_t hb = (uint32_t)__shfl((int)b0, leader), hd = (uint32_t)__shfl((int)d, leader);
          const uint64_t sb = wave_type_bound<false>(edge_type, hb, hd, r, lane);
          const uint64_t se = wave_type_bound<true>(edge_type, sb, hb + hd - sb, r, lane);
          if ((int)lane == leader) {
            lb = (uint32_t)(sb - hb);
            ub = (uint32_t)(se - hb);
          }
        }
        const uint32_t e = ub > lb ? ub - lb : 0u;
        if (alive) {
          if (e == 0u) alive = false; // no edge of relation r (degree 0 included): the walk ends
          else u = indices[(uint64_t)b0 + lb + __umulhi(draw(2u * (t * M + j)), e)];
        }
      }
      // visit t * W + w of the seed: k_random_walk's [step][walk] order, a traversal in the place of a step
      if (in) {
        const uint64_t pos = ((uint64_t)t * W + w) * stride + i;
        if (alive) {
          tmp_src[pos] = seed;
          tmp_dst[pos] = u;
          if ((uint64_t)draw(2u * t + 1u) < thr) alive = false; // restart
        } else {
          tmp_src[pos] = kEmptyKey;
        }
      }
    }
  }
}

// what include/ggms.h says ggms_sample_walk_metapath refuses about the walk itself; host arithmetic only
int walk_metapath_check(uint32_t num_type, const uint32_t *metapath, uint32_t metapath_len, size_t num_traversal,
                        double restart_prob, size_t num_walk, size_t K, const char *who) {
  if (num_type < 1 || num_type > GGMS_MAX_EDGE_TYPES) {
    set_error("%s: num_type %u (1 .. %u relations)", who, num_type, (unsigned)GGMS_MAX_EDGE_TYPES);
    return GGMS_ERR_INVALID;
  }
  if (!metapath || metapath_len < 1 || metapath_len > GGMS_MAX_METAPATH) {
    set_error("%s: metapath_len %u (a host array of 1 .. %u relation ids)", who, metapath_len, (unsigned)GGMS_MAX_METAPATH);
    return GGMS_ERR_INVALID;
  }
  for (uint32_t j = 0; j < metapath_len; ++j)
    if (metapath[j] >= num_type) {
      set_error("%s: metapath[%u] = %u is no relation (num_type %u)", who, j, metapath[j], num_type);
      return GGMS_ERR_INVALID;
    }
  if (num_traversal == 0 || num_walk == 0 || K == 0) {
    set_error("%s: num_traversal %zu, num_walk %zu, K %zu: each at least 1", who, num_traversal, num_walk, K);
    return GGMS_ERR_INVALID;
  }
  if (num_traversal * num_walk >= (1ull << 31) || num_traversal * metapath_len >= (1ull << 30)) {
    set_error("%s: num_traversal %zu x num_walk %zu visits per seed (below 2^31; steps below 2^30)", who, num_traversal,
              num_walk);
    return GGMS_ERR_INVALID;
  }
  if (!std::isfinite(restart_prob) || restart_prob < 0.0 || restart_prob > 1.0) {
    set_error("%s: restart_prob %g (a probability, 0 .. 1)", who, restart_prob);
    return GGMS_ERR_INVALID;
  }
  return GGMS_OK;
}

int sample_walk_metapath_impl(const SampleLayer &l) {
  const size_t n_max = l.n_max;
  const uint32_t T = (uint32_t)l.walk_length, W = (uint32_t)l.num_walk, M = l.metapath_len;
  const uint32_t per = T * W;
  uint32_t *w = l.workspace;
  uint32_t *tmp_src = w; w += n_max * per;
  uint32_t *tmp_dst = w; w += n_max * per;
  Metapath mp{};
  for (uint32_t j = 0; j < M; ++j) mp.w[j >> 2] |= (l.metapath[j] & 0xffu) << ((j & 3u) * 8u);
  // thr = min(2^32, floor(p 2^32)): a walk restarts when its 32-bit draw lies below it
  const double scaled = std::floor(l.restart_prob * 4294967296.0);
  const uint64_t thr = scaled >= 4294967296.0 ? (1ull << 32) : (uint64_t)scaled;
  const size_t items = (n_max + kWave - 1) / kWave * W;
  hipLaunchKernelGGL(k_walk_metapath, dim3(grid_for(items, kBlock / kWave)), dim3(kBlock), 0, l.s, l.g.indptr, l.g.indices,
                     l.edge_type, l.input, l.n, (uint64_t)n_max, mp, M, T, W, thr, l.salt, tmp_src, tmp_dst);
  GGMS_LAUNCH_CHECK();
  return walk_topk_impl(l, tmp_src, tmp_dst, per, w);
}

} // namespace ggms

using namespace ggms;

extern "C" {

size_t ggms_sample_walk_metapath_workspace_bytes(size_t num_input, size_t num_traversal, size_t num_walk, size_t K) {
  return random_walk_ws_words(num_input, num_traversal, num_walk, K) * sizeof(uint32_t);
}

int ggms_sample_walk_metapath(const ggms_graph_t *graph, const uint8_t *edge_type, uint32_t num_type,
                              const uint32_t *metapath, uint32_t metapath_len, const ggms_id_t *input, size_t num_input,
                              size_t num_traversal, double restart_prob, size_t num_walk, size_t K, uint32_t layer_salt,
                              ggms_id_t *out_src, ggms_id_t *out_dst, ggms_id_t *out_data, uint64_t *num_out_dev,
                              void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  static const char *const who = "ggms_sample_walk_metapath";
  GGMS_CHECK_ARG(graph && num_out_dev);
  if (graph->num_part != 0) {
    set_error("%s: num_part %u: edge types are stored by position in ONE CSR, the call takes unsharded graphs only", who,
              graph->num_part);
    return GGMS_ERR_INVALID;
  }
  if (!edge_type) {
    set_error("%s: edge_type is NULL (one uint8 per position of graph->indices)", who);
    return GGMS_ERR_INVALID;
  }
  const int rc = walk_metapath_check(num_type, metapath, metapath_len, num_traversal, restart_prob, num_walk, K, who);
  if (rc != GGMS_OK) return rc;
  if (num_input != 0 &&
      workspace_bytes < ggms_sample_walk_metapath_workspace_bytes(num_input, num_traversal, num_walk, K)) {
    set_error("%s: workspace_bytes %zu, ggms_sample_walk_metapath_workspace_bytes gives %zu", who, workspace_bytes,
              ggms_sample_walk_metapath_workspace_bytes(num_input, num_traversal, num_walk, K));
    return GGMS_ERR_INVALID;
  }
  SampleLayer l{graph, input, num_input, K, out_src, out_dst, num_out_dev, nullptr, (uint32_t *)workspace,
                to_stream(stream)};
  l.out_data = out_data;
  l.walk_length = num_traversal;
  l.num_walk = num_walk;
  l.restart_prob = restart_prob;
  l.salt = layer_salt;
  l.edge_type = edge_type;
  l.num_type = num_type;
  l.metapath = metapath;
  l.metapath_len = metapath_len;
  return sample_leaf(GGMS_RANDOM_WALK_METAPATH, l, 0, workspace_bytes);
}

} // extern "C"
