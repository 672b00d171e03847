// sample_batch.hip -- one mini-batch of k-layer sampling, enqueued in one go.
//
// Reference: DoGPUSample (dist/dist_loops.cc:62-368; single-process twin
// cuda/cuda_loops.cc:54-292): per layer {sample -> D2H nnz -> FillWithDuplicates ->
// D2H num_unique -> GPUMapEdges}, i.e. two host round trips per layer plus one
// StreamSync after every kernel.
//
// Here the whole loop is a straight sequence of launches on one stream.  Every
// size that the next launch depends on (frontier size, edge count) stays in
// device memory and is read by the kernels themselves (ggms::Count); grids are
// sized from the closed-form upper bounds of PredictNumNodes (common.cc:488-497)
// and grid-stride, so a launch never needs the exact value.  The caller syncs
// once, after the feature extract that follows.
//
// Other savings against the reference, all result-preserving:
//   * the frontier of layer i-1 is the hash table's n2o prefix: no `unique`
//     buffer is allocated or copied (dist_loops.cc:271-280,350-353);
//   * `col` (local id of the edge's seed) is written by the sampler: a seed's
//     local id is its position in the frontier (n2o), so the E hash lookups of
//     GPUMapEdges' src half (cuda_mapping.cu:57-60) reduce to none (n lookups
//     for the first layer, whose input is the raw seed list);
//   * `row` (local id of the sampled neighbour) is produced by the table fill itself:
//     the instance that owns a key gets its id in the owner scan, an instance that
//     loses to an EARLIER layer resolves its id inside the sampler, and the few that
//     lose inside their own layer are looked up for all layers at once at the end
//     (k_map_rest_all) -- the dst half of GPUMapEdges without a pass of random reads
//     over all E edges, and without rewriting the table (batch mode, ggms_device.h);
//   * with the direct table layout khop3's fused launch also enters the neighbours
//     into the table (one returning atomicMin each), so FillWithDuplicates is only
//     the owner scan: 3 + 2 L + 1 launches per batch in all;
//   * the batch prologue (scan-area clear, item-count reset, |seeds| record) rides on
//     the first kernel of the batch instead of three tiny launches.
// Several batches may be in flight on different streams (own table + workspace each):
// ggms_sample_extra_t.rng_wait / rng_done chain only the sampler kernels, which share
// the RNG pool, in batch order.
#include <algorithm>
#include <functional>
#include <vector>

#include "ggms_internal.h"
#include "labor_hash.h"
#include "tile_scan.h"

namespace ggms {

__global__ void k_record(uint64_t *slot, Count c) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *slot = c.get();
}

struct BatchCaps {
  size_t max_input[16];
  size_t max_edges[16];
  size_t max_in_all, max_e_all;
};

static BatchCaps caps_of(size_t num_seeds, const size_t *fanouts, uint32_t L) {
  BatchCaps c{};
  size_t n = num_seeds;
  for (int i = (int)L - 1; i >= 0; --i) {
    c.max_input[i] = n;
    c.max_edges[i] = n * fanouts[i];
    n += c.max_edges[i]; // unique nodes so far <= previous unique + new edges
    if (c.max_input[i] > c.max_in_all) c.max_in_all = c.max_input[i];
    if (c.max_edges[i] > c.max_e_all) c.max_e_all = c.max_edges[i];
  }
  return c;
}

// ---- the per-sampler rules: one copy for the leaf entry points and ggms_sample_batch --------------------------

size_t layer_ws_words(int type, size_t n, size_t fanout, size_t walk_length, size_t num_walk, size_t num_type) {
  switch (type) {
  case GGMS_KHOP_TYPED: return typed_ws_words(n, num_type);
  case GGMS_KHOP0: return khop0_ws_words(n, fanout);
  case GGMS_KHOP1:
  case GGMS_WEIGHTED_KHOP:
  case GGMS_WEIGHTED_KHOP_PREFIX: return weighted_ws_words(n, fanout);
  case GGMS_RANDOM_WALK: return random_walk_ws_words(n, walk_length, num_walk, fanout);
  case GGMS_KHOP_LABOR: return labor_ws_words(n);
  case GGMS_KHOP_TEMPORAL: return temporal_ws_words(n);
  default: return sample_ws_words(n); // khop3, khop2, weighted_khop_hash_dedup
  }
}

// fanout limits, sharded graphs, walk parameters: checked first, even by a leaf call with nothing to sample
static int layer_shape_check(int type, const SampleLayer &l) {
  GGMS_CHECK_ARG(l.fanout > 0); // a layer that samples nothing is a config error
  if (type == GGMS_KHOP3) GGMS_CHECK_ARG(l.fanout < 128);                            // khop3.cu:85
  if (type == GGMS_WEIGHTED_KHOP_HASH_DEDUP) GGMS_CHECK_ARG(l.fanout < kDedupSlots); // hash_dedup.cu:42
  if (type == GGMS_KHOP_LABOR) GGMS_CHECK_ARG(l.fanout < 128); // the hub route ranks its selection in LDS
  if (type == GGMS_KHOP_TEMPORAL) GGMS_CHECK_ARG(l.fanout < 128); // khop_labor's selection on a prefix
  if (type == GGMS_KHOP_TYPED) { // khop_labor's selection per segment: every k_r < 128; `fanout` is the row's sum
    size_t sum = 0;
    const int rc = typed_fanout_sum(l.type_fanout, l.num_type, &sum);
    if (rc != GGMS_OK) return rc;
    GGMS_CHECK_ARG(sum == l.fanout);
  }
  if (type == GGMS_RANDOM_WALK) GGMS_CHECK_ARG(l.walk_length > 0 && l.num_walk > 0);
  // "this algorithm not support DistGraph engine", dist_loops.cc:167-228
  if (type != GGMS_KHOP3 && type != GGMS_KHOP0 && type != GGMS_RANDOM_WALK && type != GGMS_KHOP_LABOR)
    GGMS_CHECK_ARG(l.graph->num_part == 0);
  return GGMS_OK;
}

// + the tables the sampler reads and its RNG-pool bound
static int layer_check(int type, const SampleLayer &l, size_t num_states) {
  const int rc = layer_shape_check(type, l);
  if (rc != GGMS_OK) return rc;
  const uint64_t n = l.n_max;
  if (type == GGMS_KHOP1 || type == GGMS_KHOP2 || type == GGMS_KHOP_TEMPORAL || type == GGMS_KHOP_TYPED)
    GGMS_CHECK_ARG(l.graph->indptr && l.graph->indices);
  if (type == GGMS_KHOP_TYPED) GGMS_CHECK_ARG(l.edge_type && l.out_pos && l.out_type);
  if (type == GGMS_KHOP_TEMPORAL) GGMS_CHECK_ARG(l.edge_time && l.out_pos && (l.input_cut || l.cut_table));
  if (type == GGMS_WEIGHTED_KHOP || type == GGMS_WEIGHTED_KHOP_HASH_DEDUP) GGMS_CHECK_ARG(l.prob && l.alias);
  if (type == GGMS_WEIGHTED_KHOP_PREFIX) GGMS_CHECK_ARG(l.prob);
  // the RNG pool: assert(i < num_random_states) in every sampler of the reference but khop0
  switch (type) {
  case GGMS_KHOP0:
  case GGMS_KHOP_LABOR:
  case GGMS_KHOP_TEMPORAL:
  case GGMS_KHOP_TYPED: return GGMS_OK; // stateless
  case GGMS_KHOP3: GGMS_CHECK_ARG(l.states && (n + 127) / 128 * 8 <= num_states); return GGMS_OK; // khop3.cu:89
  case GGMS_KHOP2:                                                                                   // khop2.cu:57
  case GGMS_WEIGHTED_KHOP_HASH_DEDUP: // hash_dedup.cu:70
    GGMS_CHECK_ARG(l.states && (n + 1023) / 1024 * 256 <= num_states);
    return GGMS_OK;
  case GGMS_RANDOM_WALK:
    GGMS_CHECK_ARG(l.states && ggms_random_walk_num_states(n, l.num_walk) <= num_states);
    return GGMS_OK;
  default: { // khop1.cu:51, weighted_khop.cu:52, prefix.cu:50: one stream per draw thread
    const uint64_t tasks = n * l.fanout;
    const uint64_t threads = tasks < kWeightedMaxThreads ? tasks : kWeightedMaxThreads;
    const uint64_t span = (threads + 255) / 256 * 256;
    GGMS_CHECK_ARG(l.states && (span < tasks ? span : tasks) <= num_states);
    return GGMS_OK;
  }
  }
}

static int sample_layer(int type, const SampleLayer &l) {
  switch (type) {
  case GGMS_KHOP3: return sample_khop3_impl(l);
  case GGMS_KHOP0: return sample_khop0_impl(l);
  case GGMS_KHOP2: return sample_khop2_impl(l);
  case GGMS_WEIGHTED_KHOP_HASH_DEDUP: return sample_weighted_hash_dedup_impl(l);
  case GGMS_RANDOM_WALK: return sample_random_walk_impl(l);
  case GGMS_KHOP_LABOR: return sample_khop_labor_impl(l);
  case GGMS_KHOP_TEMPORAL: return sample_khop_temporal_impl(l);
  case GGMS_KHOP_TYPED: return sample_khop_typed_impl(l);
  default: return sample_weighted_impl(l, type); // khop1, weighted_khop, weighted_khop_prefix
  }
}

// Whether the sampler enters its own output into the direct table (DedupInsert): khop3 and random walk on the way
// out, khop0 where it produces it, the weighted family in the compaction's emit, hash_dedup by a seed's 16 lanes once
// the seed is done.  khop2 does not: even with the four seeds of a lane in lock-step and their atomics issued together,
// the returning atomics sit in the draw loop's dependency chain (measured on products: 0.45 -> 0.62 ms per step; the
// separate insert launch of ht_fill_impl follows).  khop_labor does not either: its selection writes each edge from
// the lane that held the key, after a search that is all ballots -- a returning atomic per edge there would serialise
// behind the search of the seed's whole wave, and the sampler stays a pure function of its inputs.
// khop_temporal and khop_typed are khop_labor's selection: the same holds.
static bool layer_enters_output(int type) {
  return type != GGMS_KHOP2 && type != GGMS_KHOP_LABOR && type != GGMS_KHOP_TEMPORAL && type != GGMS_KHOP_TYPED;
}

// a leaf entry point: shape checks; nothing to sample -> a zero count (null pointers allowed); pointers, workspace and
// RNG pool; the sampler
int sample_leaf(int type, SampleLayer l, size_t num_states, size_t workspace_bytes) {
  GGMS_CHECK_ARG(l.graph && l.num_out);
  int rc = layer_shape_check(type, l);
  if (rc != GGMS_OK) return rc;
  if (l.n_max == 0) {
    GGMS_HIP(hipMemsetAsync(l.num_out, 0, sizeof(uint64_t), l.s));
    return GGMS_OK;
  }
  GGMS_CHECK_ARG(l.input && l.out_src && l.out_dst && l.workspace && (type != GGMS_RANDOM_WALK || l.out_data));
  GGMS_CHECK_ARG(workspace_bytes >=
                 layer_ws_words(type, l.n_max, l.fanout, l.walk_length, l.num_walk, l.num_type) * sizeof(uint32_t));
  // 32-bit output positions; a random walk's are bounded by walk_length * num_walk < 2^31 instead
  GGMS_CHECK_ARG(type == GGMS_RANDOM_WALK || (uint64_t)l.n_max * l.fanout < (1ull << 32));
  rc = layer_check(type, l, num_states);
  if (rc != GGMS_OK) return rc;
  if (!view_of(l.graph, l.g)) return GGMS_ERR_INVALID; // after layer_check's refusal of a sharded graph
  l.n = count_of(l.n_max);
  return sample_layer(type, l);
}

} // namespace ggms

using namespace ggms;

extern "C" {

int ggms_event_create(ggms_event_t *event) {
  GGMS_CHECK_ARG(event);
  hipEvent_t e;
  GGMS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *event = (ggms_event_t)e;
  return GGMS_OK;
}

int ggms_event_destroy(ggms_event_t event) {
  if (event) GGMS_HIP(hipEventDestroy((hipEvent_t)event));
  return GGMS_OK;
}

int ggms_sample_batch_capacity(size_t num_seeds, const size_t *fanouts, uint32_t num_layer, size_t *max_input,
                               size_t *max_edges, size_t *max_unique) {
  GGMS_CHECK_ARG(fanouts && num_layer >= 1 && num_layer <= 16);
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  for (uint32_t i = 0; i < num_layer; ++i) {
    if (max_input) max_input[i] = c.max_input[i];
    if (max_edges) max_edges[i] = c.max_edges[i];
  }
  if (max_unique) *max_unique = c.max_input[0] + c.max_edges[0];
  return GGMS_OK;
}

static size_t sampler_ws_words(int sample_type, const BatchCaps &c, const size_t *fanouts, uint32_t L,
                               const ggms_sample_extra_t *extra, size_t num_type) {
  size_t w = sample_ws_words(c.max_in_all);
  if (sample_type == GGMS_RANDOM_WALK && !extra) return w; // no walk: ggms_sample_batch refuses the call
  for (uint32_t i = 0; i < L; ++i)
    w = std::max(w, layer_ws_words(sample_type, c.max_input[i], fanouts[i], extra ? extra->random_walk_length : 0,
                                   extra ? extra->num_random_walk : 0, num_type));
  return w;
}

// ---- workspace layout of one batch (uint32 words; every piece starts 16-byte aligned) --------------------------
struct BatchLayout {
  size_t seed_local, samp_ws, tmp_dst[16], cand, lost, scan, chunk, total;
  size_t pf_keys, pf_local, pf_pre, pf_scan, pf_total; // ggms_sample_batch_prefetch only
  size_t dedup_items; // entries of cand / lost
  size_t scan_tiles;  // descriptors the scans of the batch may use (cleared by the batch prologue)
};
static inline size_t up4(size_t w) { return (w + 3) & ~(size_t)3; }

// pf_edges: the prefetching batch's expansion capacity (its keys are one more fill of the batch); 0 = none
// num_type: khop_typed's R (its boundary words); 0 = sized for GGMS_MAX_EDGE_TYPES.  seed_local is the first piece
// whatever it is
static BatchLayout layout_of(int sample_type, size_t num_seeds, const size_t *fanouts, uint32_t L, const BatchCaps &c,
                             const ggms_sample_extra_t *extra, size_t pf_edges = 0, size_t num_type = 0) {
  BatchLayout l{};
  size_t w = 0;
  l.seed_local = w;  w += up4(num_seeds + 16);
  l.samp_ws = w;     w += up4(sampler_ws_words(sample_type, c, fanouts, L, extra, num_type));
  for (uint32_t i = 0; i < L; ++i) { // global neighbour ids of every layer: kept for the end-of-batch id look-ups
    l.tmp_dst[i] = w;
    w += up4(c.max_edges[i] + 16);
  }
  l.dedup_items = std::max({c.max_e_all, num_seeds, pf_edges});
  l.cand = w;        w += up4(l.dedup_items + 16);          // hashed layout: bucket positions
  l.lost = w;        w += up4(2 * (l.dedup_items + 16));    // 64-bit tags
  // ONE scan area for the batch: sampler offsets (tiles of 128 seeds), owner scans (tiles of 2048 items), the
  // generic tile scans of the other samplers (<= kSinglePassTiles descriptors, else three launches)
  l.scan_tiles = std::max<size_t>({c.max_in_all / 128 + 2, owner_scan_tiles(l.dedup_items) + 2, kSinglePassTiles + 2});
  if (sample_type == GGMS_RANDOM_WALK) l.scan_tiles = std::max(l.scan_tiles, walk_scan_tiles(c.max_in_all));
  if (sample_type == GGMS_KHOP0) l.scan_tiles = std::max<size_t>(l.scan_tiles, 2 * (kSinglePassTiles + 2)); // two sums per pass
  l.scan = w;
  w += up4(std::max(tile_scan_words(std::max(c.max_e_all, c.max_in_all)), 8 + 2 * l.scan_tiles + 4) + 16);
  // the chunked owner scan's 32-bit descriptors + one ticket set per ticketed sampler launch: a piece of their own,
  // cleared by the batch prologue too
  l.chunk = w;
  w += up4(chunk_desc_words() + (size_t)kTicketSets * kTicketWords);
  if (pf_edges) { // the expansion: its keys, their local ids, the degree scan over the set after L - 1 layers
    l.pf_keys = w;   w += up4(pf_edges + 16);
    l.pf_local = w;  w += up4(pf_edges + 16);
    l.pf_pre = w;    w += up4(c.max_input[0] + 16);
    l.pf_scan = w;   w += up4(prefetch_scan_words(c.max_input[0]) + 16);
    l.pf_total = w;  w += 4;
  }
  l.total = w;
  return l;
}

size_t ggms_sample_batch_workspace_bytes(int sample_type, size_t num_seeds, const size_t *fanouts, uint32_t num_layer,
                                         const ggms_sample_extra_t *extra) {
  if (!fanouts || num_layer < 1 || num_layer > 16) return 0;
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  return layout_of(sample_type, num_seeds, fanouts, num_layer, c, extra).total * sizeof(uint32_t) + 16;
}

// ggms_sample_batch_prefetch's part of a batch (NULL: a plain ggms_sample_batch)
struct Prefetch {
  size_t max_edges;
  hipEvent_t start, final;
};

// ggms_sample_batch_typed's part of a batch (NULL: any other batch)
struct TypedBatch {
  const ggms_typed_t *t;
  ggms_id_t *const *eid;
  uint8_t *const *etype;
};

// ggms_sample_batch_temporal's part of a batch (NULL: any other batch)
struct TemporalBatch {
  const ggms_temporal_t *t;
  const uint32_t *seed_time;
  ggms_id_t *const *eid;
  uint32_t *node_cut;
};

// the body of ggms_sample_batch, ggms_sample_batch_prefetch, ggms_sample_batch_temporal and ggms_sample_batch_typed;
// every argument check is the caller's
static int sample_batch_impl(int sample_type, const ggms_graph_t *graph, const ggms_id_t *seeds, size_t num_seeds,
                             const size_t *fanouts, uint32_t num_layer, ggms_hashtable_t *ht, void *states,
                             size_t num_states, ggms_id_t *const *row, ggms_id_t *const *col, uint64_t *counts_dev,
                             const ggms_sample_extra_t *extra, void *workspace, const Prefetch *pf, hipStream_t s,
                             const TemporalBatch *tb = nullptr, const TypedBatch *yb = nullptr) {
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  // what every layer's sampler call shares; the loop below fills in the rest
  SampleLayer L{graph, nullptr, 0, 0, nullptr, nullptr, nullptr, (uint32_t *)states, nullptr, s};
  if (extra) {
    L.prob = extra->prob_table;
    L.alias = extra->alias_table;
    L.walk_length = extra->random_walk_length;
    L.num_walk = extra->num_random_walk;
    L.restart_prob = extra->random_walk_restart_prob;
  }
  // a stateless sampler has nothing to order between batches
  const bool ordered_rng = sample_type != GGMS_KHOP_LABOR && sample_type != GGMS_KHOP_TEMPORAL &&
                           sample_type != GGMS_KHOP_TYPED;
  if (tb) {
    L.edge_time = tb->t->edge_time;
    L.cut_table = tb->t->cut_table;
    L.stamp = tb->t->stamp;
    L.pick = (int)tb->t->pick;
    L.out_pos = tb->eid[0]; // layer_check's non-null test; every layer sets its own below
  }
  if (yb) {
    L.edge_type = yb->t->edge_type;
    L.num_type = yb->t->num_type;
    L.out_pos = yb->eid[0]; // layer_check's non-null tests; every layer sets its own below
    L.out_type = yb->etype[0];
  }
  for (uint32_t i = 0; i < num_layer; ++i) {
    L.n_max = c.max_input[i];
    L.fanout = fanouts[i];
    if (yb) L.type_fanout = yb->t->type_fanout + (size_t)i * L.num_type; // fanouts[i] must be this row's sum
    const int rc = layer_check(sample_type, L, num_states);
    if (rc != GGMS_OK) return rc;
  }

  const BatchLayout lay = layout_of(sample_type, num_seeds, fanouts, num_layer, c, extra,
                                    pf ? std::max<size_t>(pf->max_edges, 1) : 0, L.num_type);
  uint32_t *w = (uint32_t *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  uint32_t *seed_local = w + lay.seed_local;
  uint32_t *samp_ws = w + lay.samp_ws;
  uint32_t *item_pos = w + lay.cand;
  unsigned long long *lost = reinterpret_cast<unsigned long long *>(w + lay.lost);
  // every ordered scan of the batch (seed offsets, owner flags) shares one control/descriptor area that is
  // cleared once here: descriptors are epoch-tagged, the control words re-arm themselves
  ScanArea scan{w + lay.scan, true};
  L.workspace = samp_ws;
  L.scan = &scan;
  scan.chunk = w + lay.chunk;
  scan.tickets = scan.chunk + chunk_desc_words(); // chunk_desc_words() is a multiple of 4: the sets stay 16-byte aligned
  // every kernel of this batch reports a bound it hits into the BATCH's status word (behind the table's item counter;
  // zero since ggms_hashtable_init or the previous batch's last kernel), never into a word shared with the batches
  // in flight beside it (include/ggms.h, "Status words")
  scan.status = ht->num_items_dev + 1;

  if (!view_of(graph, L.g)) return GGMS_ERR_INVALID;
  // hash_table->Reset (dist_loops.cc:105): a new version stamp; the item count is zeroed by the prologue below
  if (ht->version >= 0x7ffffff0u) {
    int rc0 = ggms_hashtable_init(ht, (ggms_stream_t)s);
    if (rc0 != GGMS_OK) return rc0;
  }
  ht->version += 1;
  // FillWithDupRevised(seeds), dist_loops.cc:110-111, + the local ids of the raw seeds (they may repeat): the
  // first layer's `col`.  Its insert kernel is the first kernel of the batch and carries the prologue:
  // scan-area clear, item count reset, num_dst of the first layer = |seeds| (dist_loops.cc:305).
  BatchPrologue pro{scan_align(scan.words), (uint32_t)(8 + 2 * lay.scan_tiles),
                    scan.chunk, (uint32_t)(chunk_desc_words() + (size_t)kTicketSets * kTicketWords), ht->num_items_dev,
                    counts_dev + GGMS_COUNT_DST(num_layer - 1)};
  // direct table = batch mode of the dedup protocol (ggms_device.h): one index space for the whole batch, seeds first
  DedupInsert di{};
  di.cand = item_pos;
  di.lost = lost;
  di.batch = ht->direct ? 1u : 0u;
  di.base = 0;
  di.map.n = 1;
  di.map.base[0] = 0;
  di.map.arr[0] = seed_local;
  // Seeds the caller promises to be distinct (ggms_sample_extra_t.seeds_distinct), direct table: seed i is item i of the
  // unique list and its own local id -- no insert / ordered scan / look-up launches.  khop3 enters them inside the
  // first layer's launch (FirstLayer), every other sampler with one small launch (k_seed_enter).
  const bool distinct = extra && extra->seeds_distinct && ht->direct && num_seeds != 0;
  const bool fuse_seeds = distinct && sample_type == GGMS_KHOP3 && khop3_can_fuse_seeds(num_seeds) &&
                          c.max_edges[num_layer - 1] != 0;
  // khop0: its plan pass (both running sums of the first layer) reads the seeds anyway and enters them on the way
  const bool khop0_enters = distinct && sample_type == GGMS_KHOP0 && khop0_can_enter_seeds(num_seeds) &&
                            c.max_input[num_layer - 1] != 0;
  FirstLayer first_layer{};
  SeedEnter seed_enter{};
  int rc = GGMS_OK;
  if (distinct) {
    seed_local = nullptr;       // SrcMode: the first layer's `col` is the seed's position
    di.map.arr[0] = nullptr;    // IdxMap: segment 0 is the identity
    pro.items_are_seeds = 1;
    if (khop0_enters) {
      // as below: the prologue must leave alone the descriptors its own launch publishes (epoch-tagged; the rest of
      // the area is zeroed as usual)
      const size_t used = khop0_plan_desc_words(num_seeds);
      pro.num_zero = 8;
      pro.zero_words3 = pro.zero_words + 8 + used;
      pro.num_zero3 = (uint32_t)(2 * lay.scan_tiles > used ? 2 * lay.scan_tiles - used : 0);
      seed_enter = SeedEnter{(unsigned long long *)ht->o2n, ht->version, ht->n2o, pro};
    } else if (fuse_seeds) {
      // the prologue rides on the first layer's launch and must leave alone the tile descriptors that launch uses
      // (words [8, 8 + 2 tiles) of the area; they are epoch-tagged like every descriptor shared inside a batch)
      const size_t tiles0 = (num_seeds + 127) / 128;
      pro.num_zero = 8;
      pro.zero_words3 = pro.zero_words + 8 + 2 * tiles0;
      pro.num_zero3 = (uint32_t)(lay.scan_tiles > tiles0 ? 2 * (lay.scan_tiles - tiles0) : 0);
      first_layer.pro = pro;
      first_layer.n2o = ht->n2o;
    } else {
      rc = seed_enter_impl(ht, seeds, num_seeds, pro, s);
    }
  } else {
    rc = ht_fill_impl(ht, seeds, num_seeds, count_of(num_seeds), di, false, scan, nullptr, nullptr, s, seed_local, &pro,
                      kRestNow, pro.record_n);
  }
  if (rc != GGMS_OK) return rc;
  // khop_temporal: cut[seed] = min over the raw seeds' times, entered before the first layer's snapshot of the table
  if (tb) rc = temporal_seed_cut_impl(seeds, tb->seed_time, num_seeds, L.cut_table, L.stamp, s);
  if (rc != GGMS_OK) return rc;
  uint32_t next_base = (uint32_t)num_seeds;

  MapRestJobs jobs{};
  uint32_t num_jobs = 0;
  size_t job_items = 0;
  for (int i = (int)num_layer - 1; i >= 0; --i) {
    const bool first = (i == (int)num_layer - 1);
    const bool last_pf = pf && i == 0; // the prefetching batch's last layer (num_layer >= 2: never the first)
    uint32_t *tmp_dst = w + lay.tmp_dst[i];
    const size_t n_max = c.max_input[i], e_max = c.max_edges[i];
    // the last layer of a prefetching batch samples from the set BEFORE the expansion: its size as the previous fill
    // recorded it (num_dst(0)), not the table's count
    uint64_t *num_dst0 = counts_dev + GGMS_COUNT_DST(0);
    const Count n = first ? count_of(num_seeds) : (last_pf ? count_of(n_max, num_dst0) : count_of32(n_max, ht->num_items_dev));
    uint64_t *num_edge = counts_dev + GGMS_COUNT_EDGES(i);
    uint64_t *num_src = counts_dev + GGMS_COUNT_SRC(i);                 // unique nodes after this layer (:304)
    uint64_t *next_dst = i > 0 ? counts_dev + GGMS_COUNT_DST(i - 1)     // = next layer's frontier size (:305)
                               : counts_dev + GGMS_COUNT_INPUT(num_layer); // = number of input nodes
    // batch order on the shared RNG pool (and on khop2's CSR): only the sampler kernels are ordered
    if (first && ordered_rng && extra && extra->rng_wait) GGMS_HIP(hipStreamWaitEvent(s, (hipEvent_t)extra->rng_wait, 0));
    di.w = (unsigned long long *)ht->o2n;
    di.version = ht->version;
    if (last_pf) { // the expansion: one more fill of the batch, over every neighbour of n2o[0, k).  Layer 0: num_src
                   // is num_src(0), next_dst the input count
      if (pf->start) GGMS_HIP(hipEventRecord(pf->start, s));
      uint32_t *keys = w + lay.pf_keys, *local = w + lay.pf_local;
      uint64_t *total = reinterpret_cast<uint64_t *>(w + lay.pf_total);
      rc = prefetch_list_impl(L.g, ht->n2o, n_max, num_dst0, w + lay.pf_pre, w + lay.pf_scan, scan.status, total,
                              pf->max_edges, counts_dev + GGMS_COUNT_EXPANSION(num_layer), keys, s);
      if (rc != GGMS_OK) return rc;
      if (pf->max_edges == 0) { // no list to enter: the set is final as it is
        hipLaunchKernelGGL(k_record, dim3(1), dim3(64), 0, s, num_src, count_of32(0, ht->num_items_dev));
        hipLaunchKernelGGL(k_record, dim3(1), dim3(64), 0, s, next_dst, count_of32(0, ht->num_items_dev));
        GGMS_LAUNCH_CHECK();
      } else { // new nodes join n2o in first-occurrence order; num_src(0) and the input count get the new size
        di.base = next_base;
        rc = ht_fill_impl(ht, keys, pf->max_edges, count_of(pf->max_edges, total), di, false, scan, num_src, next_dst, s,
                          local, nullptr, kRestDefer, nullptr);
        if (rc != GGMS_OK) return rc;
        di.map.base[di.map.n] = next_base; // the last layer's look-ups find the new nodes' ids in `local`
        di.map.arr[di.map.n] = local;
        ++di.map.n;
        next_base += (uint32_t)pf->max_edges;
      }
      if (pf->final) GGMS_HIP(hipEventRecord(pf->final, s));
    }
    if (i == 0 && extra && extra->heavy_wait) GGMS_HIP(hipStreamWaitEvent(s, (hipEvent_t)extra->heavy_wait, 0));
    di.base = next_base; // this layer's edges take the indices [base, base + e_max)
    const bool inserted = !last_pf && ht->direct != 0 && e_max != 0 && layer_enters_output(sample_type);
    if (inserted) di.tag = next_dedup_tag();
    if (n_max == 0) {
      GGMS_HIP(hipMemsetAsync(num_edge, 0, sizeof(uint64_t), s));
    } else {
      L.input = first ? seeds : ht->n2o;
      L.n_max = n_max;
      L.n = n;
      L.fanout = fanouts[i]; // random walk: num_neighbor = K (operation.cc:174)
      L.salt = labor_layer_salt(extra ? extra->labor_salt : 0u, (uint32_t)i);
      L.out_src = col[i];
      L.out_dst = tmp_dst;
      L.num_out = num_edge;
      L.src = SrcMode{first ? seed_local : nullptr, 1};
      L.insert = inserted ? &di : nullptr;
      L.first = first && fuse_seeds ? &first_layer : nullptr;
      L.enter = first && khop0_enters ? &seed_enter : nullptr;
      if (sample_type == GGMS_RANDOM_WALK) L.out_data = extra->data[i];
      if (tb) L.out_pos = tb->eid[i];
      if (yb) {
        L.type_fanout = yb->t->type_fanout + (size_t)i * L.num_type;
        L.out_pos = yb->eid[i];
        L.out_type = yb->etype[i];
      }
      rc = sample_layer(sample_type, L);
    }
    if (rc != GGMS_OK) return rc;
    if (i == 0 && ordered_rng && extra && extra->rng_done) GGMS_HIP(hipEventRecord((hipEvent_t)extra->rng_done, s));
    const Count ne = count_of(e_max, num_edge);
    if (e_max == 0) { // nothing can be sampled: the counts are the current table size
      hipLaunchKernelGGL(k_record, dim3(1), dim3(64), 0, s, num_src, count_of32(0, ht->num_items_dev));
      hipLaunchKernelGGL(k_record, dim3(1), dim3(64), 0, s, next_dst, count_of32(0, ht->num_items_dev));
      GGMS_LAUNCH_CHECK();
      continue;
    }
    if (last_pf) { // every sampled neighbour is in the table already: row = its id, looked up with the other layers'
      GGMS_HIP(hipMemsetAsync(row[i], 0xff, e_max * sizeof(uint32_t), s));
      jobs.row[num_jobs] = row[i];
      jobs.key[num_jobs] = tmp_dst;
      jobs.num[num_jobs] = num_edge;
      ++num_jobs;
      job_items = std::max(job_items, e_max);
      continue;
    }
    // FillWithDuplicates (:279) + the dst half of GPUMapEdges (:296): row[i] = local id of every sampled neighbour
    // (direct table: the instances that do not own their key are resolved for all layers at once, below)
    rc = ht_fill_impl(ht, tmp_dst, e_max, ne, di, inserted, scan, num_src, next_dst, s, row[i], nullptr,
                      ht->direct ? kRestDefer : kRestNow, nullptr);
    if (rc != GGMS_OK) return rc;
    if (ht->direct) {
      di.map.base[di.map.n] = next_base; // later fills (and the final look-ups) find this layer's local ids in row[i]
      di.map.arr[di.map.n] = row[i];
      ++di.map.n;
      next_base += (uint32_t)e_max;
      jobs.row[num_jobs] = row[i];
      jobs.key[num_jobs] = tmp_dst;
      jobs.num[num_jobs] = num_edge;
      ++num_jobs;
      job_items = std::max(job_items, e_max);
    }
  }
  // khop_temporal: the final cut of every input node, by local id (the table keeps changing with the next batch)
  if (tb) {
    rc = temporal_node_cut_impl(ht->n2o, c.max_input[0] + c.max_edges[0],
                                count_of32(c.max_input[0] + c.max_edges[0], ht->num_items_dev), L.cut_table, L.stamp,
                                tb->node_cut, s);
    if (rc != GGMS_OK) return rc;
  }
  // the rest of GPUMapEdges' dst half for every layer + the batch's status word (GGMS_COUNT_STATUS)
  return launch_map_rest_all(ht, jobs, num_jobs, job_items, di.map, counts_dev + GGMS_COUNT_STATUS(num_layer), s);
}

int ggms_sample_batch(int sample_type, const ggms_graph_t *graph, const ggms_id_t *seeds, size_t num_seeds,
                      const size_t *fanouts, uint32_t num_layer, ggms_hashtable_t *ht, void *states,
                      size_t num_states, ggms_id_t *const *row, ggms_id_t *const *col, uint64_t *counts_dev,
                      const ggms_sample_extra_t *extra, void *workspace, size_t workspace_bytes,
                      ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph && fanouts && ht && row && col && counts_dev);
  GGMS_CHECK_ARG(num_layer >= 1 && num_layer <= 16);
  if (sample_type == GGMS_KHOP_TEMPORAL) {
    set_error("ggms_sample_batch: sample type %d (khop_temporal) takes edge times, seed times and a cut table: call "
              "ggms_sample_batch_temporal", sample_type);
    return GGMS_ERR_INVALID;
  }
  if (sample_type == GGMS_KHOP_TYPED) {
    set_error("ggms_sample_batch: sample type %d (khop_typed) takes edge types and a fanout per type and layer: call "
              "ggms_sample_batch_typed", sample_type);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(sample_type >= GGMS_KHOP0 && sample_type <= GGMS_KHOP_LABOR);
  GGMS_CHECK_ARG(num_seeds == 0 || seeds);
  GGMS_CHECK_ARG(workspace && workspace_bytes >= ggms_sample_batch_workspace_bytes(sample_type, num_seeds, fanouts,
                                                                                   num_layer, extra));
  GGMS_CHECK_ARG(sample_type != GGMS_RANDOM_WALK || (extra && extra->data)); // the visit counts of every layer
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] <= ht->n2o_size);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] < (1ull << 32) - 4); // indices and 2 + local id fit 32 bits
  return sample_batch_impl(sample_type, graph, seeds, num_seeds, fanouts, num_layer, ht, states, num_states, row, col,
                           counts_dev, extra, workspace, nullptr, to_stream(stream));
}

// The raw seeds' local ids are `seed_local`, a piece of its own that only the batch's look-ups read after the seeds'
// fill has written it (kRestNow: every position, owners or not): it survives to the end of the batch as it is.
int ggms_sample_batch_seed_ids(int sample_type, size_t num_seeds, const size_t *fanouts, uint32_t num_layer,
                               const ggms_sample_extra_t *extra, const void *workspace, const ggms_id_t **seed_ids_dev) {
  GGMS_CHECK_ARG(fanouts && workspace && seed_ids_dev);
  GGMS_CHECK_ARG(num_layer >= 1 && num_layer <= 16);
  GGMS_CHECK_ARG(sample_type >= GGMS_KHOP0 && sample_type <= GGMS_KHOP_TYPED);
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  const BatchLayout lay = layout_of(sample_type, num_seeds, fanouts, num_layer, c, extra);
  const uint32_t *w = (const uint32_t *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  *seed_ids_dev = w + lay.seed_local;
  return GGMS_OK;
}

// ---- khop_temporal: the batch with per-seed times and a cut table --------------------------------------------------
size_t ggms_sample_batch_temporal_workspace_bytes(size_t num_seeds, const size_t *fanouts, uint32_t num_layer,
                                                  const ggms_sample_extra_t *extra) {
  return ggms_sample_batch_workspace_bytes(GGMS_KHOP_TEMPORAL, num_seeds, fanouts, num_layer, extra);
}

int ggms_sample_batch_temporal(const ggms_graph_t *graph, const ggms_id_t *seeds, const uint32_t *seed_time,
                               size_t num_seeds, const size_t *fanouts, uint32_t num_layer, ggms_hashtable_t *ht,
                               ggms_id_t *const *row, ggms_id_t *const *col, ggms_id_t *const *eid, uint32_t *node_cut,
                               uint64_t *counts_dev, const ggms_temporal_t *t, const ggms_sample_extra_t *extra,
                               void *workspace, size_t workspace_bytes, ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph && fanouts && ht && row && col && eid && node_cut && counts_dev && t);
  GGMS_CHECK_ARG(num_layer >= 1 && num_layer <= 16);
  GGMS_CHECK_ARG(graph->num_part == 0); // edge positions are those of one CSR
  GGMS_CHECK_ARG(t->edge_time && t->cut_table && t->stamp != 0);
  GGMS_CHECK_ARG(t->pick == GGMS_PICK_UNIFORM || t->pick == GGMS_PICK_RECENT);
  GGMS_CHECK_ARG(num_seeds == 0 || (seeds && seed_time));
  for (uint32_t i = 0; i < num_layer; ++i) GGMS_CHECK_ARG(row[i] && col[i] && eid[i]);
  GGMS_CHECK_ARG(workspace && workspace_bytes >= ggms_sample_batch_temporal_workspace_bytes(num_seeds, fanouts,
                                                                                            num_layer, extra));
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] <= ht->n2o_size);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] < (1ull << 32) - 4); // indices and 2 + local id fit 32 bits
  // the seeds may repeat with different times: never the distinct-seeds path, whatever the caller promises
  ggms_sample_extra_t ex{};
  if (extra) ex = *extra;
  ex.seeds_distinct = 0;
  const TemporalBatch tb{t, seed_time, eid, node_cut};
  return sample_batch_impl(GGMS_KHOP_TEMPORAL, graph, seeds, num_seeds, fanouts, num_layer, ht, nullptr, 0, row, col,
                           counts_dev, &ex, workspace, nullptr, to_stream(stream), &tb);
}

// ---- khop_typed: the batch with a fanout per edge type and layer ---------------------------------------------------
size_t ggms_sample_batch_typed_workspace_bytes(size_t num_seeds, const size_t *fanouts, uint32_t num_layer,
                                               uint32_t num_type, const ggms_sample_extra_t *extra) {
  if (!fanouts || num_layer < 1 || num_layer > 16 || num_type < 1 || num_type > GGMS_MAX_EDGE_TYPES) return 0;
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  return layout_of(GGMS_KHOP_TYPED, num_seeds, fanouts, num_layer, c, extra, 0, num_type).total * sizeof(uint32_t) + 16;
}

int ggms_sample_batch_typed(const ggms_graph_t *graph, const ggms_id_t *seeds, size_t num_seeds, const size_t *fanouts,
                            uint32_t num_layer, ggms_hashtable_t *ht, ggms_id_t *const *row, ggms_id_t *const *col,
                            ggms_id_t *const *eid, uint8_t *const *etype, uint64_t *counts_dev, const ggms_typed_t *t,
                            const ggms_sample_extra_t *extra, void *workspace, size_t workspace_bytes,
                            ggms_stream_t stream) {
  GGMS_CHECK_ARG(graph && fanouts && ht && row && col && eid && etype && counts_dev && t);
  GGMS_CHECK_ARG(num_layer >= 1 && num_layer <= 16);
  GGMS_CHECK_ARG(graph->num_part == 0); // edge positions are those of one CSR
  GGMS_CHECK_ARG(t->edge_type && t->type_fanout);
  GGMS_CHECK_ARG(t->num_type >= 1 && t->num_type <= GGMS_MAX_EDGE_TYPES);
  for (uint32_t i = 0; i < num_layer; ++i) { // every row: k_r < 128, and fanouts[i] is its sum (>= 1)
    size_t sum = 0;
    const int rc = typed_fanout_sum(t->type_fanout + (size_t)i * t->num_type, t->num_type, &sum);
    if (rc != GGMS_OK) return rc;
    GGMS_CHECK_ARG(sum >= 1 && sum == fanouts[i]);
  }
  GGMS_CHECK_ARG(num_seeds == 0 || seeds);
  for (uint32_t i = 0; i < num_layer; ++i) GGMS_CHECK_ARG(row[i] && col[i] && eid[i] && etype[i]);
  GGMS_CHECK_ARG(workspace && workspace_bytes >= ggms_sample_batch_typed_workspace_bytes(num_seeds, fanouts, num_layer,
                                                                                         t->num_type, extra));
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] <= ht->n2o_size);
  GGMS_CHECK_ARG(c.max_input[0] + c.max_edges[0] < (1ull << 32) - 4); // indices and 2 + local id fit 32 bits
  const TypedBatch yb{t, eid, etype};
  return sample_batch_impl(GGMS_KHOP_TYPED, graph, seeds, num_seeds, fanouts, num_layer, ht, nullptr, 0, row, col,
                           counts_dev, extra, workspace, nullptr, to_stream(stream), nullptr, &yb);
}

// ---- arch4: the prefetching batch ----------------------------------------------------------------------------------
int ggms_sample_batch_prefetch_capacity(size_t num_seeds, const size_t *fanouts, uint32_t num_layer,
                                        const ggms_id_t *indptr, size_t num_node, size_t max_edges_budget,
                                        size_t *max_prefetch_edges, size_t *max_input_nodes) {
  GGMS_CHECK_ARG(fanouts && num_layer >= 2 && num_layer <= 16 && (indptr || num_node == 0));
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  const size_t k = std::min(c.max_input[0], num_node); // unique nodes after L - 1 layers
  // the k largest degrees bound the expansion's edges (every node of the set contributes its whole list)
  std::vector<uint32_t> deg(num_node);
  for (size_t v = 0; v < num_node; ++v) deg[v] = indptr[v + 1] - indptr[v];
  if (k < num_node) std::nth_element(deg.begin(), deg.begin() + k, deg.end(), std::greater<uint32_t>());
  size_t top = 0;
  for (size_t v = 0; v < k; ++v) top += deg[v];
  const size_t e = std::min(top, max_edges_budget);
  if (max_prefetch_edges) *max_prefetch_edges = e;
  if (max_input_nodes) *max_input_nodes = std::min(num_node, k + e);
  return GGMS_OK;
}

size_t ggms_sample_batch_prefetch_workspace_bytes(int sample_type, size_t num_seeds, const size_t *fanouts,
                                                  uint32_t num_layer, const ggms_sample_extra_t *extra,
                                                  size_t max_prefetch_edges) {
  if (!fanouts || num_layer < 2 || num_layer > 16) return 0;
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  // pf_edges = 0 would drop the pieces: keep them (4 words each) for an expansion that can have no edge
  return layout_of(sample_type, num_seeds, fanouts, num_layer, c, extra, std::max<size_t>(max_prefetch_edges, 1)).total *
             sizeof(uint32_t) + 16;
}

int ggms_sample_batch_prefetch(int sample_type, const ggms_graph_t *graph, const ggms_id_t *seeds, size_t num_seeds,
                               const size_t *fanouts, uint32_t num_layer, ggms_hashtable_t *ht, void *states,
                               size_t num_states, ggms_id_t *const *row, ggms_id_t *const *col, uint64_t *counts_dev,
                               const ggms_sample_extra_t *extra, size_t max_prefetch_edges, ggms_event_t expand_start,
                               ggms_event_t input_final, void *workspace, size_t workspace_bytes,
                               ggms_stream_t stream) {
  // the reference's switch (cuda_loops.cc:347-377) builds the dynamic-cache batch for these three samplers only
  if (sample_type != GGMS_KHOP0 && sample_type != GGMS_KHOP1 && sample_type != GGMS_WEIGHTED_KHOP) {
    set_error("ggms_sample_batch_prefetch: sample type %d is not supported (khop0, khop1 and weighted_khop only)",
              sample_type);
    return GGMS_ERR_INVALID;
  }
  // without a second-to-last layer the reference never enters the last layer's samples, so it cannot remap them
  if (num_layer < 2 || num_layer > 16) {
    set_error("ggms_sample_batch_prefetch: num_layer %u (2 .. 16 layers: the expansion follows the second-to-last)",
              num_layer);
    return GGMS_ERR_INVALID;
  }
  GGMS_CHECK_ARG(graph && fanouts && ht && row && col && counts_dev);
  GGMS_CHECK_ARG(ht->direct); // one word per node id: the superset can be far beyond PredictNumNodes
  GGMS_CHECK_ARG(num_seeds == 0 || seeds);
  GGMS_CHECK_ARG(workspace && workspace_bytes >= ggms_sample_batch_prefetch_workspace_bytes(
                                                     sample_type, num_seeds, fanouts, num_layer, extra, max_prefetch_edges));
  const BatchCaps c = caps_of(num_seeds, fanouts, num_layer);
  const size_t k = c.max_input[0];
  GGMS_CHECK_ARG(std::min<size_t>(graph->num_node, k + max_prefetch_edges) <= ht->n2o_size);
  // the batch's index space: seeds, the first L - 1 layers, the expansion, the last layer
  GGMS_CHECK_ARG(k + max_prefetch_edges + c.max_edges[0] < (1ull << 32) - 4);
  const Prefetch pf{max_prefetch_edges, (hipEvent_t)expand_start, (hipEvent_t)input_final};
  return sample_batch_impl(sample_type, graph, seeds, num_seeds, fanouts, num_layer, ht, states, num_states, row, col,
                           counts_dev, extra, workspace, &pf, to_stream(stream));
}

} // extern "C"
