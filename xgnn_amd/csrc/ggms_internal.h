// ggms_internal.h -- cross-file C++ entry points (count-on-device variants of the leaf ops).
#pragma once
#include "tile_scan.h"

namespace ggms {

// What goes into out_src: the seed's global id (leaf API, like the reference) or
// its local id (fused batch path: the COO `col` is written by the sampler itself).
struct SrcMode {
  const uint32_t *seed_local; // local id per seed position; NULL = the position itself
  int local;
  __device__ __forceinline__ uint32_t value(uint32_t rid, uint64_t index) const {
    if (!local) return rid;
    return seed_local ? seed_local[index] : (uint32_t)index;
  }
};

// What the first kernel of a batch (the insert of the seeds) does on the side: clear the shared scan area's
// control words + single-pass descriptors, reset the table's item count, record |seeds|.
struct BatchPrologue {
  uint32_t *zero_words;
  uint32_t num_zero;
  uint32_t *zero_words2; // second range (the chunked owner scan's descriptors)
  uint32_t num_zero2;
  uint32_t *num_items;
  uint64_t *record_n;
  uint32_t *zero_words3 = nullptr; // third range (fused first layer: the descriptors behind the ones it uses itself)
  uint32_t num_zero3 = 0;
  uint32_t items_are_seeds = 0;    // distinct seeds: the table's item count starts at |seeds| instead of 0
  __device__ __forceinline__ void run(uint64_t n, uint32_t tid, uint32_t nthreads) const { // by ONE workgroup
    for (uint32_t z = tid; z < num_zero; z += nthreads) zero_words[z] = 0u;
    for (uint32_t z = tid; z < num_zero2; z += nthreads) zero_words2[z] = 0u;
    for (uint32_t z = tid; z < num_zero3; z += nthreads) zero_words3[z] = 0u;
    if (tid == 0) {
      if (num_items) *num_items = items_are_seeds ? (uint32_t)n : 0u;
      if (record_n) *record_n = n;
    }
  }
};
// distinct seeds entered by the first layer's own launch (khop3): the batch prologue rides on it, the seeds become
// the head of the unique list where they are read
struct FirstLayer {
  BatchPrologue pro;
  uint32_t *n2o;
};
bool khop3_can_fuse_seeds(size_t num_seeds); // every tile of the first layer has a workgroup of its own
// distinct seeds, any sampler: one launch -- table entries, head of the unique list, batch prologue (hashtable.hip)
int seed_enter_impl(const ggms_hashtable_t *ht, const uint32_t *seeds, size_t num_seeds, const BatchPrologue &pro,
                    hipStream_t s);
// distinct seeds entered by khop0's plan pass (the first kernel of the batch): table words, head of the unique list,
// batch prologue -- k_seed_enter's work without its launch
struct SeedEnter {
  unsigned long long *w;
  uint32_t version;
  uint32_t *n2o;
  BatchPrologue pro;
};
bool khop0_can_enter_seeds(size_t num_seeds); // its plan pass is one launch
size_t khop0_plan_desc_words(size_t num_seeds); // descriptor words of the batch's scan area that launch uses itself

constexpr uint64_t kWeightedMaxThreads = 512 * 1024; // Constant::kWeightedKHopMaxThreads, constant.h:72
constexpr uint32_t kDedupSlots = 50; // table slots per seed of weighted_khop_hash_dedup: fanout < 50, hash_dedup.cu:42

// One sampler call: a layer of ggms_sample_batch or a leaf entry point.  The leaf path leaves `src` at {nullptr, 0}
// and the batch's pieces (scan, insert, first, enter) null.  Sizes are the caller's; the samplers narrow them.
struct SampleLayer {
  const ggms_graph_t *graph;
  const uint32_t *input;
  size_t n_max;                  // bound of n: grids and workspace pieces are sized from it
  size_t fanout;                 // random walk: K
  uint32_t *out_src, *out_dst;
  uint64_t *num_out;             // device
  uint32_t *states, *workspace;
  hipStream_t s;
  Count n = {};
  GraphView g = {};              // view_of(graph)
  SrcMode src = {};
  ScanArea *scan = nullptr;             // the batch's scan area; else the workspace holds a private one
  const DedupInsert *insert = nullptr;  // direct table: the sampler enters its output itself
  const FirstLayer *first = nullptr;    // khop3: the batch's distinct seeds ride on the first layer
  const SeedEnter *enter = nullptr;     // khop0: its plan pass enters the batch's distinct seeds
  const float *prob = nullptr;          // weighted family
  const uint32_t *alias = nullptr;
  uint32_t *out_data = nullptr;         // random walk: visit counts
  size_t walk_length = 0, num_walk = 0;
  double restart_prob = 0;
  uint32_t salt = 0;                    // khop_labor, khop_temporal: the layer salt
  // khop_temporal: per-position times; the seeds' cuts (leaf) or the batch's cut table + stamp; the positions' output
  const uint32_t *edge_time = nullptr;
  const uint32_t *input_cut = nullptr;
  uint64_t *cut_table = nullptr;
  uint32_t stamp = 0;
  int pick = 0;
  uint32_t *out_pos = nullptr;
  // khop_typed: per-position types, their number R, the R type fanouts of this layer (host; `fanout` is their sum), the
  // types' output.  Shares out_pos with khop_temporal
  const uint8_t *edge_type = nullptr;
  uint32_t num_type = 0;
  const uint32_t *type_fanout = nullptr;
  uint8_t *out_type = nullptr;
};

// sample_khop.hip
size_t sample_ws_words(size_t num_input);
size_t khop0_ws_words(size_t num_input, size_t fanout);
int sample_khop3_impl(const SampleLayer &l);
int sample_khop0_impl(const SampleLayer &l);
int sample_khop2_impl(const SampleLayer &l);
// sample_weighted.hip
size_t weighted_ws_words(size_t num_input, size_t fanout);
int sample_weighted_impl(const SampleLayer &l, int type); // khop1, weighted_khop, weighted_khop_prefix
int sample_weighted_hash_dedup_impl(const SampleLayer &l);
// sample_random_walk.hip
size_t random_walk_ws_words(size_t num_input, size_t walk_length, size_t num_walk, size_t K);
int sample_random_walk_impl(const SampleLayer &l);
size_t walk_scan_tiles(size_t num_input);

// sample_labor.hip
size_t labor_ws_words(size_t num_input);
int sample_khop_labor_impl(const SampleLayer &l);

// sample_temporal.hip
size_t temporal_ws_words(size_t num_input);
int sample_khop_temporal_impl(const SampleLayer &l);
int temporal_seed_cut_impl(const uint32_t *seeds, const uint32_t *seed_time, size_t num_seeds, uint64_t *cut_table,
                           uint32_t stamp, hipStream_t s); // cut[seed] = min(cut[seed], seed_time), under `stamp`
int temporal_node_cut_impl(const uint32_t *n2o, size_t n_max, Count n, const uint64_t *cut_table, uint32_t stamp,
                           uint32_t *node_cut, hipStream_t s); // node_cut[local id] = cut[n2o[local id]]

// sample_typed.hip
size_t typed_ws_words(size_t num_input, size_t num_type); // num_type 0: sized for GGMS_MAX_EDGE_TYPES
int typed_fanout_sum(const uint32_t *type_fanout, uint32_t num_type, size_t *sum); // refuses R, a null row, a k_r >= 128
int sample_khop_typed_impl(const SampleLayer &l);

// sample_batch.hip: the per-sampler rules, one copy for the leaf entry points and ggms_sample_batch
size_t layer_ws_words(int type, size_t n, size_t fanout, size_t walk_length, size_t num_walk, size_t num_type = 0);
int sample_leaf(int type, SampleLayer l, size_t num_states, size_t workspace_bytes); // a leaf entry point's body

// hashtable.hip
size_t ht_ws_words(size_t num_input);
size_t chunk_desc_words(); // 32-bit descriptors of the chunked owner scan: their own piece of a scan area
// the end-of-batch id look-ups of the instances that do not own their key: one job per layer
struct MapRestJobs {
  uint32_t *row[16];
  const uint32_t *key[16];
  const uint64_t *num[16];
};
int launch_map_rest_all(const ggms_hashtable_t *ht, const MapRestJobs &jobs, uint32_t num_jobs, size_t max_items,
                        const IdxMap &map, uint64_t *status_out, hipStream_t s);
size_t owner_scan_tiles(size_t n_max);
// insert + ordered local-id assignment (see DedupInsert in ggms_device.h for the two modes).
// di: cand (n_max words; hashed layout: bucket positions) + lost (n_max 64-bit words), and in batch mode the index
//     base of this fill + the IdxMap of the fills before it; w / version / tag are filled in here.
// inserted: the producer of `input` already entered every item with exactly this `di` (fused sampler).
// mirror_a/b (optional): 64-bit device slots that also receive the new item count.
// mapped (optional): mapped[i] = local id of input[i] (the dst half of GPUMapEdges, fused).
// rest: kRestNow resolves the instances that do not own their key here (batch mode: needs n_dev_for_rest, a device
//       copy of the item count, and di.map must already include this fill); kRestDefer leaves kEmptyKey for the
//       caller's launch_map_rest_all at the end of the batch.
constexpr int kRestNow = 0, kRestDefer = 1;
int ht_fill_impl(const ggms_hashtable_t *ht, const uint32_t *input, size_t n_max, Count n, DedupInsert di,
                 bool inserted, ScanArea scan, uint64_t *mirror_a, uint64_t *mirror_b, hipStream_t s, uint32_t *mapped,
                 const BatchPrologue *prologue, int rest, const uint64_t *n_dev_for_rest);

// prefetch.hip: arch4's expansion list.  pre: max_nodes words; scan_words: prefetch_scan_words(max_nodes); the scan's
// total goes to *total_dev and *need_dev; a total above max_edges sets GGMS_STATUS_PREFETCH_FULL in *status and zeroes
// *total_dev and *num_nodes_dev.  keys: max_edges words.
size_t prefetch_scan_words(size_t max_nodes);
int prefetch_list_impl(const GraphView &g, const uint32_t *nodes, size_t max_nodes, uint64_t *num_nodes_dev,
                       uint32_t *pre, uint32_t *scan_words, uint32_t *status, uint64_t *total_dev, size_t max_edges,
                       uint64_t *need_dev, uint32_t *keys, hipStream_t s);

// extract.hip: hands the launch timer armed on this thread (include/ggms.h) to the launch about to be issued -- its
// start / stop events for hipExtLaunchKernel -- and disarms it; false if none is armed
bool take_armed_timer(hipEvent_t *start, hipEvent_t *stop);
// extract.hip: GGMS_EXTRACT_BLOCKS, the cap on a row gather's workgroups (read once)
int gather_max_blocks();

} // namespace ggms
