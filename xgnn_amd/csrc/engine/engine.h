// engine.h -- host orchestration behind the samgraph_* ABI (include/samgraph.h).
//
// Counterpart of the reference's Engine / GPUEngine / DistEngine
// (samgraph/common/engine.{h,cc}, cuda/cuda_engine.cc, dist/dist_engine.cc) for the
// deployments on the hot path: arch1 (one process, one GPU), arch3 (one process, a
// sampler GPU and a trainer GPU), arch5 (sampler processes and trainer processes joined by a batch queue in shared host
// memory) and arch6 (one process per GPU, GGMS shards).  It owns device memory (hipMalloc, no framework allocator),
// streams, the shuffler, the sampler state and the feature cache, and drives the
// leaf operators of include/ggms.h.  Everything below is plain C++17 + HIP runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../../include/ggms.h"
#include "../../../include/samgraph.h"

namespace sam {

// ---- fatal checks: print + abort like LOG(FATAL)/CHECK (logging.cc:69-73) ----
[[noreturn]] void fatal(const char *file, int line, const std::string &msg);
#define SAM_CHECK(cond, msg)                                   \
  do {                                                         \
    if (!(cond)) ::sam::fatal(__FILE__, __LINE__, std::string("Check failed: " #cond " ") + (msg)); \
  } while (0)
#define SAM_HIP(call)                                          \
  do {                                                         \
    hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) ::sam::fatal(__FILE__, __LINE__, std::string(#call " -> ") + hipGetErrorString(e_)); \
  } while (0)
#define SAM_GGMS(call)                                         \
  do {                                                         \
    int rc_ = (call);                                          \
    if (rc_ != 0) ::sam::fatal(__FILE__, __LINE__, std::string(#call " -> ") + ggms_last_error()); \
  } while (0)
void log_info(const std::string &msg);
int parse_device(const std::string &ctx); // the N of "cuda:N" / "cpu:N", or SAMGRAPH_FORCE_DEVICE

// ---- RunConfig: run_config.h + operation.cc:64-326 -----------------------------
enum Arch { kArch0 = 0, kArch1, kArch2, kArch3, kArch4, kArch5, kArch6, kArch7 };
struct RunConfig {
  std::unordered_map<std::string, std::string> raw;
  std::string dataset_path;
  int arch = kArch1;
  int sample_type = GGMS_KHOP3;
  size_t batch_size = 8000, num_epoch = 1;
  int cache_policy = 0;
  double cache_percentage = 0.0;
  size_t num_layer = 0;
  std::vector<size_t> fanout;
  size_t random_walk_length = 0, num_random_walk = 0, num_neighbor = 0;
  double random_walk_restart_prob = 0.0;
  size_t num_worker = 1;
  // arch5: S sampler processes, T trainer processes; the batch queue's ring size and the deadline of every wait on it
  size_t num_sample_worker = 0, num_train_worker = 0, queue_depth = 0;
  double queue_timeout_s = 300.0;
  int sampler_device = 0, trainer_device = 0;
  bool trainer_on_host = false; // arch0 with trainer_ctx = cpu:N (host-only plumbing runs)
  size_t omp_thread_num = 1;    // arch0: threads of the sampling / extract loops (RunConfig::omp_thread_num)
  bool use_dist_graph = false;
  double dist_graph_percentage = 0.0;
  bool part_cache = false, gpu_extract = false;
  double replicate_percentage = 0.0; // of the cached slots, hottest first: kept on every GPU (hybrid store)
  bool configured = false;
  // extensions (optional keys)
  bool has_seed = false;
  uint64_t seed = 0;
  uint64_t labor_seed = 0; // khop_labor's batch salts: `seed`, or a wall-clock base taken once, when the run is configured
  bool direct_table = true;
  size_t lookahead = 2; // batches sample_once() keeps enqueued beyond the one it was asked for (config key `lookahead`)
  size_t extract_streams = 2; // lean batches' gathers alternate between this many streams (1 or 2; config key `extract_streams`)
  size_t pipelines = 1; // batches the sampler itself has in flight: own stream + dedup table + workspace each (`pipelines`);
                        // measured on papers100M-shaped GCN: a second pipeline loses 2-3 % (the step is bound by the memory
                        // fabric, not by sampler latency) and costs a second 8 B x num_node table
  size_t presample_epoch = 0;
  // arch4: dynamic_cache (cache_policy 6) -- the trainer GPU keeps the previous batch's rows; the expansion's edge
  // budget of one batch (config key `prefetch_max_edges`; ggms_sample_batch_prefetch_capacity)
  bool dynamic_cache = false;
  size_t prefetch_max_edges = (size_t)1 << 26;
  // extension (config key `feat_out_dtype` = f32 | f16 | bf16): the dtype the batch's feature rows are DELIVERED in; the
  // gather converts from the table's (FEAT_DATA_TYPE) in its one pass.  -1: key absent, the table's dtype
  int feat_out_dtype = -1;
  // extension (config key `feat_store_dtype` = F16 | BF16 | F8E4M3 | F8E5M2 | Q8ROW): the F32 / F16 table on disk is
  // encoded into this type by the trainer GPU before the cache is built (Engine::QuantizeStore); from then on the
  // dataset is what a meta.txt naming the type would have loaded.  -1: key absent, the table stays as it is on disk
  int feat_store_dtype = -1;
  // extension (config key `inline_heads` = auto | 0 | 1; arch1, whole CSR on the GPU): the 64-byte-per-node table of
  // include/ggms.h ("Inline list heads"), built once at graph load and attached to the graph; khop3 then finds a
  // frontier node's list with one request.  -1 = auto: khop3, and 64 x num_node bytes at most a quarter of the free
  // device memory at that point.  1: build it or stop with a message.  0: never
  int inline_heads = -1;
  // extension (config keys `task` = node_classification | link_prediction, `num_negative` = 1 .. 64, `negative_mode` =
  // uniform | exclude; arch1): a batch is batch_size positive EDGES of the shuffled train edge set; its seed list is
  // their endpoints and num_negative negative destinations each (ggms_link_seeds), batch_size x (2 + num_negative) ids
  bool link_prediction = false;
  uint32_t num_negative = 1;
  int negative_mode = GGMS_NEG_EXCLUDE;
  // extension (config key `exclude_seed_edges` = none | self | both; read with task = link_prediction only): the batch's
  // positive edges (self), and their mirrors (both), leave its sampled layers (ggms_drop_pair_edges' `which`; 0 = none)
  uint32_t exclude_seed_edges = 0;
  // extension (config keys `feat_learnable` = sgd | adagrad, `feat_lr`, `feat_eps`; arch1, F32 tables): the device table
  // is LEARNABLE -- samgraph_update_graph_feat applies a batch's gradient to the rows the batch gathered
  // (ggms_update_rows' rule; -1: key absent, the table is read-only).  The other two keys are read with the first only
  int feat_learnable = -1;
  float feat_lr = 0.0f, feat_eps = 1e-10f;
  // extension (config keys `edge_ids` = on, `edge_feat` = on; arch1, one CSR, not random_walk / khop2): every layer of a
  // batch comes with its edges' CSR positions (ggms_edge_positions behind the sampler), and with edge_feat -- which
  // implies edge_ids -- with the rows of edge_feat.bin those positions name
  bool edge_ids = false, edge_feat = false;
  // extension (`_sample_type` 9 = khop_temporal, config key `temporal_pick` = uniform | recent; arch1, link_prediction,
  // one CSR): every seed is sampled strictly before the time of its positive edge (ggms_sample_batch_temporal).  Implies
  // edge_ids -- the sampler itself emits the positions, ggms_edge_positions is not enqueued
  int temporal_pick = GGMS_PICK_UNIFORM;
  bool Temporal() const { return sample_type == GGMS_KHOP_TEMPORAL; }
  // extension (`_sample_type` 10 = khop_typed, config key `type_fanout` = num_layer x NUM_EDGE_TYPE integers, layer-major;
  // arch1, one CSR, both tasks): a fanout per edge type (ggms_sample_batch_typed); `fanout` holds the rows' sums.  Implies
  // edge_ids like khop_temporal
  std::vector<uint32_t> type_fanout;
  uint32_t num_edge_type = 0; // type_fanout.size() / num_layer; LoadDataset checks it against meta.txt's NUM_EDGE_TYPE
  bool Typed() const { return sample_type == GGMS_KHOP_TYPED; }
  bool SamplerEmitsEdgeIds() const { return Temporal() || Typed(); } // ggms_edge_positions is not enqueued
  // extension (config keys `induced_subgraph` = on, `induced_max_edges`; arch1, one CSR, not khop2 / khop_temporal, no
  // exclude_seed_edges): every batch also carries the subgraph its input nodes induce -- every edge of the graph with
  // both ends among them, one COO over the batch's local ids with the edges' CSR positions (ggms_induced_edges behind
  // the sampler), and with edge_feat the edge table's rows under those.  induced_max_edges 0: the default, the sum of the
  // layers' edge capacities capped at NUM_EDGE (Engine::ResolveInducedCapacity)
  bool induced = false;
  size_t induced_max_edges = 0;
  // extension (config key `hetero_batch` = on; arch1 with _sample_type 10 (khop_typed), one CSR): every batch also carries
  // its heterogeneous view -- the input nodes grouped by node type, every layer's edges grouped by relation with ids local
  // to their types' lists (ggms_hetero_nodes / ggms_hetero_edges behind the sampler) -- and the feature rows are gathered
  // in the grouped order
  bool hetero = false;
  // extension (config key `typed_feat` = on; needs hetero_batch = on): the feature store is one table PER NODE TYPE, each
  // with its own width and element type (node_feat_<t>.bin, NODE_FEAT_DIM_<t>, NODE_FEAT_DATA_TYPE_<t>); a batch's rows are
  // gathered by ggms_gather_typed into per-type blocks of one buffer.  feat.bin is then neither mapped nor uploaded
  bool typed_feat = false;
  size_t staged_serial_epochs = 0; // host-staged path: the first N epochs run the reference's serial, per-phase-timed sequence
  size_t staged_serial_steps = 0;  // ... or this worker's first N batches
  // worker 0 ranks the nodes at init: pre_sample (sampled input nodes) or presample_static (L-hop closures)
  bool UsePresample() const {
    return UseGPUCache() && (cache_policy == 2 /*kCacheByPreSample*/ || cache_policy == 4 /*kCacheByPreSampleStatic*/);
  }
  bool UseGPUCache() const { return cache_percentage > 0 && arch != kArch1; } // run_config.h:124-126
};

// ---- Dataset: common.h:216-243 + engine.cc:109-443 -----------------------------
struct HostArray {
  void *ptr = nullptr;
  size_t bytes = 0;
  bool mapped_file = false, shared_anon = false, owned = false;
};
struct Dataset {
  size_t num_node = 0, num_edge = 0, num_class = 0, feat_dim = 0;
  int feat_dtype = GGMS_F32;
  size_t num_train = 0, num_valid = 0, num_test = 0;
  HostArray indptr, indices, feat, label, train_set, valid_set, test_set, ranking_nodes, prob_table, alias_table;
  // task = link_prediction: the train edge set, CSR positions below num_edge -- train_edge_set.bin, or every edge
  // (`all_edges`, built at load) where the dataset has no such file
  HostArray train_edge_set;
  std::vector<uint32_t> all_edges;
  const uint32_t *train_edges = nullptr;
  size_t num_train_edge = 0;
  bool feat_is_fake = false;
  bool feat_is_zero = false; // the stand-in table of a dataset without feat.bin that nobody has written: every row is zero
  // SAMGRAPH_EMPTY_FEAT = k (engine.cc:198-235): the feature table is a 2^k-row stand-in, row of node v = v & mask
  uint32_t feat_mask = 0xffffffffu;
  size_t feat_rows = 0; // rows of ds.feat (num_node, or 2^k)
  // bytes from one STORED row of the table to the next: what sizes and strides the table, the cache, its shards and
  // replicas and the staging buffers (feat_dim x element bytes; a Q8ROW row is its codes, pad and scale / bias trailer)
  size_t feat_row_bytes() const { return ggms_row_bytes(feat_dtype, feat_dim); }
  // edge_feat: edge_feat.bin, NUM_EDGE rows of EDGE_FEAT_DIM elements of EDGE_FEAT_DATA_TYPE (F32 without the key) in CSR
  // order
  size_t edge_feat_dim = 0;
  int edge_feat_dtype = GGMS_F32;
  HostArray edge_feat;
  // khop_temporal: edge_time.bin, NUM_EDGE uint32 in CSR order, non-decreasing inside every node's list (checked at load)
  HostArray edge_time;
  // khop_typed: edge_type.bin, NUM_EDGE uint8 in CSR order, non-decreasing inside every node's list and below NUM_EDGE_TYPE
  // (checked at load)
  HostArray edge_type;
  // hetero_batch: node_type.bin, NUM_NODE uint8 below NUM_NODE_TYPE, and every relation's (source type, destination type)
  // as its edges have them -- 255 / 255 for a relation without an edge
  HostArray node_type;
  uint32_t num_node_type = 0;
  std::vector<uint8_t> rel_src_type, rel_dst_type;
  // typed_feat: per node type its table (the mapped node_feat_<t>.bin; dim 0: the type has none), the number of nodes of
  // the type (= the table's rows) and its first node id.  Row k of a table belongs to the type's k-th node in ascending
  // id.  node_rank: every node's rank inside its type -- empty where node_type.bin is non-decreasing in the node id (the
  // rank is then node - first_node)
  struct NodeFeat {
    HostArray file;
    size_t dim = 0, rows = 0;
    int dtype = GGMS_F32;
    uint32_t first_node = 0;
    size_t row_bytes() const { return dim * ggms_dtype_bytes(dtype); }
  };
  std::vector<NodeFeat> node_feat;
  std::vector<uint32_t> node_rank;
  size_t edge_feat_row_bytes() const { return edge_feat_dim * ggms_dtype_bytes(edge_feat_dtype); }
};

// ---- Profiler log store: profiler.h:166-215 ------------------------------------
class Profiler {
 public:
  void Resize(size_t num_epoch, size_t num_step);
  void LogInit(int item, double v) { init_[item] = v; }
  void LogInitAdd(int item, double v) { init_[item] += v; }
  void LogStep(uint64_t key, int item, double v);
  void LogStepAdd(uint64_t key, int item, double v);
  void LogEpochAdd(uint64_t key, int item, double v);
  double GetInit(int item) const { return init_[item]; }
  double GetStep(uint64_t key, int item) const;
  double GetEpoch(uint64_t epoch, int item) const;
  void Trace(uint64_t key, int item, uint64_t ts, bool begin);
  void DumpTrace();
  void ReportStep(uint64_t epoch, uint64_t step);
  void ReportEpoch(uint64_t epoch);
  static constexpr int kMaxInit = 64, kMaxStep = 96, kMaxEpoch = 32;
  size_t num_step_ = 1, num_epoch_ = 1;

 private:
  double init_[kMaxInit] = {0};
  std::vector<double> step_;  // [key][item]
  std::vector<double> epoch_; // [epoch][item]
  struct TraceRec { uint64_t key; int item; uint64_t begin, end; };
  std::vector<TraceRec> trace_;
  std::mutex mu_;
};

inline size_t CountsBytes(size_t L) { return GGMS_COUNTS_WORDS(L) * sizeof(uint64_t); } // a batch's counts words

// ---- the arrays of one sampled batch on one device ------------------------------
struct BatchArrays {
  std::vector<uint32_t *> row, col, data; // per layer; data: random walk only (else null)
  uint32_t *input_nodes = nullptr, *output_nodes = nullptr;
  uint64_t *counts_dev = nullptr; // GGMS_COUNTS_WORDS(L) words (include/ggms.h, "Batch counts words")
  // hipMalloc on the current device at the batch bounds (Engine::ComputeBounds); counts_dev starts zeroed
  void Alloc(const std::vector<size_t> &max_edges, size_t max_unique, size_t max_seeds, bool with_data);
  ggms_queue_batch_t View() const; // (arch5: the batch as the queue kernels take it)
};

// ---- one mini-batch in flight (Task / TrainGraph, common.h:246-283) -------------
struct Batch {
  uint64_t key = 0;
  int slot = -1;
  std::atomic<int> refs{0};
  bool in_use = false;
  bool host = false; // arch0 with a host trainer: the buffers below are host memory, complete when enqueued
  // device buffers, allocated once at their upper bounds: the batch as handed out, on the trainer GPU ...
  BatchArrays trainer;
  // ... and as the sampler writes it.  arch3: its own copies on the SAMPLER GPU, which ggms_batch_handoff copies into
  // `trainer` (handoff_timer rides on that launch).  Every other deployment samples straight into `trainer`: these
  // are the same pointers.
  BatchArrays sampler;
  void *feat = nullptr;
  int64_t *label = nullptr;
  // pinned host copy (hipHostMalloc) of trainer.counts_dev, valid after Finish()
  uint64_t *counts = nullptr;
  size_t num_seeds = 0, num_input = 0;
  // task = link_prediction: the batch's positive edge ids (what the shuffler hands out), and the local id of every
  // entry of the seed list -- the pair ids -- copied out of the sampling workspace before the next batch reuses it
  uint32_t *edge_ids = nullptr, *seed_ids = nullptr;
  size_t num_pos = 0;
  // exclude_seed_edges: the edges ggms_drop_pair_edges took out of each layer -- device words (zeroed per batch) and
  // their pinned host copy, valid with the counts.  Null without the key: the batch then carries no extra packet.
  uint64_t *excluded_dev = nullptr, *excluded = nullptr;
  // edge_ids / edge_feat: per layer, the CSR positions of the layer's edges (max_edges words) and the edge table's rows
  // under them.  Empty without the keys.
  std::vector<uint32_t *> eid;
  std::vector<void *> efeat;
  // khop_temporal: the seed list's times (ggms_link_seed_times; the first num_pos are the positives'), the final cut of
  // every input node, and per layer edge_time[eid].  Null / empty with every other sampler.
  uint32_t *seed_time = nullptr, *node_cut = nullptr;
  std::vector<uint32_t *> etime;
  // khop_typed: per layer the sampled edges' types, written by the sampler beside eid.  Empty with every other sampler.
  std::vector<uint8_t *> etype;
  // induced_subgraph: the induced COO and its edges' CSR positions (induced_max_edges words each), with edge_feat the edge
  // table's rows under them; three device words -- ggms_induced_edges' two counts [M, list entries walked] and
  // min(M, induced_max_edges), the gather's row count -- and the pinned host copy of the first two, valid with the
  // counts.  Null without the key.
  uint32_t *ind_row = nullptr, *ind_col = nullptr, *ind_eid = nullptr;
  void *ind_efeat = nullptr;
  uint64_t *ind_counts_dev = nullptr, *ind_counts = nullptr;
  // hetero_batch: per input node its type, its rank inside the type and its slot in the grouped list, the grouped list
  // itself (max_unique entries each); per layer the edges grouped by relation (row / col as ranks inside their types, the
  // CSR positions; the layer's edge capacity each); the small words [base: T + 1 | cuts: (L + 1) x T | offsets: L x (R + 1)]
  // on the device and their pinned host copy, valid with the counts.  Null / empty without the key.
  uint8_t *het_ntype = nullptr;
  uint32_t *het_local = nullptr, *het_slot = nullptr, *het_typed = nullptr;
  std::vector<uint32_t *> het_row, het_col, het_eid;
  uint32_t *het_words_dev = nullptr, *het_words = nullptr;
  // typed_feat: the T + 1 byte offsets of the types' blocks in `feat`, as ggms_gather_typed wrote them, and their pinned
  // host copy, valid with the counts.  Null without the key.
  uint64_t *het_off_dev = nullptr, *het_off = nullptr;
  uint64_t num_miss = 0;
  hipEvent_t ev_seeds = nullptr, ev_start = nullptr, ev_sampled = nullptr, ev_xstart = nullptr, ev_done = nullptr;
  // arch6 with `gpu_extract` off: the host-staged miss path (dist_loops.cc:1015-1207)
  uint32_t *miss_src = nullptr, *miss_dst = nullptr, *hit_src = nullptr, *hit_dst = nullptr;
  void *idx_ws = nullptr, *miss_rows_dev = nullptr;
  void *miss_rows_host = nullptr;   // hipHostMalloc (pinned): CPU-gathered miss rows, copied down chunk by chunk
  uint32_t *miss_ids_host = nullptr; // hipHostMalloc
  hipEvent_t ev_ids = nullptr;       // the miss ids have reached the host
  hipEvent_t ev_label = nullptr;     // the labels of the batch are gathered
  // the feature gather's own start / end timestamps, riding on its dispatch packet (include/ggms.h, launch timer);
  // lean: this batch's extract stream carried the gather and nothing else (EnqueueOne)
  ggms_launch_timer_t *gather_timer = nullptr;
  bool lean = false;
  ggms_launch_timer_t *handoff_timer = nullptr; // arch3: rides on the hand-off; arch5: on the unpack
  // arch4: around the expansion on the sampling stream (recorded by ggms_sample_batch_prefetch); the trainer's stream
  // starts the gather at ev_final, the COO hand-off waits for ev_sampled
  hipEvent_t ev_expand = nullptr, ev_final = nullptr;
  Batch *dyn_hold = nullptr; // dynamic_cache: the previous batch, whose rows this batch's gather reads
  // arch5 trainer: the queue ticket whose slot this batch came from, and the host's wait for that message
  uint64_t queue_pos = 0;
  double recv_s = 0;
};

class Engine {
 public:
  static Engine &Get();
  Engine();
  ~Engine();
  RunConfig cfg;
  Dataset ds;
  Profiler prof;

  void Configure(const std::unordered_map<std::string, std::string> &kv);
  void DataInit();                                    // load dataset (host only; fork-safe)
  void SampleInit(int worker_id, const std::string &ctx); // device state for sampling
  void TrainInit(int worker_id, const std::string &ctx);  // feature cache / extract state
  void Init();                                        // arch1: all three
  void Start();
  void Shutdown();
  void RunSampleOnce(bool background = false);
  bool EnqueueOne(bool background);
  uint64_t GetNextBatch();
  void ExtractStart(int count);
  Batch *Current(uint64_t key);
  void Retain(uint64_t key);
  void Release(uint64_t key);
  // feat_learnable: the current batch's gradient, (num_input, feat_dim) F32 produced on `caller`, moves the table rows the
  // batch gathered; the live table and (Adagrad) its accumulator as they lie on the trainer GPU
  void UpdateGraphFeat(uint64_t key, const void *grad, size_t num_rows, size_t dim, hipStream_t caller);
  void *StoreFeat(const char *who) const;
  void *StoreState(const char *who) const;

  size_t NumEpoch() const { return cfg.num_epoch; }
  size_t NumStep() const { return num_global_step_; }
  size_t NumLocalStep() const { return num_local_step_; }
  uint64_t BatchKey(uint64_t epoch, uint64_t step) const { return epoch * num_global_step_ + step; }
  // arch3 / arch4: one GPU samples, another trains (arch4 adds the early prefetch and dynamic_cache)
  bool Dedicated() const { return cfg.arch == kArch3 || cfg.arch == kArch4; }
  int trainer_device() const { return Dedicated() ? trainer_device_ : device_; }
  bool IsArch5Sampler() const { return cfg.arch == kArch5 && role_ == kRoleSampler; }
  // arch3 / arch5: the batch is sampled elsewhere (sampler GPU / process) and handed to the trainer GPU's extract stream
  bool BatchSampledElsewhere() const { return Dedicated() || cfg.arch == kArch5; }
  // dtype of a batch's feature buffer: the configured feat_out_dtype, else the table's
  int batch_feat_dtype() const { return cfg.feat_out_dtype < 0 ? ds.feat_dtype : cfg.feat_out_dtype; }
  // bytes of one row of a batch's feature buffer: always dim x batch dtype, whatever the table stores per row
  size_t batch_feat_row_bytes() const { return ds.feat_dim * ggms_dtype_bytes(batch_feat_dtype()); }
  // typed_feat: the dtype type t's rows are delivered in (feat_out_dtype, else the table's own)
  int typed_feat_dtype(size_t t) const { return cfg.feat_out_dtype < 0 ? ds.node_feat[t].dtype : cfg.feat_out_dtype; }
  int batch_device_type() const { return (cfg.arch == kArch0 && cfg.trainer_on_host) ? 0 : 2; } // DeviceType, common.h:48
  void Barrier(const char *what = "step");
  void *OpenPeer(const hipIpcMemHandle_t &handle, uint32_t peer, size_t bytes, const char *what);

 private:
  // dataset
  void LoadDataset();
  HostArray MapFile(const std::string &name, size_t bytes, bool to_shared_anon);
  // shuffler (cuda/cuda_shuffler.cc, dist/dist_shuffler_aligned.cc)
  void ShufflerInit();
  // what the shuffler permutes: the train node set, or the train edge set of a link_prediction run
  const uint32_t *SeedSet() const { return cfg.link_prediction ? ds.train_edges : (const uint32_t *)ds.train_set.ptr; }
  size_t SeedSetSize() const { return cfg.link_prediction ? ds.num_train_edge : ds.num_train; }
  uint64_t link_forced_ = 0; // link_prediction: forced negatives of the batches handed out so far in this epoch
  bool ShufflerNext(Batch *b, hipStream_t copy_stream); // false at end of training
  void Reshuffle();
  // GGMS
  void DetectTopo(); // PartitionSolver::DetectTopo (dist_graph.cu:684-726): P2P reachability + link rates, probed in a forked child
  ggms_topology_t topo_{};
  bool topo_valid_ = false;
  void UploadGraph();
  void AttachListHeads(); // config key inline_heads
  void Presample();
  void QuantizeStore(); // config key feat_store_dtype: ds.feat re-encoded by ggms_quantize_rows, before BuildCache
  void BuildCache();
  Batch *AcquireSlot(bool background);
  // `gpu_extract` off (SGNN mode of arch6): miss ids -> host, CPU gather into pinned memory, async H2D, combine
  // (a partial cache: its table exists; no cache at all: every row is a miss.  A FULL cache has no table and no misses.)
  bool StagedHostTier() const { return cfg.arch == kArch6 && !cfg.gpu_extract && (cache_table_ != nullptr || !cfg.UseGPUCache()); }
  void StagedExtract(Batch *b, hipStream_t ss, hipStream_t xs);
  void HostGatherRows(char *rows, const uint32_t *ids, size_t first, size_t count); // ExtractMissData on the host team
  std::unique_ptr<class Team> host_team_;
  size_t staged_batches_ = 0;
  void SanityCheckBatch(const uint32_t *seeds, size_t n); // SAMGRAPH_SANITY_CHECK
  std::vector<bool> sanity_seen_;
  uint32_t *node_access_dev_ = nullptr; // SAMGRAPH_LOG_NODE_ACCESS[_SIMPLE]: visits per node (input nodes of every batch)
 public:
  void ReportNodeAccess();
 private:
  // arch0 (cpu_engine.cc): sampler + extractor on the host cores
  struct CpuPath;
  std::unique_ptr<CpuPath> cpu_;
  void CpuInit();
  bool CpuEnqueueOne(bool background);
  void CpuShutdown();
  void Finish(Batch *b, Batch *prev);
  void CheckBatchStatus(uint64_t status, uint64_t key) const; // the device status word of a completed batch
  void EnablePeerAccess(); // arch3: the trainer GPU reads the sampler GPU's batch buffers in place
  enum HandoffPart { kHandoffAll, kHandoffIds, kHandoffGraph }; // arch4: ids at "input set final", the COO at the end
  void Handoff(Batch *b, hipStream_t xs, HandoffPart part = kHandoffAll);
  void EnqueueGather(Batch *b, hipStream_t ss); // label + feature gather of a sampled (arch3: handed-off) batch

  // arch5 (dist/dist_engine.cc, dist_loops_arch5.cc): a process is a sampler or a trainer.  The batch queue is one
  // anonymous MAP_SHARED mapping made by DataInit (before the fork): a control page, then queue_depth_ slots of
  // qlay_.slot_bytes each (include/ggms.h, ggms_queue_header_t).  Tickets: the k-th message goes to slot k % depth;
  // a slot's `seq` word is k when a producer may fill it for ticket k, k + 1 once it holds ticket k's batch, and
  // k + depth when the consumer has freed it (a bounded MPMC ring with one sequence word per slot).
  enum Role { kRoleNone, kRoleSampler, kRoleTrainer };
  Role role_ = kRoleNone;
  struct QueueCtl;
  QueueCtl *queue_ = nullptr;
  char *queue_slots_ = nullptr;     // host address of slot 0
  char *queue_slots_dev_ = nullptr; // ... the same memory as this process's device sees it (hipHostRegister, Mapped)
  size_t queue_depth_ = 0;
  ggms_queue_layout_t qlay_{};
  std::unique_ptr<Batch> sbatch_; // the sampler's own batch buffers (it packs each batch before it samples the next)
  void ComputeBounds();
  void QueueInit();
  void QueueMap();
  ggms_queue_header_t *QueueHeader(uint64_t pos) const;
  bool QueueWait(const uint64_t *word, uint64_t want, const char *what, bool stoppable);
  void PublishRanking();   // pre_sample: sampler 0's ranking is written ...
  void WaitRankingReady(); // ... and everybody else waits for it
  void Arch5TrainerInit(int worker_id, const std::string &ctx);
  void SendOne();                                // a sampler's sample_once
  bool Receive(Batch *b);                        // a trainer takes the next message (host side)
  void Unpack(Batch *b, hipStream_t xs);         // ... copies it out of its slot and frees the slot

  bool data_ready_ = false, sample_ready_ = false, train_ready_ = false, shutdown_ = false;
  int worker_id_ = 0, device_ = 0;
  int trainer_device_ = 0; // arch3: the trainer GPU (label table, feature cache, the batch as handed out); else device_
  hipStream_t stream_ = nullptr;         // shuffle + sampling (latency-bound)
  hipStream_t stream_extract_ = nullptr; // feature gather (HBM-bound): overlaps the next batch's sampling
                                         // (arch3: on the trainer GPU, with the hand-off and the label gather)
  // a second one: consecutive lean batches' gathers alternate and may overlap -- no wait packet between two gathers, and
  // one gather's head fills the other's tail (default workload -5 %, profiles/r05_ab_extract_streams.txt)
  hipStream_t stream_extract2_ = nullptr;
  // device graph
  uint32_t *d_indptr_ = nullptr, *d_indices_ = nullptr;
  void *d_heads_ = nullptr; // inline list heads (config key inline_heads), attached to graph_
  std::vector<void *> part_indptr_, part_indices_; // P+1 entries (slot P = host CSR)
  ggms_graph_t graph_{};
  // sampler state
  ggms_hashtable_t ht_{};
  ggms_sample_extra_t extra_{};
  void *d_prob_ = nullptr, *d_alias_ = nullptr;
  void *states_ = nullptr;
  size_t num_states_ = 0;
  void *ws_ = nullptr;
  size_t ws_bytes_ = 0;
  // sampling pipelines 1..K-1 (pipeline 0 is {stream_, ht_, ws_}); the RNG pool is consumed in batch order
  struct Pipe {
    hipStream_t stream = nullptr;
    ggms_hashtable_t ht{};
    void *ws = nullptr;
    hipEvent_t rng_done = nullptr;
    void *drop_ws = nullptr; // exclude_seed_edges: ggms_drop_pair_edges' workspace, a piece of its own (the seed ids it
                             // reads lie in `ws`)
    void *eid_ws = nullptr;  // edge_ids: ggms_edge_positions' workspace
    uint64_t *cut_table = nullptr; // khop_temporal: the pipeline's cut table (8 B x num_node, zeroed once) and the stamp of
    uint32_t stamp = 0;            // its last batch
    uint32_t *induced_map = nullptr; // induced_subgraph: the pipeline's membership map (4 B x num_node, all EMPTY between
    void *induced_ws = nullptr;      // batches) and ggms_induced_edges' workspace
    void *hetero_ws = nullptr;       // hetero_batch: the one workspace of ggms_hetero_nodes and ggms_hetero_edges
  };
  size_t hetero_ws_bytes_ = 0;
  uint8_t *d_node_type_ = nullptr; // hetero_batch: the node types in HBM
  // typed_feat: the tables in HBM (null for a type without one), the rank table (null: ranks are node - first_node), the
  // leaf's table array and the bytes of a batch's feature buffer
  std::vector<void *> d_node_feat_;
  uint32_t *d_node_rank_ = nullptr;
  std::vector<ggms_typed_table_t> typed_tables_;
  size_t typed_feat_bytes_ = 0;
  void LoadTypedFeat(const std::unordered_map<std::string, size_t> &meta,
                     const std::unordered_map<std::string, std::string> &meta_text);
 public:
  // hetero_batch: where the three groups of Batch::het_words start
  size_t HetBaseAt() const { return 0; }
  size_t HetCutsAt() const { return ds.num_node_type + 1; }
  size_t HetOffsetsAt() const { return HetCutsAt() + (cfg.fanout.size() + 1) * ds.num_node_type; }
  size_t HetWords() const { return HetOffsetsAt() + cfg.fanout.size() * (cfg.num_edge_type + 1); }
 private:
  size_t induced_ws_bytes_ = 0;
  size_t induced_max_edges_ = 0; // induced_subgraph: the capacity of a batch's induced arrays (ResolveInducedCapacity)
  void ResolveInducedCapacity();
  size_t drop_ws_bytes_ = 0;
  size_t eid_ws_bytes_ = 0;    // edge_ids: ggms_edge_positions' workspace (Pipe::eid_ws)
  void *d_edge_feat_ = nullptr; // edge_feat: the edge table in HBM
  uint32_t *d_edge_time_ = nullptr; // khop_temporal: the edge times in HBM
  uint8_t *d_edge_type_ = nullptr;  // khop_typed: the edge types in HBM
  uint64_t link_excluded_ = 0; // exclude_seed_edges: edges dropped from the batches handed out so far in this epoch
  std::vector<Pipe> pipes_;
  size_t enq_count_ = 0;
  hipEvent_t last_rng_done_ = nullptr;
  void SampleInto(Batch *b, Pipe &P); // sample b's seeds into b->sampler on P's stream, then record b->ev_sampled
  size_t max_seeds_ = 0, max_unique_ = 0; // batch bounds (ComputeBounds)
  size_t max_prefetch_edges_ = 0;         // arch4: the expansion's capacity (max_unique_ is then the superset's)
  // dynamic_cache: node -> (seq << 32) | slot of its last batch, on the trainer GPU; the batch the next gather reads
  uint64_t *dyn_stamps_ = nullptr;
  uint32_t dyn_seq_ = 0;
  Batch *dyn_prev_ = nullptr;
  std::vector<size_t> max_input_, max_edges_;
  // shuffler
  std::vector<uint32_t> shuf_host_;
  uint32_t *shuf_dev_ = nullptr;
  size_t num_data_ = 0, num_local_data_ = 0, num_local_step_ = 0, num_global_step_ = 0;
  size_t global_step_offset_ = 0, global_data_offset_ = 0;
  size_t cur_epoch_ = 0, cur_step_ = 0;
  bool shuf_initialized_ = false;
  // ggms_sample_extra_t.seeds_distinct: the train set holds no node twice (checked once), so a batch's seeds are
  // distinct unless both copies of a node that pads the aligned epoch (dist_shuffler_aligned.cc:52-54) fall into it
  bool train_distinct_ = false;
  std::vector<std::pair<size_t, size_t>> pad_pairs_; // this worker's slice, this epoch: local positions of such copies
  bool BatchSeedsDistinct(size_t offset, size_t size) const;
  // features
  uint32_t *cache_table_ = nullptr;            // id -> slot (GPUCacheManager::_sampler_gpu_hashtable)
  std::vector<void *> cache_parts_;            // shard base pointers (local or IPC-mapped)
  uint32_t num_cache_part_ = 0;
  size_t num_cached_nodes_ = 0;
  size_t num_replica_ = 0;                     // hybrid store: slots [0, num_replica_) live in d_replica_ on every GPU
  void *d_replica_ = nullptr;
  void *d_feat_ = nullptr;                     // full feature table on the device (arch1) ...
  void *d_feat_state_ = nullptr;               // feat_learnable = adagrad: the accumulator, shaped like d_feat_
  hipEvent_t ev_grad_ = nullptr, ev_updated_ = nullptr; // feat_learnable: caller's stream -> extract stream and back
  const void *feat_src_ = nullptr;             // ... or device-mapped host memory (gpu_extract / miss tier)
  const void *label_src_ = nullptr;
  // batches
  std::vector<std::unique_ptr<Batch>> slots_;
  std::deque<Batch *> pool_;
  std::mutex pool_mu_;
  std::condition_variable pool_cv_;
  Batch *current_ = nullptr;
  std::thread bg_;
  size_t fg_calls_ = 0, fg_enqueued_ = 0; // foreground sample_once() calls / batches enqueued for them
  std::atomic<bool> bg_stop_{false};
  std::atomic<bool> bg_running_{false};
  // shared (arch6): control block inherited through fork
  struct Shared;
  Shared *shared_ = nullptr;
};

} // namespace sam
