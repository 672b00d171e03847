// engine.cc -- host orchestration (see engine.h).  Citations are relative to
// /root/reference/samgraph/common/.
#include "engine.h"
#include "team.h"
#include "../labor_hash.h"
#include "../row_formats.h"

#include <fcntl.h>
#include <pthread.h>
#include <sys/mman.h>
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <thread>

namespace sam {

void fatal(const char *file, int line, const std::string &msg) {
  std::fprintf(stderr, "[samgraph-amd FATAL] %s:%d: %s\n", file, line, msg.c_str());
  std::fflush(stderr);
  std::abort(); // logging.cc:69-73: failed CHECK aborts the process
}

void log_info(const std::string &msg) {
  static const bool on = [] { const char *e = getenv("SAMGRAPH_LOG_LEVEL"); return e && (std::string(e) == "info" || std::string(e) == "debug"); }();
  if (on) std::fprintf(stderr, "[samgraph-amd] %s\n", msg.c_str());
}

// process-shared control block for arch6 workers (dist_graph.cu:566-636: anonymous MAP_SHARED mmap +
// PTHREAD_PROCESS_SHARED barrier, inherited through fork)
struct Engine::Shared {
  // worker barrier with a deadline (pthread_barrier_wait has none): arrivals of the current generation + the
  // generation counter; zero-initialised by the anonymous mapping, lock-free atomics are valid across processes
  std::atomic<uint32_t> arrived, generation;
  int num_worker;
  static constexpr int kMaxWorker = 16;
  hipIpcMemHandle_t graph_indptr[kMaxWorker], graph_indices[kMaxWorker], feat_part[kMaxWorker];
  size_t indptr_words[kMaxWorker], indices_words[kMaxWorker], feat_rows[kMaxWorker];
};

Engine &Engine::Get() {
  static Engine e;
  return e;
}

int parse_device(const std::string &ctx) {
  // "cuda:3" / "cpu:0" (Context(std::string), common.cc)
  auto p = ctx.find(':');
  int id = p == std::string::npos ? 0 : std::atoi(ctx.c_str() + p + 1);
  const char *force = getenv("SAMGRAPH_FORCE_DEVICE"); // test hook: all workers on one physical GPU
  if (force) id = std::atoi(force);
  return id;
}

static std::string ctx_id_as_written(const std::string &ctx) { // the device id of "cuda:N", SAMGRAPH_FORCE_DEVICE not applied
  auto p = ctx.find(':');
  return std::to_string(p == std::string::npos ? 0 : std::atoi(ctx.c_str() + p + 1));
}

// ------------------------------------------------------------------ configuration
// arch3 / arch5 build no GGMS shards: the keys that ask for them are refused, naming the deployment
static void refuse_arch6_keys(std::unordered_map<std::string, std::string> &kv, const std::string &arch) {
  const bool dist_graph = kv.count("use_dist_graph") && std::stod(kv["use_dist_graph"]) > 0.0;
  for (const char *k : {"part_cache", "gpu_extract"})
    if (kv.count(k) && kv[k] == "True") fatal(__FILE__, __LINE__, arch + ": " + k + " is an arch6 key (GGMS shards across workers)");
  if (dist_graph) fatal(__FILE__, __LINE__, arch + ": use_dist_graph is an arch6 key (GGMS shards across workers)");
}

// a row-scaled table (FEAT_DATA_TYPE Q8ROW on disk, or made by feat_store_dtype = Q8ROW) without feat_out_dtype
static const char *const kQ8RowNeedsOutDtype =
    "FEAT_DATA_TYPE Q8ROW needs the config key feat_out_dtype (f32 | f16 | bf16): a row of 8-bit codes with its scale and "
    "bias is decoded by the feature gather, there is no element type to deliver it in as it is";
// the dtype names of meta.txt's FEAT_DATA_TYPE; feat_store_dtype takes those of them the quantiser writes
static const std::map<std::string, int> kFeatDtypeNames = {{"F32", GGMS_F32}, {"F64", GGMS_F64}, {"F16", GGMS_F16},
                                                           {"U8", GGMS_U8},   {"I32", GGMS_I32}, {"I8", GGMS_I8},
                                                           {"I64", GGMS_I64}, {"BF16", GGMS_BF16},
                                                           {"F8E4M3", GGMS_F8E4M3}, {"F8E5M2", GGMS_F8E5M2},
                                                           {"Q8ROW", GGMS_Q8ROW}};

void Engine::Configure(const std::unordered_map<std::string, std::string> &kv_in) {
  auto kv = kv_in;
  SAM_CHECK(!cfg.configured, "samgraph_config called twice");
  // required keys, operation.cc:68-81
  for (const char *k : {"dataset_path", "_arch", "_sample_type", "batch_size", "num_epoch", "_cache_policy",
                        "cache_percentage", "max_sampling_jobs", "max_copying_jobs", "omp_thread_num", "num_layer",
                        "num_hidden", "lr", "dropout"})
    SAM_CHECK(kv.count(k), std::string("missing config key ") + k);
  cfg.raw = kv;
  cfg.dataset_path = kv["dataset_path"];
  cfg.arch = std::stoi(kv["_arch"]);
  cfg.sample_type = std::stoi(kv["_sample_type"]);
  cfg.batch_size = std::stoull(kv["batch_size"]);
  cfg.num_epoch = std::stoull(kv["num_epoch"]);
  cfg.cache_policy = std::stoi(kv["_cache_policy"]);
  cfg.cache_percentage = std::stod(kv["cache_percentage"]);
  cfg.num_layer = std::stoull(kv["num_layer"]);
  SAM_CHECK(cfg.batch_size > 0 && cfg.num_layer >= 1 && cfg.num_layer <= 16, "batch_size >= 1 and 1 <= num_layer <= 16");
  // every deployment: arch0's sampler / extractor team and arch6's host-staged miss path (gpu_extract off) use it
  cfg.omp_thread_num = std::max<size_t>(1, std::stoull(kv["omp_thread_num"]));
  switch (cfg.arch) { // operation.cc:101-148
    case kArch1:
      SAM_CHECK(kv.count("sampler_ctx") && kv.count("trainer_ctx"), "arch1 needs sampler_ctx/trainer_ctx");
      cfg.sampler_device = parse_device(kv["sampler_ctx"]);
      cfg.trainer_device = parse_device(kv["trainer_ctx"]);
      cfg.num_worker = 1;
      break;
    case kArch0: // CPU sampler + extractor, trainer on a GPU or (plumbing runs) on the host
      SAM_CHECK(kv.count("sampler_ctx") && kv.count("trainer_ctx"), "arch0 needs sampler_ctx/trainer_ctx");
      cfg.trainer_on_host = kv["trainer_ctx"].rfind("cpu", 0) == 0;
      cfg.trainer_device = parse_device(kv["trainer_ctx"]);
      cfg.num_worker = 1;
      break;
    case kArch3:   // GPUEngine::ArchCheck (cuda/cuda_engine.cc:410-435): one GPU samples, a different GPU trains
    case kArch4: { // the same, + early prefetch and dynamic_cache (cuda/cuda_loops_arch4.cc)
      const std::string a = cfg.arch == kArch4 ? "arch4" : "arch3";
      SAM_CHECK(kv.count("sampler_ctx") && kv.count("trainer_ctx"), a + " needs sampler_ctx/trainer_ctx");
      const std::string sc = kv["sampler_ctx"], tc = kv["trainer_ctx"];
      if (sc.rfind("cuda", 0) != 0 || tc.rfind("cuda", 0) != 0)
        fatal(__FILE__, __LINE__, a + ": sampler_ctx and trainer_ctx must both be GPU contexts (cuda:N), got " + sc +
                                      " and " + tc);
      if (ctx_id_as_written(sc) == ctx_id_as_written(tc))
        fatal(__FILE__, __LINE__, a + ": sampler_ctx and trainer_ctx are the same GPU (" + sc + "): " + a + " samples on one "
                                      "GPU and trains on another; one GPU for both is arch1");
      const bool log_access = getenv("SAMGRAPH_LOG_NODE_ACCESS") || getenv("SAMGRAPH_LOG_NODE_ACCESS_SIMPLE");
      if (cfg.cache_percentage > 0 && log_access)
        fatal(__FILE__, __LINE__, a + ": a GPU cache (cache_percentage > 0) cannot be combined with node access logging "
                                  "(SAMGRAPH_LOG_NODE_ACCESS*)");
      refuse_arch6_keys(kv, a);
      cfg.sampler_device = parse_device(sc);
      cfg.trainer_device = parse_device(tc);
      cfg.num_worker = 1;
      break;
    }
    case kArch5: { // DistEngine (dist/dist_engine.cc, operation.cc:112-121): S sampler processes, T trainer processes
      SAM_CHECK(kv.count("num_sample_worker") && kv.count("num_train_worker"), "arch5 needs num_sample_worker/num_train_worker");
      cfg.num_sample_worker = std::stoull(kv["num_sample_worker"]);
      cfg.num_train_worker = std::stoull(kv["num_train_worker"]);
      if (cfg.num_sample_worker < 1 || cfg.num_train_worker < 1)
        fatal(__FILE__, __LINE__, "arch5: num_sample_worker and num_train_worker must both be >= 1, got " +
                                      kv["num_sample_worker"] + " and " + kv["num_train_worker"]);
      if (cfg.num_sample_worker + cfg.num_train_worker > 16)
        fatal(__FILE__, __LINE__, "arch5: num_sample_worker + num_train_worker = " +
                                      std::to_string(cfg.num_sample_worker + cfg.num_train_worker) + ": at most 16 workers");
      if (kv.count("have_switcher") && kv["have_switcher"] != "0" && kv["have_switcher"] != "False")
        fatal(__FILE__, __LINE__, "arch5: have_switcher = " + kv["have_switcher"] + ": the switcher is not built "
                                  "(samgraph_switch_init); set have_switcher = 0");
      refuse_arch6_keys(kv, "arch5");
      if (kv.count("unified_memory") && (kv["unified_memory"] == "True" || kv["unified_memory"] == "1"))
        fatal(__FILE__, __LINE__, "arch5: unified_memory is not built (arch9, unified-memory sampling)");
      // the queue: 2 slots per trainer (one being unpacked, one filled meanwhile), at least 4
      cfg.queue_depth = std::max<size_t>(4, 2 * cfg.num_train_worker);
      if (kv.count("queue_depth")) cfg.queue_depth = std::stoull(kv["queue_depth"]);
      if (cfg.queue_depth < 1 || cfg.queue_depth > 1024)
        fatal(__FILE__, __LINE__, "arch5: queue_depth = " + kv["queue_depth"] + ": 1 .. 1024 slots");
      if (kv.count("queue_timeout_s")) cfg.queue_timeout_s = std::stod(kv["queue_timeout_s"]);
      if (!(cfg.queue_timeout_s > 0))
        fatal(__FILE__, __LINE__, "arch5: queue_timeout_s = " + kv["queue_timeout_s"] + ": a positive number of seconds");
      cfg.num_worker = cfg.num_sample_worker + cfg.num_train_worker;
      break;
    }
    case kArch6:
      SAM_CHECK(kv.count("num_worker"), "arch6 needs num_worker");
      cfg.num_worker = std::stoull(kv["num_worker"]);
      SAM_CHECK(cfg.num_worker >= 1, "num_worker >= 1");
      break;
    default:
      fatal(__FILE__, __LINE__, "only arch0 (CPU), arch1 (standalone), arch3 (dedicated), arch4 (dedicated with prefetch), "
                                "arch5 (factored) and arch6 (SGNN/XGNN) are built; see DESIGN.md");
  }
  if (cfg.sample_type != GGMS_RANDOM_WALK) { // operation.cc:150-163
    SAM_CHECK(kv.count("num_fanout") && kv.count("fanout"), "khop sampling needs num_fanout/fanout");
    size_t nf = std::stoull(kv["num_fanout"]);
    std::stringstream ss(kv["fanout"]);
    for (size_t i = 0; i < nf; ++i) {
      size_t f = 0;
      ss >> f;
      SAM_CHECK(f > 0, "fanout: num_fanout positive integers expected");
      cfg.fanout.push_back(f);
    }
  } else { // :164-175
    cfg.random_walk_length = std::stoull(kv["random_walk_length"]);
    cfg.random_walk_restart_prob = std::stod(kv["random_walk_restart_prob"]);
    cfg.num_random_walk = std::stoull(kv["num_random_walk"]);
    cfg.num_neighbor = std::stoull(kv["num_neighbor"]);
    SAM_CHECK(cfg.random_walk_length > 0 && cfg.num_random_walk > 0 && cfg.num_neighbor > 0,
              "random walk needs random_walk_length, num_random_walk and num_neighbor >= 1");
    cfg.fanout.assign(cfg.num_layer, cfg.num_neighbor);
  }
  if (kv.count("use_dist_graph")) { // :191-203
    cfg.dist_graph_percentage = std::stod(kv["use_dist_graph"]);
    cfg.use_dist_graph = cfg.dist_graph_percentage > 0.0;
  }
  if (kv.count("part_cache") && kv["part_cache"] == "True") { // :205-211
    SAM_CHECK(cfg.arch == kArch6, "partition cache can only be used in arch6");
    cfg.part_cache = true;
  }
  if (kv.count("gpu_extract") && kv["gpu_extract"] == "True") cfg.gpu_extract = (cfg.arch == kArch6); // :229-235
  // extension: the hottest fraction of the CACHED slots is kept on every GPU instead of being sharded (what the
  // reference's PartitionSolver buys with replica placement on NVLink, dist_graph.cu:40-222); 0 = pure modulo shards
  if (kv.count("replicate_percentage")) cfg.replicate_percentage = std::stod(kv["replicate_percentage"]);
  if (kv.count("presample_epoch")) cfg.presample_epoch = std::stoull(kv["presample_epoch"]); // operation.cc:184-189
  if (kv.count("seed")) { cfg.has_seed = true; cfg.seed = std::stoull(kv["seed"]); }
  if (kv.count("hash_table")) cfg.direct_table = kv["hash_table"] != "hashed";
  if (kv.count("lookahead")) cfg.lookahead = std::stoull(kv["lookahead"]);
  if (kv.count("staged_serial_epochs")) cfg.staged_serial_epochs = std::stoull(kv["staged_serial_epochs"]);
  if (kv.count("staged_serial_steps")) cfg.staged_serial_steps = std::stoull(kv["staged_serial_steps"]);
  if (kv.count("extract_streams")) cfg.extract_streams = std::max<size_t>(1, std::min<size_t>(2, std::stoull(kv["extract_streams"])));
  if (const char *e = getenv("SAMGRAPH_EXTRACT_STREAMS")) cfg.extract_streams = (e[0] == '1') ? 1 : 2; // A/B hook
  if (kv.count("pipelines")) cfg.pipelines = std::max<size_t>(1, std::min<size_t>(4, std::stoull(kv["pipelines"])));
  if (cfg.lookahead + 1 < cfg.pipelines) cfg.pipelines = cfg.lookahead + 1; // nothing to overlap without batches ahead
  if (cfg.arch == kArch5) { // a trainer's sample_once() handles exactly one message; a sampler packs each batch it samples
    cfg.lookahead = 0;
    cfg.pipelines = 1;
  }
  SAM_CHECK(cfg.sample_type >= GGMS_KHOP0 && cfg.sample_type <= GGMS_KHOP_TYPED, "unknown sample type");
  if (kv.count("hetero_batch")) { // extension: the batch's heterogeneous view (node types, per-relation blocks)
    if (kv["hetero_batch"] != "on" && kv["hetero_batch"] != "off")
      fatal(__FILE__, __LINE__, "hetero_batch = " + kv["hetero_batch"] + ": on or off (the default)");
    cfg.hetero = kv["hetero_batch"] == "on";
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    if (cfg.hetero && cfg.arch != kArch1)
      fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": hetero_batch is not built: the typed view is computed "
                                "behind arch1's sampling chain and travels through no hand-off or queue");
  }
  if (cfg.Typed() && cfg.arch != kArch1) {
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": _sample_type 10 (khop_typed) is not built: the edge "
                              "types and the edge positions run in arch1's sampling chain only");
  }
  if (cfg.Temporal() && cfg.arch != kArch1) {
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": _sample_type 9 (khop_temporal) is not built: the seed "
                              "times, the cut table and the edge positions run in arch1's sampling chain only");
  }
  if (cfg.sample_type == GGMS_KHOP_LABOR && cfg.arch == kArch0)
    fatal(__FILE__, __LINE__, "arch0: _sample_type 8 (khop_labor) is not supported: the CPU engine has no sampler for "
                              "it; it samples with khop0 or khop2");
  // khop_labor's batch salts: taken here, once, so that every process forked from this one derives the same salts
  cfg.labor_seed = cfg.has_seed ? cfg.seed : (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
  if (kv.count("feat_out_dtype")) { // extension: deliver the batch's rows in this dtype, converted by the gather itself
    static const std::map<std::string, int> names = {{"f32", GGMS_F32}, {"f16", GGMS_F16}, {"bf16", GGMS_BF16}};
    const std::string v = kv["feat_out_dtype"];
    if (!names.count(v))
      fatal(__FILE__, __LINE__, "feat_out_dtype = " + v + ": the converting gather delivers f32, f16 or bf16");
    cfg.feat_out_dtype = names.at(v);
    // (the table's side of the pair is checked when meta.txt has been read: LoadDataset)
    if (cfg.arch == kArch0)
      fatal(__FILE__, __LINE__, "arch0: feat_out_dtype is not built for the CPU engine: its extractor copies rows, it does "
                                "not convert them");
    if (cfg.arch == kArch6 && !cfg.gpu_extract && cfg.cache_percentage < 1.0)
      fatal(__FILE__, __LINE__, "arch6: feat_out_dtype needs gpu_extract = True or cache_percentage 1.0: the host-staged "
                                "tier's rows land in the batch by hipMemcpyAsync, which does not convert");
  }
  if (kv.count("feat_store_dtype")) { // extension: the F32 / F16 table on disk is encoded into this type on the trainer GPU
    const std::string v = kv["feat_store_dtype"];
    const auto name = kFeatDtypeNames.find(v);
    if (name == kFeatDtypeNames.end() || !ggms::quantiser_writes(name->second))
      fatal(__FILE__, __LINE__, "feat_store_dtype = " + v + ": unknown store type; the GPU quantiser writes F16, BF16, "
                                "F8E4M3, F8E5M2 or Q8ROW");
    cfg.feat_store_dtype = name->second;
    if (cfg.arch == kArch0)
      fatal(__FILE__, __LINE__, "arch0: feat_store_dtype needs a GPU: the table is encoded by a kernel, and the CPU engine "
                                "has no GPU; quantise the dataset offline (datagen.quantize_features)");
    if (cfg.arch == kArch5 || cfg.arch == kArch6)
      fatal(__FILE__, __LINE__, std::string(cfg.arch == kArch5 ? "arch5" : "arch6") + ": feat_store_dtype is not built: the "
                                "process that loads the dataset forks its workers and must not initialise the GPU before it "
                                "forks; quantise the dataset offline (datagen.quantize_features)");
    // the batch dtype rule of a table of that type (the table's side of it is checked in LoadDataset)
    if (cfg.feat_store_dtype == GGMS_Q8ROW && cfg.feat_out_dtype < 0) fatal(__FILE__, __LINE__, kQ8RowNeedsOutDtype);
  }
  if (kv.count("inline_heads")) { // extension: inline list heads for khop3 (include/ggms.h), built at graph load
    const std::string v = kv["inline_heads"];
    if (v != "auto" && v != "0" && v != "1") fatal(__FILE__, __LINE__, "inline_heads = " + v + ": auto (the default), 0 or 1");
    cfg.inline_heads = v == "auto" ? -1 : (v == "1" ? 1 : 0);
    if (cfg.inline_heads == 1 && (cfg.arch != kArch1 || cfg.use_dist_graph || cfg.sample_type == GGMS_KHOP2))
      fatal(__FILE__, __LINE__, "inline_heads = 1: built for arch1 with the whole CSR on the GPU, and not beside khop2, "
                                "which permutes the neighbour lists the table copies");
  }
  if (kv.count("task")) { // extension: what a batch is made of
    const std::string v = kv["task"];
    if (v != "node_classification" && v != "link_prediction")
      fatal(__FILE__, __LINE__, "task = " + v + ": node_classification (the default) or link_prediction");
    cfg.link_prediction = v == "link_prediction";
  }
  if (cfg.link_prediction) {
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    if (cfg.arch != kArch1)
      fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": task = link_prediction is not built: edge seeds, "
                                "negative sampling and the pair ids run in arch1's sampling chain only");
    if (cfg.sample_type == GGMS_RANDOM_WALK)
      fatal(__FILE__, __LINE__, "task = link_prediction with _sample_type 3 (random_walk) is not built: the pair ids are "
                                "the k-hop batch's seed ids");
    if (kv.count("num_negative")) {
      long long k = 0;
      try { k = std::stoll(kv["num_negative"]); } catch (...) { k = 0; }
      if (k < 1 || k > 64)
        fatal(__FILE__, __LINE__, "num_negative = " + kv["num_negative"] + ": 1 .. 64 negatives per positive edge");
      cfg.num_negative = (uint32_t)k;
    }
    if (kv.count("negative_mode")) {
      const std::string v = kv["negative_mode"];
      if (v != "uniform" && v != "exclude")
        fatal(__FILE__, __LINE__, "negative_mode = " + v + ": uniform or exclude (the default)");
      cfg.negative_mode = v == "uniform" ? GGMS_NEG_UNIFORM : GGMS_NEG_EXCLUDE;
    }
    if (kv.count("exclude_seed_edges")) {
      const std::string v = kv["exclude_seed_edges"];
      if (v != "none" && v != "self" && v != "both")
        fatal(__FILE__, __LINE__, "exclude_seed_edges = " + v + ": none (the default), self (the positive edges leave "
                                  "the sampled layers) or both (and their mirrors)");
      cfg.exclude_seed_edges = v == "none" ? 0u : v == "self" ? GGMS_DROP_FORWARD : (GGMS_DROP_FORWARD | GGMS_DROP_REVERSE);
    }
  }
  if (kv.count("feat_learnable")) { // extension: the device table is trainable (samgraph_update_graph_feat)
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    if (cfg.arch != kArch1)
      fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": feat_learnable is not built: only arch1 keeps the "
                                "whole table in one GPU's memory; the cache tiers and shards of the other deployments "
                                "have no write path");
    const std::string v = kv["feat_learnable"];
    if (v != "sgd" && v != "adagrad") fatal(__FILE__, __LINE__, "feat_learnable = " + v + ": sgd or adagrad");
    cfg.feat_learnable = v == "sgd" ? GGMS_UPDATE_SGD : GGMS_UPDATE_ADAGRAD;
    // a whole, finite number that is finite as the f32 the kernel takes
    auto number = [&](const char *key, float &out) {
      const std::string s = kv[key];
      char *end = nullptr;
      const double d = std::strtod(s.c_str(), &end);
      out = (float)d;
      return !s.empty() && end == s.c_str() + s.size() && std::isfinite(d) && std::isfinite(out);
    };
    if (!kv.count("feat_lr")) fatal(__FILE__, __LINE__, "feat_learnable needs the config key feat_lr (the table's learning rate)");
    if (!number("feat_lr", cfg.feat_lr)) fatal(__FILE__, __LINE__, "feat_lr = " + kv["feat_lr"] + ": a finite number");
    if (cfg.feat_learnable == GGMS_UPDATE_ADAGRAD && kv.count("feat_eps") && !(number("feat_eps", cfg.feat_eps) && cfg.feat_eps > 0))
      fatal(__FILE__, __LINE__, "feat_eps = " + kv["feat_eps"] + ": a finite number > 0 (as f32)");
    if (kv.count("feat_store_dtype"))
      fatal(__FILE__, __LINE__, "feat_learnable with feat_store_dtype: the update reads and writes F32 rows, an encoded "
                                "table has none");
    if (cfg.feat_out_dtype >= 0 && cfg.feat_out_dtype != GGMS_F32)
      fatal(__FILE__, __LINE__, "feat_learnable with feat_out_dtype = " + kv["feat_out_dtype"] + ": the gradient comes back "
                                "in f32, row for row of what the batch delivered; f32 or no key");
    if (getenv("SAMGRAPH_EMPTY_FEAT"))
      fatal(__FILE__, __LINE__, "feat_learnable with SAMGRAPH_EMPTY_FEAT: several nodes share a row of a masked mock "
                                "table, an update has no single row to move");
    // gathers and updates are totally ordered on the one extract stream: a batch's rows reflect exactly the updates
    // enqueued before its gather was
    cfg.extract_streams = 1;
  }
  if (cfg.Temporal()) { // extension: sampling strictly before the positive edge's time
    const std::string who = "_sample_type 9 (khop_temporal)";
    if (!cfg.link_prediction)
      fatal(__FILE__, __LINE__, who + " needs task = link_prediction: a seed's time is the time of its positive edge; "
                                "task = node_classification has no time for a node");
    if (cfg.use_dist_graph)
      fatal(__FILE__, __LINE__, who + " with use_dist_graph: edge times are stored by position in ONE CSR, a sharded "
                                "topology has none");
    if (cfg.exclude_seed_edges)
      fatal(__FILE__, __LINE__, who + " with exclude_seed_edges = " + kv["exclude_seed_edges"] + ": strictly-before already "
                                "removes the positive, its mirror at the same time, and everything later.");
    if (kv.count("temporal_pick")) {
      const std::string v = kv["temporal_pick"];
      if (v != "uniform" && v != "recent")
        fatal(__FILE__, __LINE__, "temporal_pick = " + v + ": uniform (the default) or recent");
      cfg.temporal_pick = v == "recent" ? GGMS_PICK_RECENT : GGMS_PICK_UNIFORM;
    }
  }
  if (cfg.Typed()) { // extension: a fanout per edge type
    const std::string who = "_sample_type 10 (khop_typed)";
    if (cfg.use_dist_graph)
      fatal(__FILE__, __LINE__, who + " with use_dist_graph: edge types are stored by position in ONE CSR, a sharded "
                                "topology has none");
    if (cfg.exclude_seed_edges)
      fatal(__FILE__, __LINE__, who + " with exclude_seed_edges = " + kv["exclude_seed_edges"] + " is not built: the filter "
                                "compacts row / col and knows nothing of the position and type streams the sampler wrote "
                                "beside them");
    if (!kv.count("type_fanout"))
      fatal(__FILE__, __LINE__, who + " needs the config key type_fanout: num_layer x NUM_EDGE_TYPE fanouts, layer-major");
    std::stringstream ss(kv["type_fanout"]);
    long long v;
    while (ss >> v) {
      if (v < 0 || v >= 128)
        fatal(__FILE__, __LINE__, "type_fanout: the value " + std::to_string(v) + " is out of range: a relation's fanout is "
                                  "0 (not sampled) .. 127");
      cfg.type_fanout.push_back((uint32_t)v);
    }
    const size_t L = cfg.fanout.size(), nv = cfg.type_fanout.size();
    if (!ss.eof() || nv == 0 || nv % L != 0 || nv / L > GGMS_MAX_EDGE_TYPES)
      fatal(__FILE__, __LINE__, "type_fanout has " + std::to_string(nv) + " values: num_layer (" + std::to_string(L) +
                                ") rows of NUM_EDGE_TYPE (1 .. " + std::to_string(GGMS_MAX_EDGE_TYPES) + ") integers");
    cfg.num_edge_type = (uint32_t)(nv / L);
    for (size_t i = 0; i < L; ++i) {
      size_t sum = 0;
      for (uint32_t r = 0; r < cfg.num_edge_type; ++r) sum += cfg.type_fanout[i * cfg.num_edge_type + r];
      if (sum == 0)
        fatal(__FILE__, __LINE__, "type_fanout: row " + std::to_string(i) + " is all zero: a layer that samples no relation");
      if (sum != cfg.fanout[i])
        fatal(__FILE__, __LINE__, "fanout[" + std::to_string(i) + "] = " + std::to_string(cfg.fanout[i]) + " disagrees with "
                                  "type_fanout: row " + std::to_string(i) + " sums to " + std::to_string(sum) +
                                  " (leave fanout to the Python front-end, or give the rows' sums)");
    }
  }
  if (kv.count("edge_ids") || kv.count("edge_feat")) { // extension: CSR positions (and edge-table rows) of the sampled edges
    for (const char *key : {"edge_ids", "edge_feat"})
      if (kv.count(key) && kv[key] != "on" && kv[key] != "off")
        fatal(__FILE__, __LINE__, std::string(key) + " = " + kv[key] + ": on or off (the default)");
    cfg.edge_feat = kv.count("edge_feat") && kv["edge_feat"] == "on";
    cfg.edge_ids = cfg.edge_feat || (kv.count("edge_ids") && kv["edge_ids"] == "on");
  }
  if (cfg.SamplerEmitsEdgeIds()) cfg.edge_ids = true; // implied: the sampler emits the positions itself
  if (cfg.edge_ids) {
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    const std::string key = cfg.edge_feat ? "edge_feat" : "edge_ids";
    if (cfg.arch != kArch1)
      fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": " + key + " is not built: the edge positions are "
                                "computed behind arch1's sampling chain and travel through no hand-off or queue");
    if (cfg.use_dist_graph)
      fatal(__FILE__, __LINE__, key + " with use_dist_graph: an edge id is a position in ONE CSR, a sharded topology has "
                                "none");
    if (cfg.sample_type == GGMS_RANDOM_WALK)
      fatal(__FILE__, __LINE__, key + " with _sample_type 3 (random_walk) is not built: its edges join a node and a node "
                                "it visited, they are not edges of the graph");
    if (cfg.sample_type == GGMS_KHOP2)
      fatal(__FILE__, __LINE__, key + " with _sample_type 5 (khop2) is not built: khop2 permutes indices in place, a "
                                "position names another edge after every batch");
  }
  if (kv.count("induced_subgraph") || kv.count("induced_max_edges")) { // extension: the subgraph a batch's input nodes induce
    if (kv.count("induced_subgraph") && kv["induced_subgraph"] != "on" && kv["induced_subgraph"] != "off")
      fatal(__FILE__, __LINE__, "induced_subgraph = " + kv["induced_subgraph"] + ": on or off (the default)");
    cfg.induced = kv.count("induced_subgraph") && kv["induced_subgraph"] == "on";
    if (kv.count("induced_max_edges") && !cfg.induced)
      fatal(__FILE__, __LINE__, "induced_max_edges without induced_subgraph = on: the key sizes the induced arrays only");
  }
  if (cfg.induced) {
    static const char *const arch_names[] = {"arch0", "arch1", "arch2", "arch3", "arch4", "arch5", "arch6", "arch7"};
    if (cfg.arch != kArch1)
      fatal(__FILE__, __LINE__, std::string(arch_names[cfg.arch]) + ": induced_subgraph is not built: the induced edges are "
                                "computed behind arch1's sampling chain and travel through no hand-off or queue");
    if (cfg.use_dist_graph)
      fatal(__FILE__, __LINE__, "induced_subgraph with use_dist_graph is not built: the induced edges come with their "
                                "positions in ONE CSR, a sharded topology has none");
    if (cfg.sample_type == GGMS_KHOP2)
      fatal(__FILE__, __LINE__, "induced_subgraph with _sample_type 5 (khop2) is not built: khop2 permutes indices in "
                                "place, a position names another edge after every batch");
    if (cfg.Temporal())
      fatal(__FILE__, __LINE__, "induced_subgraph with _sample_type 9 (khop_temporal) is not built: an induced edge may lie "
                                "after a node's cut-off, which leaks the future into the batch");
    if (cfg.exclude_seed_edges)
      fatal(__FILE__, __LINE__, "induced_subgraph with exclude_seed_edges = " + kv["exclude_seed_edges"] + " is not built: "
                                "the filter does not compact an id stream, and the induced subgraph of a link batch holds "
                                "its positive edges; take exclude_seed_edges = none and drop them in the trainer");
    if (kv.count("induced_max_edges")) {
      unsigned long long v = 0;
      try {
        size_t used = 0;
        v = std::stoull(kv["induced_max_edges"], &used);
        if (used != kv["induced_max_edges"].size() || kv["induced_max_edges"][0] == '-') v = 0;
      } catch (...) { v = 0; }
      if (v == 0 || v >= 0xffffffffull - 1023ull)
        fatal(__FILE__, __LINE__, "induced_max_edges = " + kv["induced_max_edges"] + ": the capacity of a batch's induced "
                                  "arrays, 1 .. 2^32 - 1025 edges");
      cfg.induced_max_edges = (size_t)v;
    }
  }
  if (kv.count("typed_feat")) { // extension: one feature table per node type (in front of hetero_batch's own refusals)
    if (kv["typed_feat"] != "on" && kv["typed_feat"] != "off")
      fatal(__FILE__, __LINE__, "typed_feat = " + kv["typed_feat"] + ": on or off (the default)");
    cfg.typed_feat = kv["typed_feat"] == "on";
  }
  if (cfg.typed_feat) {
    if (!cfg.hetero)
      fatal(__FILE__, __LINE__, "typed_feat without hetero_batch = on is not built: the typed tables are gathered over the "
                                "batch's nodes grouped by type, which hetero_batch computes");
    if (cfg.feat_learnable >= 0)
      fatal(__FILE__, __LINE__, "typed_feat with feat_learnable is not built: the update moves rows of ONE F32 table; "
                                "per-type learnable tables are a follow-up");
    if (cfg.feat_store_dtype >= 0)
      fatal(__FILE__, __LINE__, "typed_feat with feat_store_dtype is not built: the quantiser re-encodes ONE table; FP8 and "
                                "Q8ROW typed tables are a follow-up");
    for (const char *e : {"SAMGRAPH_EMPTY_FEAT", "SAMGRAPH_FAKE_FEAT_DIM"})
      if (getenv(e))
        fatal(__FILE__, __LINE__, std::string("typed_feat with ") + e + " is not built: the stand-in is ONE table of one "
                                  "width; the typed tables are the dataset's own node_feat_<t>.bin");
  }
  if (cfg.hetero) { // (the key itself and the deployment: above, in front of khop_typed's own refusals)
    if (!cfg.Typed())
      fatal(__FILE__, __LINE__, "hetero_batch with _sample_type " + std::to_string(cfg.sample_type) + " is not built: the "
                                "relation of every sampled edge comes from _sample_type 10 (khop_typed) only");
    if (cfg.use_dist_graph) // (khop_typed refuses it first; kept for the day it does not)
      fatal(__FILE__, __LINE__, "hetero_batch with use_dist_graph is not built: relations are stored by position in ONE CSR");
    if (cfg.edge_feat)
      fatal(__FILE__, __LINE__, "hetero_batch with edge_feat is not built: the edge rows are gathered in the layers' "
                                "homogeneous order, not per relation");
    if (cfg.induced)
      fatal(__FILE__, __LINE__, "hetero_batch with induced_subgraph is not built: the induced edges carry no relation");
    if (cfg.feat_learnable >= 0)
      fatal(__FILE__, __LINE__, "hetero_batch with feat_learnable is not built: the gradient rows come back in the grouped "
                                "order, the update scatters them by input_nodes");
  }
  if (cfg.arch == kArch4) { // DoGPUSampleDyCache's switch (cuda/cuda_loops.cc:347-377) and what it needs
    if (cfg.sample_type != GGMS_KHOP0 && cfg.sample_type != GGMS_KHOP1 && cfg.sample_type != GGMS_WEIGHTED_KHOP)
      fatal(__FILE__, __LINE__, "arch4: _sample_type " + std::to_string(cfg.sample_type) + " is not supported: the "
                                "prefetching sampler takes khop0, khop1 and weighted_khop only");
    if (cfg.fanout.size() < 2)
      fatal(__FILE__, __LINE__, "arch4: num_layer " + std::to_string(cfg.fanout.size()) + ": the expansion follows the "
                                "second-to-last layer, so arch4 needs at least 2 layers");
    // a non-zero percentage takes the reference's static-cache branch (cuda/cuda_engine.cc:160-186), which its arch4
    // copy loop never reads: refused rather than built and ignored
    if (cfg.cache_policy == 6 && cfg.cache_percentage > 0)
      fatal(__FILE__, __LINE__, "arch4: cache policy dynamic_cache (6) takes cache_percentage 0 (got " +
                                kv["cache_percentage"] + "): it caches the previous batch's rows, not a ranked share");
    if (cfg.cache_policy != 6 && cfg.cache_percentage > 0)
      fatal(__FILE__, __LINE__, "arch4: cache_percentage " + kv["cache_percentage"] + " with the static cache policy " +
                                std::to_string(cfg.cache_policy) + ": arch4 reads every row from host memory or, with "
                                "dynamic_cache, from the previous batch; set cache_percentage 0");
    if (!cfg.direct_table) fatal(__FILE__, __LINE__, "arch4: hash_table = hashed: the superset needs the direct table layout");
    cfg.dynamic_cache = cfg.cache_policy == 6;
    if (cfg.dynamic_cache && cfg.feat_out_dtype >= 0)
      fatal(__FILE__, __LINE__, "arch4: feat_out_dtype with cache policy dynamic_cache (6): a gather reads the previous "
                                "batch's rows (the output dtype) beside the host table's (the table dtype), one dtype per source");
    if (cfg.dynamic_cache) cfg.extract_streams = 1; // gathers in batch order, each after the one whose rows it reads
    if (kv.count("prefetch_max_edges")) cfg.prefetch_max_edges = std::stoull(kv["prefetch_max_edges"]);
  }
  if (cfg.sample_type == GGMS_WEIGHTED_KHOP || cfg.sample_type == GGMS_KHOP2 || cfg.sample_type == GGMS_KHOP1 ||
      cfg.sample_type == GGMS_WEIGHTED_KHOP_PREFIX ||
      cfg.sample_type == GGMS_WEIGHTED_KHOP_HASH_DEDUP) // dist_loops.cc:167-168,171-172,209-210,219-220,227-228
    SAM_CHECK(!cfg.use_dist_graph, "this algorithm not support DistGraph engine");
  // shard base pointers travel in the kernels' arguments (include/ggms.h, GGMS_MAX_PARTS): a larger group is refused
  // HERE, before any shard is built, exported or mapped (the reference's device pointer tables take any num_part)
  if (cfg.arch == kArch6 && (cfg.use_dist_graph || cfg.part_cache))
    SAM_CHECK(cfg.num_worker <= GGMS_MAX_PARTS, "use_dist_graph / part_cache: at most GGMS_MAX_PARTS (8) workers share a sharded store");
  cfg.configured = true;
}

// ------------------------------------------------------------------ dataset
HostArray Engine::MapFile(const std::string &name, size_t bytes, bool to_shared_anon) {
  HostArray a;
  a.bytes = bytes;
  const std::string path = cfg.dataset_path + name;
  int fd = open(path.c_str(), O_RDONLY);
  SAM_CHECK(fd >= 0, "cannot open " + path);
  struct stat st;
  fstat(fd, &st);
  SAM_CHECK((size_t)st.st_size >= bytes, path + " is smaller than meta.txt says");
  void *m = bytes ? mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr; // Tensor::FromMmap
  SAM_CHECK(bytes == 0 || m != MAP_FAILED, "mmap failed for " + path);
  close(fd);
  if (to_shared_anon && bytes) {
    // ConverToAnonMmap, engine.cc:91-107: workers forked later share one locked copy
    void *s = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    SAM_CHECK(s != MAP_FAILED, "anonymous shared mmap failed");
    std::memcpy(s, m, bytes);
    munmap(m, bytes);
    a.ptr = s;
    a.shared_anon = true;
  } else {
    a.ptr = m;
    a.mapped_file = true;
  }
  return a;
}

static bool file_exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }

void Engine::LoadDataset() {
  if (cfg.dataset_path.back() != '/') cfg.dataset_path.push_back('/');
  // meta.txt, engine.cc:126-142; names constant.cc:23-51
  std::ifstream meta_file(cfg.dataset_path + "meta.txt");
  SAM_CHECK(meta_file.good(), "cannot read " + cfg.dataset_path + "meta.txt");
  std::unordered_map<std::string, size_t> meta;
  std::unordered_map<std::string, std::string> meta_text; // NODE_FEAT_DATA_TYPE_<t>: names, read by typed_feat only
  std::string line;
  while (std::getline(meta_file, line)) {
    std::istringstream iss(line);
    std::string k, v;
    if (!(iss >> k >> v)) break;
    if (k.rfind("NODE_FEAT_DATA_TYPE_", 0) == 0) {
      meta_text[k] = v;
    } else if (k == "FEAT_DATA_TYPE" && cfg.typed_feat) {
      // (the one table is neither mapped nor uploaded: whatever type it has concerns nobody)
    } else if (k == "FEAT_DATA_TYPE") {
      SAM_CHECK(kFeatDtypeNames.count(v), "unknown FEAT_DATA_TYPE " + v);
      ds.feat_dtype = kFeatDtypeNames.at(v);
      // (an FP8 table is a source of the converting gather only: without the key its rows are moved as bytes)
      if (cfg.feat_out_dtype >= 0 && !ggms::gather_converts_from(ds.feat_dtype))
        fatal(__FILE__, __LINE__, "feat_out_dtype with FEAT_DATA_TYPE " + v + ": the gather converts F16, BF16, F32, "
                                  "F8E4M3, F8E5M2 and Q8ROW tables only");
      // a row-scaled table has no element type to hand out raw: only the converting gather can deliver its rows
      if (ds.feat_dtype == GGMS_Q8ROW && cfg.feat_out_dtype < 0) fatal(__FILE__, __LINE__, kQ8RowNeedsOutDtype);
    } else if (k == "EDGE_FEAT_DATA_TYPE") { // (read whatever the config says: the file describes the dataset)
      SAM_CHECK(kFeatDtypeNames.count(v), "unknown EDGE_FEAT_DATA_TYPE " + v);
      ds.edge_feat_dtype = kFeatDtypeNames.at(v);
      if (cfg.edge_feat && ds.edge_feat_dtype == GGMS_Q8ROW)
        fatal(__FILE__, __LINE__, "edge_feat with EDGE_FEAT_DATA_TYPE Q8ROW: the edge rows are moved by the plain gather, "
                                  "which takes element types only; a row-scaled edge table is not built");
    } else {
      meta[k] = std::stoull(v);
    }
  }
  for (const char *k : {"NUM_NODE", "NUM_EDGE", "FEAT_DIM", "NUM_CLASS", "NUM_TRAIN_SET", "NUM_TEST_SET", "NUM_VALID_SET"})
    SAM_CHECK(meta.count(k), std::string("meta.txt lacks ") + k);
  ds.num_node = meta["NUM_NODE"]; ds.num_edge = meta["NUM_EDGE"]; ds.feat_dim = meta["FEAT_DIM"];
  ds.num_class = meta["NUM_CLASS"]; ds.num_train = meta["NUM_TRAIN_SET"]; ds.num_test = meta["NUM_TEST_SET"];
  ds.num_valid = meta["NUM_VALID_SET"];
  if (cfg.feat_learnable >= 0 && ds.feat_dtype != GGMS_F32) {
    std::string name = std::to_string(ds.feat_dtype);
    for (const auto &kvp : kFeatDtypeNames)
      if (kvp.second == ds.feat_dtype) name = kvp.first;
    fatal(__FILE__, __LINE__, "feat_learnable with FEAT_DATA_TYPE " + name + ": the learnable table is F32 (the update's "
                              "arithmetic is f32, one rounding per operation)");
  }
  const bool share = cfg.arch == kArch6; // forked workers read the same pages
  ds.indptr = MapFile("indptr.bin", (ds.num_node + 1) * 4, share);
  ds.indices = MapFile("indices.bin", ds.num_edge * 4, share);
  // SAMGRAPH_FAKE_FEAT_DIM (run_config.cc:156-159, engine.cc:202-204): pretend the features have this width and
  // do not read feat.bin -- lets a big graph run without its feature file
  size_t fake_dim = 0;
  if (const char *e = getenv("SAMGRAPH_FAKE_FEAT_DIM")) fake_dim = std::strtoull(e, nullptr, 10);
  if (fake_dim) ds.feat_dim = fake_dim;
  if (cfg.feat_store_dtype >= 0) { // what QuantizeStore reads: a real F32 / F16 table of another type than the store's
    const std::string key = "feat_store_dtype = " + cfg.raw["feat_store_dtype"];
    if (!ggms::quantiser_reads(ds.feat_dtype))
      fatal(__FILE__, __LINE__, key + ": the quantiser reads FEAT_DATA_TYPE F32 or F16, this dataset's table has another type");
    if (ds.feat_dtype == cfg.feat_store_dtype)
      fatal(__FILE__, __LINE__, key + ": FEAT_DATA_TYPE is that type already, there is nothing to encode; drop the key");
    if (fake_dim || getenv("SAMGRAPH_EMPTY_FEAT") || !file_exists(cfg.dataset_path + "feat.bin"))
      fatal(__FILE__, __LINE__, key + ": needs the dataset's own feat.bin; a stand-in table (SAMGRAPH_EMPTY_FEAT, "
                                "SAMGRAPH_FAKE_FEAT_DIM, or a dataset without feat.bin) is not quantised");
  }
  const size_t row_bytes = ds.feat_row_bytes();
  ds.feat_rows = ds.num_node;
  size_t empty_bits = 0; // SAMGRAPH_EMPTY_FEAT = k (run_config.cc:137-139, engine.cc:205-207): a 2^k-row stand-in table,
                         // node v reads row v & (2^k - 1) (gpu_mock_extract / cpu_mock_extract)
  if (const char *e = getenv("SAMGRAPH_EMPTY_FEAT")) empty_bits = std::strtoull(e, nullptr, 10);
  if (cfg.typed_feat) {
    // typed_feat: feat.bin is neither mapped nor uploaded; the tables are node_feat_<t>.bin (LoadTypedFeat, below)
    ds.feat_rows = 0;
  } else if (empty_bits) {
    SAM_CHECK(empty_bits < 32, "SAMGRAPH_EMPTY_FEAT out of range");
    ds.feat_rows = (size_t)1 << empty_bits;
    ds.feat_mask = (uint32_t)(ds.feat_rows - 1);
    ds.feat.bytes = ds.feat_rows * row_bytes;
    ds.feat.ptr = mmap(nullptr, ds.feat.bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    SAM_CHECK(ds.feat.ptr != MAP_FAILED, "feature mmap failed");
    ds.feat.shared_anon = true;
    ds.feat_is_fake = true;
    // the reference leaves the stand-in uninitialised; ours starts as the first 2^k rows of feat.bin where that file
    // exists (any content is as valid, and this one can be checked), zeros otherwise
    if (!fake_dim && file_exists(cfg.dataset_path + "feat.bin")) {
      HostArray f = MapFile("feat.bin", std::min(ds.feat_rows, ds.num_node) * row_bytes, false);
      std::memcpy(ds.feat.ptr, f.ptr, f.bytes);
    }
  } else if (!fake_dim && file_exists(cfg.dataset_path + "feat.bin")) {
    ds.feat = MapFile("feat.bin", ds.num_node * row_bytes, share);
  } else { // engine.cc:199-235: datasets without feat.bin get an (uninitialised) table; ours is zero-filled
    ds.feat.bytes = ds.num_node * row_bytes;
    ds.feat.ptr = mmap(nullptr, ds.feat.bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    SAM_CHECK(ds.feat.ptr != MAP_FAILED, "feature mmap failed");
    ds.feat.shared_anon = true;
    ds.feat_is_fake = true;
    // An anonymous mapping nobody has written is ONE zero page behind every address: a host gather of such a table reads
    // 4 KB over and over and measures the cache.  SAMGRAPH_FILL_FAKE_FEAT=1 gives every page a frame of its own (and the
    // rows a checkable content: 32-bit word w of the table holds w), filled by omp_thread_num threads.
    ds.feat_is_zero = !getenv("SAMGRAPH_FILL_FAKE_FEAT");
    if (!ds.feat_is_zero) {
      Team team((int)cfg.omp_thread_num);
      uint32_t *words = (uint32_t *)ds.feat.ptr;
      team.ParallelFor(ds.feat.bytes / 4, [&](size_t lo, size_t hi, int) {
        for (size_t w = lo; w < hi; ++w) words[w] = (uint32_t)w;
      });
    }
  }
  if (file_exists(cfg.dataset_path + "label.bin")) {
    ds.label = MapFile("label.bin", ds.num_node * 8, share);
  } else {
    ds.label.bytes = ds.num_node * 8;
    ds.label.ptr = mmap(nullptr, ds.label.bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    ds.label.shared_anon = true;
  }
  ds.train_set = MapFile("train_set.bin", ds.num_train * 4, false);
  ds.test_set = MapFile("test_set.bin", ds.num_test * 4, false);
  ds.valid_set = MapFile("valid_set.bin", ds.num_valid * 4, false);
  if (cfg.link_prediction) { // the train edge set: positions in indices.bin
    const std::string name = cfg.dataset_path + "train_edge_set.bin";
    if (file_exists(name)) {
      struct stat st;
      SAM_CHECK(stat(name.c_str(), &st) == 0 && st.st_size % 4 == 0, "train_edge_set.bin: uint32 CSR positions expected");
      ds.num_train_edge = (size_t)st.st_size / 4;
      ds.train_edge_set = MapFile("train_edge_set.bin", ds.num_train_edge * 4, false);
      ds.train_edges = (const uint32_t *)ds.train_edge_set.ptr;
      for (size_t i = 0; i < ds.num_train_edge; ++i)
        if (ds.train_edges[i] >= ds.num_edge)
          fatal(__FILE__, __LINE__, "train_edge_set.bin: entry " + std::to_string(i) + " is " +
                                        std::to_string(ds.train_edges[i]) + ", the graph has " +
                                        std::to_string(ds.num_edge) + " edges (ids are positions in indices.bin)");
    } else { // every edge once per epoch
      if (ds.num_edge >= (1ull << 32))
        fatal(__FILE__, __LINE__, "task = link_prediction without train_edge_set.bin takes every edge: " +
                                      std::to_string(ds.num_edge) + " edges do not fit 32-bit edge ids");
      ds.all_edges.resize(ds.num_edge);
      for (size_t i = 0; i < ds.num_edge; ++i) ds.all_edges[i] = (uint32_t)i;
      ds.train_edges = ds.all_edges.data();
      ds.num_train_edge = ds.num_edge;
    }
    SAM_CHECK(ds.num_train_edge > 0, "task = link_prediction: the train edge set is empty");
  }
  if (cfg.edge_ids && ds.num_edge >= 0xffffffffull)
    fatal(__FILE__, __LINE__, std::string(cfg.edge_feat ? "edge_feat" : "edge_ids") + ": " + std::to_string(ds.num_edge) +
                                  " edges: edge ids are 32-bit positions, at most 2^32 - 2 of them");
  if (cfg.induced && ds.num_edge >= 0xffffffffull)
    fatal(__FILE__, __LINE__, "induced_subgraph: " + std::to_string(ds.num_edge) + " edges: the induced edges come with "
                                  "32-bit positions, at most 2^32 - 2 of them");
  if (cfg.edge_feat) { // the edge table: NUM_EDGE rows in CSR order
    if (!meta.count("EDGE_FEAT_DIM") || meta["EDGE_FEAT_DIM"] == 0)
      fatal(__FILE__, __LINE__, "edge_feat: meta.txt lacks EDGE_FEAT_DIM (elements per row of edge_feat.bin)");
    ds.edge_feat_dim = meta["EDGE_FEAT_DIM"];
    const std::string name = cfg.dataset_path + "edge_feat.bin";
    struct stat st;
    if (stat(name.c_str(), &st) != 0)
      fatal(__FILE__, __LINE__, "edge_feat: " + name + " is missing (NUM_EDGE rows of EDGE_FEAT_DIM elements, CSR order)");
    const size_t want = ds.num_edge * ds.edge_feat_row_bytes();
    if ((size_t)st.st_size != want)
      fatal(__FILE__, __LINE__, "edge_feat: edge_feat.bin has " + std::to_string((size_t)st.st_size) + " bytes, NUM_EDGE x "
                                    "EDGE_FEAT_DIM x the element size is " + std::to_string(want));
    ds.edge_feat = MapFile("edge_feat.bin", want, false);
  }
  if (cfg.Temporal()) { // the edge times: NUM_EDGE uint32 in CSR order, sorted inside every list
    const std::string name = cfg.dataset_path + "edge_time.bin";
    struct stat st;
    if (stat(name.c_str(), &st) != 0)
      fatal(__FILE__, __LINE__, "khop_temporal: " + name + " is missing (NUM_EDGE uint32 times, one per position of "
                                    "indices.bin; datagen.write_dataset(edge_time=...))");
    if ((size_t)st.st_size != ds.num_edge * 4)
      fatal(__FILE__, __LINE__, "khop_temporal: edge_time.bin has " + std::to_string((size_t)st.st_size) + " bytes, NUM_EDGE x 4 is " +
                                    std::to_string(ds.num_edge * 4));
    ds.edge_time = MapFile("edge_time.bin", ds.num_edge * 4, false);
    const uint32_t *ip = (const uint32_t *)ds.indptr.ptr, *t = (const uint32_t *)ds.edge_time.ptr;
    for (size_t v = 0; v < ds.num_node; ++v)
      for (size_t p = (size_t)ip[v] + 1; p < ip[v + 1]; ++p)
        if (t[p] < t[p - 1])
          fatal(__FILE__, __LINE__, "khop_temporal: edge_time.bin: the times of node " + std::to_string(v) + "'s list are not "
                                        "non-decreasing (position " + std::to_string(p) + "); datagen.sort_lists_by_time "
                                        "re-sorts a graph");
  }
  if (cfg.hetero) { // the node types: NUM_NODE uint8 below NUM_NODE_TYPE
    if (!meta.count("NUM_NODE_TYPE"))
      fatal(__FILE__, __LINE__, "hetero_batch: meta.txt lacks NUM_NODE_TYPE (datagen.write_dataset(node_type=, num_node_type=))");
    const size_t T = meta["NUM_NODE_TYPE"];
    if (T < 1 || T > GGMS_MAX_NODE_TYPES)
      fatal(__FILE__, __LINE__, "hetero_batch: NUM_NODE_TYPE = " + std::to_string(T) + ": 1 .. " + std::to_string(GGMS_MAX_NODE_TYPES));
    const std::string name = cfg.dataset_path + "node_type.bin";
    struct stat st;
    if (stat(name.c_str(), &st) != 0)
      fatal(__FILE__, __LINE__, "hetero_batch: " + name + " is missing (NUM_NODE uint8 types, one per node id; "
                                    "datagen.write_dataset(node_type=...))");
    if ((size_t)st.st_size != ds.num_node)
      fatal(__FILE__, __LINE__, "hetero_batch: node_type.bin has " + std::to_string((size_t)st.st_size) + " bytes, NUM_NODE is " +
                                    std::to_string(ds.num_node));
    ds.node_type = MapFile("node_type.bin", ds.num_node, false);
    ds.num_node_type = (uint32_t)T;
    const uint8_t *nt = (const uint8_t *)ds.node_type.ptr;
    for (size_t v = 0; v < ds.num_node; ++v)
      if (nt[v] >= T)
        fatal(__FILE__, __LINE__, "hetero_batch: node_type.bin: node " + std::to_string(v) + " has the type " +
                                      std::to_string((unsigned)nt[v]) + ", NUM_NODE_TYPE is " + std::to_string(T));
    if (cfg.typed_feat) LoadTypedFeat(meta, meta_text);
  }
  if (cfg.Typed()) { // the edge types: NUM_EDGE uint8 in CSR order, sorted inside every list, below NUM_EDGE_TYPE
    if (!meta.count("NUM_EDGE_TYPE"))
      fatal(__FILE__, __LINE__, "khop_typed: meta.txt lacks NUM_EDGE_TYPE (datagen.write_dataset(edge_type=, num_edge_type=))");
    const size_t R = meta["NUM_EDGE_TYPE"];
    if (R < 1 || R > GGMS_MAX_EDGE_TYPES)
      fatal(__FILE__, __LINE__, "khop_typed: NUM_EDGE_TYPE = " + std::to_string(R) + ": 1 .. " + std::to_string(GGMS_MAX_EDGE_TYPES));
    if (R != cfg.num_edge_type)
      fatal(__FILE__, __LINE__, "type_fanout has " + std::to_string(cfg.type_fanout.size()) + " values, num_layer x "
                                    "NUM_EDGE_TYPE is " + std::to_string(cfg.fanout.size()) + " x " + std::to_string(R));
    const std::string name = cfg.dataset_path + "edge_type.bin";
    struct stat st;
    if (stat(name.c_str(), &st) != 0)
      fatal(__FILE__, __LINE__, "khop_typed: " + name + " is missing (NUM_EDGE uint8 types, one per position of "
                                    "indices.bin; datagen.write_dataset(edge_type=...))");
    if ((size_t)st.st_size != ds.num_edge)
      fatal(__FILE__, __LINE__, "khop_typed: edge_type.bin has " + std::to_string((size_t)st.st_size) + " bytes, NUM_EDGE is " +
                                    std::to_string(ds.num_edge));
    ds.edge_type = MapFile("edge_type.bin", ds.num_edge, false);
    const uint32_t *ip = (const uint32_t *)ds.indptr.ptr;
    const uint8_t *t = (const uint8_t *)ds.edge_type.ptr;
    // hetero_batch: the same pass derives every relation's (source type, destination type) -- the list's owner is the
    // edge's destination, the entry its source -- and fails on the first edge that disagrees with its relation's others
    const uint8_t *nt = cfg.hetero ? (const uint8_t *)ds.node_type.ptr : nullptr;
    const uint32_t *ix = (const uint32_t *)ds.indices.ptr;
    if (cfg.hetero) {
      ds.rel_src_type.assign(R, 255);
      ds.rel_dst_type.assign(R, 255);
    }
    const auto pass_t0 = std::chrono::steady_clock::now();
    for (size_t v = 0; v < ds.num_node; ++v) // order and range in one pass: a sorted list's largest type is its last
      for (size_t p = ip[v]; p < ip[v + 1]; ++p) {
        if (nt && t[p] < R && ix[p] < ds.num_node) {
          const uint8_t src = nt[ix[p]], dst = nt[v];
          uint8_t &rs = ds.rel_src_type[t[p]], &rd = ds.rel_dst_type[t[p]];
          if (rs == 255) {
            rs = src;
            rd = dst;
          } else if (rs != src || rd != dst) {
            fatal(__FILE__, __LINE__, "hetero_batch: relation " + std::to_string((unsigned)t[p]) + " has two signatures: (source "
                                          "type " + std::to_string((unsigned)rs) + ", destination type " + std::to_string((unsigned)rd) +
                                          ") and (source type " + std::to_string((unsigned)src) + ", destination type " +
                                          std::to_string((unsigned)dst) + ") at position " + std::to_string(p) + " of node " +
                                          std::to_string(v) + "'s list; datagen.relation_types derives consistent relations");
          }
        }
        if (p > ip[v] && t[p] < t[p - 1])
          fatal(__FILE__, __LINE__, "khop_typed: edge_type.bin: the types of node " + std::to_string(v) + "'s list are not "
                                        "non-decreasing (position " + std::to_string(p) + "); datagen.sort_lists_by_type "
                                        "re-sorts a graph");
        if (t[p] >= R)
          fatal(__FILE__, __LINE__, "khop_typed: edge_type.bin: node " + std::to_string(v) + "'s list holds the type " +
                                        std::to_string((unsigned)t[p]) + " (position " + std::to_string(p) +
                                        "), NUM_EDGE_TYPE is " + std::to_string(R));
      }
    if (cfg.hetero)
      log_info("hetero_batch: " + std::to_string(ds.num_node_type) + " node types, " + std::to_string(R) + " relations; the "
               "pass over edge_type.bin with the relations' signatures took " +
               std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - pass_t0).count()) + " s");
  }
  if (cfg.sample_type == GGMS_WEIGHTED_KHOP || cfg.sample_type == GGMS_WEIGHTED_KHOP_HASH_DEDUP) { // engine.cc:372-384
    ds.prob_table = MapFile("prob_table.bin", ds.num_edge * 4, false);
    ds.alias_table = MapFile("alias_table.bin", ds.num_edge * 4, false);
  }
  if (cfg.sample_type == GGMS_WEIGHTED_KHOP_PREFIX) // :373-378; the kernels see it through extra_.prob_table
    ds.prob_table = MapFile("prob_prefix_table.bin", ds.num_edge * 4, false);
  if (cfg.UseGPUCache()) { // engine.cc:395-440
    static const char *rank_files[] = {"cache_by_degree.bin", "cache_by_heuristic.bin", nullptr, "cache_by_degree_hop.bin",
                                       nullptr, "cache_by_fake_optimal.bin", nullptr, "cache_by_random.bin"};
    if (cfg.cache_policy == 4 && cfg.arch == kArch0) // cpu/cpu_engine.cc:159
      fatal(__FILE__, __LINE__, "arch0: cache policy presample_static (4) is not built for the CPU engine: it ranks the "
                                "nodes with a GPU closure kernel (arch3, arch5, arch6); see DESIGN.md");
    if (cfg.cache_policy == 6) // (arch4 refuses a percentage in Configure)
      fatal(__FILE__, __LINE__, "cache policy dynamic_cache (6) is not built: it needs arch4 and a per-batch cache "
                                "replacement manager; see DESIGN.md");
    if (cfg.UsePresample()) {
      // filled by worker 0 in SampleInit, read by every worker (dist_engine.cc:455-466): shared pages
      ds.ranking_nodes.bytes = ds.num_node * 4;
      ds.ranking_nodes.ptr = mmap(nullptr, ds.ranking_nodes.bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
      SAM_CHECK(ds.ranking_nodes.ptr != MAP_FAILED, "ranking mmap failed");
      ds.ranking_nodes.shared_anon = true;
    } else {
      SAM_CHECK(cfg.cache_policy >= 0 && cfg.cache_policy < 8 && rank_files[cfg.cache_policy],
                "cache policy " + std::to_string(cfg.cache_policy) + " is not a cache policy: see DESIGN.md");
      ds.ranking_nodes = MapFile(rank_files[cfg.cache_policy], ds.num_node * 4, false);
    }
  }
}

void Engine::DataInit() {
  SAM_CHECK(cfg.configured, "samgraph_config first");
  if (data_ready_) return;
  auto t0 = std::chrono::steady_clock::now();
  LoadDataset();
  if (cfg.arch == kArch6) {
    shared_ = (Shared *)mmap(nullptr, sizeof(Shared), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    SAM_CHECK(shared_ != MAP_FAILED, "control block mmap failed");
    SAM_CHECK(cfg.num_worker <= (size_t)Shared::kMaxWorker, "too many workers");
    static_assert(std::atomic<uint32_t>::is_always_lock_free, "the worker barrier lives in shared memory");
    shared_->arrived.store(0);
    shared_->generation.store(0);
    shared_->num_worker = (int)cfg.num_worker;
    // DistGraph::DistGraph -> PartitionSolver (dist_graph.cu:592-594): which GPUs reach which, before anything is placed
    if (cfg.num_worker > 1 && (cfg.use_dist_graph || cfg.part_cache)) DetectTopo();
  }
  if (cfg.arch == kArch5) {
    num_global_step_ = (ds.num_train + cfg.batch_size - 1) / cfg.batch_size; // dist_engine.cc:139-142, drop_last false
    ComputeBounds();
    QueueInit();
  }
  if (cfg.induced) ResolveInducedCapacity();
  prof.LogInit(/*kLogInitL2LoadDataset*/ 6, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  data_ready_ = true;
}

// induced_subgraph: how many edges a batch's induced arrays hold.  Without the key `induced_max_edges`: the sum of the
// layers' edge capacities, capped at NUM_EDGE -- a CAPACITY default, not a measurement: the sampled layers hold at most
// that many edges among the same nodes, the induced subgraph holds every edge among them and may hold more (a dense
// neighbourhood; the batch then dies by name, with the count it needed).  Host arithmetic, known after data_init.
void Engine::ResolveInducedCapacity() {
  ComputeBounds();
  size_t sum = 0;
  for (size_t m : max_edges_) sum += m;
  const size_t dflt = std::max<size_t>(std::min<size_t>(std::min(sum, ds.num_edge), 0xffffffffull - 1025ull), 1);
  induced_max_edges_ = cfg.induced_max_edges ? cfg.induced_max_edges : dflt;
  log_info("induced_subgraph: induced_max_edges = " + std::to_string(induced_max_edges_) +
           (cfg.induced_max_edges ? " (config)" : " (default: the layers' edge capacities, " + std::to_string(sum) +
                                                      ", capped at NUM_EDGE = " + std::to_string(ds.num_edge) + ")"));
}

static double ipc_timeout_s();

// PartitionSolver::PartitionSolver + DetectTopo (dist_graph.cu:673-726): the parent must not touch the GPU before it
// forks its workers, so -- like the reference -- the probe runs in a forked child that sees every device: P2P
// reachability of every pair and a timed 128-MiB copy per reachable pair (ggms_detect_topology), kept in the
// reference's file format (read back here; reused by later runs on the same node, `SAMGRAPH_TOPO_FILE` names it).
// What the answer is used for: workers dereference each other's shards in place (DeviceDistGraph / DeviceDistFeature),
// so a pair of workers' GPUs that cannot reach each other is fatal HERE, with the pair named, instead of as a refused
// hipIpcOpenMemHandle after every shard has been built.  The reference's solver goes on to search clique placements
// for partially connected NVLink boxes (:728-777); an MI355X node is one clique (every GPU pair has its own xGMI
// link), so the placement is the modulo sharding of the whole group and the matrix is logged, not searched.
// A probe that cannot run (no device visible to the child, child killed) is a warning: placement does not depend on it.
void Engine::DetectTopo() {
  if (getenv("SAMGRAPH_FORCE_DEVICE")) return; // one-GPU rehearsal: every worker on one device, nothing to probe
  std::string file;
  if (const char *e = getenv("SAMGRAPH_TOPO_FILE")) {
    file = e;
  } else {
    const char *vis = getenv("HIP_VISIBLE_DEVICES");
    if (!vis) vis = getenv("ROCR_VISIBLE_DEVICES");
    std::string tag = vis ? vis : "all";
    for (auto &c : tag) if (!isalnum((unsigned char)c)) c = '_';
    const char *tmp = getenv("TMPDIR");
    file = std::string(tmp && *tmp ? tmp : "/tmp") + "/.detect_topo_amd_" + std::to_string((long)getuid()) + "_" + tag; // Constant::kDetectTopoFile
  }
  auto usable = [&](const ggms_topology_t &t) { return t.num_device >= (int)cfg.num_worker; };
  const auto t0 = std::chrono::steady_clock::now();
  bool probed = false;
  if (ggms_topology_read_host(&topo_, file.c_str()) != GGMS_OK || !usable(topo_)) {
    const pid_t pid = fork();
    SAM_CHECK(pid != -1, "fork of the topology probe failed");
    if (pid == 0) { // DetectTopo_child, :779-884
      ggms_topology_t t;
      int rc = ggms_detect_topology(&t, 0, 2);
      if (rc != GGMS_OK) fprintf(stderr, "[samgraph-amd] topology probe: %s\n", ggms_last_error());
      if (rc == GGMS_OK) rc = ggms_topology_write_host(&t, file.c_str(), "HIP_VISIBLE_DEVICES order");
      _exit(rc == GGMS_OK ? 0 : 1);
    }
    int wstatus = 0;
    bool done = false;
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < std::min(120.0, ipc_timeout_s())) {
      const pid_t r = waitpid(pid, &wstatus, WNOHANG);
      if (r == pid || r == -1) { done = true; break; }
      usleep(20000);
    }
    if (!done) { // a probe that hangs must not hold the run
      kill(pid, SIGKILL);
      waitpid(pid, &wstatus, 0);
      wstatus = -1;
    }
    probed = done && WIFEXITED(wstatus) && WEXITSTATUS(wstatus) == 0;
    if (!probed || ggms_topology_read_host(&topo_, file.c_str()) != GGMS_OK) {
      fprintf(stderr, "[samgraph-amd] warning: the topology probe did not complete (%s); placing %zu modulo shards without it\n",
              done ? "child failed" : "child timed out", cfg.num_worker);
      return;
    }
  }
  SAM_CHECK(usable(topo_), "arch6 with " + std::to_string(cfg.num_worker) + " workers, but the node shows " +
                               std::to_string(topo_.num_device) + " GPUs (" + file + ")");
  topo_valid_ = true;
  for (size_t i = 0; i < cfg.num_worker; ++i)
    for (size_t j = 0; j < cfg.num_worker; ++j)
      if (i != j && !topo_.can_access[i][j])
        fatal(__FILE__, __LINE__, "GPU " + std::to_string(i) + " cannot access GPU " + std::to_string(j) +
                                      " (hipDeviceCanAccessPeer, " + file + "): workers read each other's GGMS shards in "
                                      "place (use_dist_graph / part_cache), which needs P2P access between every pair of "
                                      "their GPUs");
  std::ostringstream ss; // "Topology Detect Debug", :714-722
  ss << "topology (" << (probed ? "probed in " : "read from " + file + " in ")
     << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s): GB/s INTO row FROM column\n";
  char cell[32];
  for (size_t i = 0; i < cfg.num_worker; ++i) {
    for (size_t j = 0; j < cfg.num_worker; ++j) {
      snprintf(cell, sizeof(cell), "%8.1f ", topo_.copy_GBps[i][j]);
      ss << cell;
    }
    ss << "\n";
  }
  log_info(ss.str());
  prof.LogInit(/*kLogInitL3DistGraphDetectTopo: extension slot*/ 40, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

// Every wait on another worker has a deadline (SAMGRAPH_IPC_TIMEOUT_S, default 300 s): a worker that died, or a
// hipIpcOpenMemHandle that never returns (seen on ROCm 7.2 for exporter sizes with bit 31 set, include/ggms.h
// ggms_ipc_safe_bytes), must end the run with a message instead of holding it until somebody's time limit.
static double ipc_timeout_s() {
  static const double v = [] { const char *e = getenv("SAMGRAPH_IPC_TIMEOUT_S"); const double x = e ? atof(e) : 0; return x > 0 ? x : 300.0; }();
  return v;
}

void Engine::Barrier(const char *what) {
  if (!shared_ || cfg.num_worker <= 1) return;
  const uint32_t gen = shared_->generation.load(std::memory_order_acquire);
  const uint32_t here = shared_->arrived.fetch_add(1, std::memory_order_acq_rel) + 1;
  if (here == (uint32_t)cfg.num_worker) { // last one in: re-arm, then release the others
    shared_->arrived.store(0, std::memory_order_relaxed);
    shared_->generation.fetch_add(1, std::memory_order_release);
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t spin = 0;; ++spin) {
    if (shared_->generation.load(std::memory_order_acquire) != gen) return;
    if (spin < 4096) continue; // a step barrier is usually released within microseconds
    if ((spin & 63) == 0) {
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (waited > ipc_timeout_s())
        fatal(__FILE__, __LINE__, "worker " + std::to_string(worker_id_) + " (device " + std::to_string(device_) + ") waited " +
                                      std::to_string((int)waited) + " s at the worker barrier '" + what + "': " +
                                      std::to_string(shared_->arrived.load()) + " of " + std::to_string(cfg.num_worker) +
                                      " workers arrived -- a worker died or is stuck (SAMGRAPH_IPC_TIMEOUT_S)");
    }
    spin < 65536 ? (void)sched_yield() : (void)usleep(200);
  }
}

// hipIpcOpenMemHandle under a deadline: the call runs on a helper thread; if it has not returned in time the process
// ends with a message (the thread cannot be cancelled, so there is nothing to retry in-process).
void *Engine::OpenPeer(const hipIpcMemHandle_t &handle, uint32_t peer, size_t bytes, const char *what) {
  struct State { std::mutex m; std::condition_variable cv; bool done = false; hipError_t err = hipSuccess; void *ptr = nullptr; };
  auto st = std::make_shared<State>();
  const int dev = device_;
  std::thread([st, handle, dev] {
    void *p = nullptr;
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipIpcOpenMemHandle(&p, handle, hipIpcMemLazyEnablePeerAccess);
    std::lock_guard<std::mutex> g(st->m);
    st->err = e;
    st->ptr = p;
    st->done = true;
    st->cv.notify_all();
  }).detach();
  std::unique_lock<std::mutex> lk(st->m);
  if (!st->cv.wait_for(lk, std::chrono::duration<double>(ipc_timeout_s()), [&] { return st->done; }))
    fatal(__FILE__, __LINE__, std::string("hipIpcOpenMemHandle(") + what + ") did not return within " +
                                  std::to_string((int)ipc_timeout_s()) + " s: worker " + std::to_string(worker_id_) + " (device " +
                                  std::to_string(device_) + ") opening the shard of worker " + std::to_string(peer) + ", " +
                                  std::to_string(bytes) + " bytes (SAMGRAPH_IPC_TIMEOUT_S)");
  SAM_CHECK(st->err == hipSuccess, std::string("hipIpcOpenMemHandle(") + what + ") from worker " + std::to_string(peer) + ": " +
                                       hipGetErrorString(st->err));
  return st->ptr;
}

// ------------------------------------------------------------------ shuffler
// GPUShuffler (cuda/cuda_shuffler.cc:38-160) for one worker, DistAlignedShuffler
// (dist/dist_shuffler_aligned.cc:37-146) for arch6, DistShuffler (dist/dist_shuffler.cc:37-90) for arch5's samplers:
// same Fisher-Yates with std::default_random_engine(seed) + uniform_int_distribution<size_t>(i, n-1).
void Engine::ShufflerInit() {
  const uint32_t *train = SeedSet();
  if (cfg.arch == kArch5) {
    // the epoch's ceil(num_train / batch_size) steps in consecutive ranges: the first (steps % S) samplers take one step
    // more ("large"), e.g. 15 steps over 4 samplers = 4, 4, 4, 3.  No padding, the last batch may be short.  (The
    // reference sizes a large sampler's slice as whole batches even where the train set ends inside it -- more
    // samplers than steps; here every slice ends at the train set.)
    const size_t S = cfg.num_sample_worker, w = (size_t)worker_id_, steps = num_global_step_;
    const size_t large = steps % S, small = steps / S;
    num_data_ = ds.num_train;
    shuf_host_.assign(train, train + num_data_);
    num_local_step_ = w < large ? small + 1 : small;
    global_step_offset_ = w < large ? (small + 1) * w : small * w + large;
    global_data_offset_ = global_step_offset_ * cfg.batch_size;
    num_local_data_ = std::min(num_local_step_ * cfg.batch_size,
                               num_data_ > global_data_offset_ ? num_data_ - global_data_offset_ : 0);
  } else {
    const size_t nw = cfg.arch == kArch6 ? cfg.num_worker : 1;
    const size_t origin = SeedSetSize();
    num_data_ = (origin + nw - 1) / nw * nw; // aligned to num_worker (:46)
    shuf_host_.assign(train, train + origin);
    for (size_t i = 0; i < num_data_ - origin; ++i) shuf_host_.push_back(train[i]); // :52-54
    num_local_data_ = num_data_ / nw;
    num_local_step_ = (num_local_data_ + cfg.batch_size - 1) / cfg.batch_size;
    num_global_step_ = num_local_step_ * nw;
    global_step_offset_ = num_local_step_ * worker_id_;
    global_data_offset_ = num_local_data_ * worker_id_;
  }
  const size_t origin = SeedSetSize();
  cur_epoch_ = 0;
  cur_step_ = num_local_step_;
  shuf_initialized_ = false;
  SAM_HIP(hipMalloc((void **)&shuf_dev_, std::max<size_t>(1, num_local_data_) * 4));
  { // a train SET: no node twice (what lets a batch promise distinct seeds to the sampler)
    std::vector<bool> seen(ds.num_node, false);
    train_distinct_ = !cfg.link_prediction; // (the endpoints of a batch of edges repeat: never promised distinct)
    for (size_t i = 0; i < origin && train_distinct_; ++i) {
      if (train[i] >= ds.num_node || seen[train[i]]) train_distinct_ = false;
      else seen[train[i]] = true;
    }
  }
}

// both copies of a padding node inside [offset, offset + size) of this worker's slice?
bool Engine::BatchSeedsDistinct(size_t offset, size_t size) const {
  if (!train_distinct_) return false;
  for (const auto &pr : pad_pairs_)
    if (pr.first >= offset && pr.first < offset + size && pr.second >= offset && pr.second < offset + size) return false;
  return true;
}

void Engine::Reshuffle() {
  if (!shuf_initialized_) { cur_epoch_ = 0; shuf_initialized_ = true; } else { cur_epoch_++; }
  cur_step_ = 0;
  if (cur_epoch_ >= cfg.num_epoch) return;
  uint64_t seed;
  if (cfg.arch == kArch6 || cfg.arch == kArch5) seed = cur_epoch_; // all samplers share the permutation (:92-94)
  else if (cfg.has_seed) seed = cfg.seed + cur_epoch_;
  else seed = std::chrono::system_clock::now().time_since_epoch().count(); // cuda_shuffler.cc:89
  auto g = std::default_random_engine(seed);
  uint32_t *data = shuf_host_.data();
  for (size_t i = 0; num_data_ && i < num_data_ - 1; i++) {
    std::uniform_int_distribution<size_t> d(i, num_data_ - 1);
    std::swap(data[i], data[d(g)]);
  }
  // where the padding copies went (at most num_worker - 1 nodes appear twice in the aligned epoch)
  pad_pairs_.clear();
  if (num_data_ > SeedSetSize()) {
    const uint32_t *train = SeedSet();
    std::unordered_map<uint32_t, size_t> first;
    for (size_t i = 0; i < num_data_ - SeedSetSize(); ++i) first[train[i]] = (size_t)-1;
    for (size_t pos = 0; pos < num_data_; ++pos) {
      auto it = first.find(data[pos]);
      if (it == first.end()) continue;
      if (it->second == (size_t)-1) { it->second = pos; continue; }
      const size_t a = it->second, b = pos, lo = global_data_offset_, hi = global_data_offset_ + num_local_data_;
      if (a >= lo && a < hi && b >= lo && b < hi) pad_pairs_.emplace_back(a - lo, b - lo);
    }
  }
  // the previous epoch's batches may still be copying their seeds out of shuf_dev_ on the pipeline streams
  for (auto &P : pipes_)
    if (P.stream) SAM_HIP(hipStreamSynchronize(P.stream));
  if (num_local_data_)
    SAM_HIP(hipMemcpyAsync(shuf_dev_, data + global_data_offset_, num_local_data_ * 4, hipMemcpyHostToDevice, stream_));
  SAM_HIP(hipStreamSynchronize(stream_));
}

// SAMGRAPH_SANITY_CHECK (cuda_shuffler.cc:147-154): no invalid id in the batch (GPUSanityCheckList) and no train node
// handed out twice within an epoch (GPUBatchSanityCheck).  The shuffled train set has a host copy, so the check
// runs there; a violation is fatal, as the device-side asserts of the reference are.
void Engine::SanityCheckBatch(const uint32_t *seeds, size_t n) {
  if (cur_step_ == 0) sanity_seen_.assign(ds.num_node, false);
  for (size_t i = 0; i < n; ++i) {
    SAM_CHECK(seeds[i] != GGMS_EMPTY_KEY && seeds[i] < ds.num_node, "sanity check: invalid node id in a batch");
    SAM_CHECK(!sanity_seen_[seeds[i]], "sanity check: a train node was handed out twice in one epoch");
    sanity_seen_[seeds[i]] = true;
  }
}

bool Engine::ShufflerNext(Batch *b, hipStream_t copy_stream) {
  if (num_local_step_ == 0) return false; // arch5: a sampler with no step (more samplers than steps)
  cur_step_++;
  if (cur_step_ >= num_local_step_) Reshuffle();
  if (cur_epoch_ >= cfg.num_epoch) return false;
  const size_t offset = cur_step_ * cfg.batch_size;
  SAM_CHECK(offset < num_local_data_, "shuffler offset out of range");
  size_t size = (offset + cfg.batch_size > num_local_data_) ? (num_local_data_ - offset) : cfg.batch_size;
  if (cfg.arch == kArch6 && cur_epoch_ == 0 && cur_step_ == 0) { // first batch x1.25, :137-140
    size = (size_t)(size * 1.25);
    size = (offset + size > num_local_data_) ? (num_local_data_ - offset) : size;
  }
  b->num_seeds = size;
  b->key = BatchKey(cur_epoch_, global_step_offset_ + cur_step_);
  static const bool sanity = getenv("SAMGRAPH_SANITY_CHECK") != nullptr; // run_config.cc:126-128
  if (cfg.link_prediction) { // the slice holds edge ids: SampleInto turns them into the batch's seed list
    b->num_pos = size;
    b->num_seeds = size * (2 + cfg.num_negative);
    SAM_HIP(hipMemcpyAsync(b->edge_ids, shuf_dev_ + offset, size * 4, hipMemcpyDeviceToDevice, copy_stream));
    return true;
  }
  if (sanity && (cfg.arch == kArch1 || Dedicated())) SanityCheckBatch(shuf_host_.data() + global_data_offset_ + offset, size);
  SAM_HIP(hipMemcpyAsync(b->sampler.output_nodes, shuf_dev_ + offset, size * 4, hipMemcpyDeviceToDevice, copy_stream)); // Copy1D
  return true;
}

// typed_feat: NODE_FEAT_DIM_<t> / NODE_FEAT_DATA_TYPE_<t> and node_feat_<t>.bin for every node type; every node's rank
// inside its type (row k of a table belongs to the type's k-th node in ascending id).  Behind the node types' own check.
void Engine::LoadTypedFeat(const std::unordered_map<std::string, size_t> &meta,
                           const std::unordered_map<std::string, std::string> &meta_text) {
  const size_t T = ds.num_node_type;
  const uint8_t *nt = (const uint8_t *)ds.node_type.ptr;
  ds.node_feat.assign(T, Dataset::NodeFeat{});
  // one pass: the types' sizes and first ids, every node's rank, and whether the types lie one behind the other
  std::vector<uint32_t> rank(ds.num_node);
  std::vector<size_t> seen(T, 0);
  bool sorted = true;
  for (size_t v = 0; v < ds.num_node; ++v) {
    const uint8_t t = nt[v];
    if (seen[t] == 0) ds.node_feat[t].first_node = (uint32_t)v;
    if (v > 0 && t < nt[v - 1]) sorted = false;
    rank[v] = (uint32_t)seen[t]++;
  }
  size_t table_bytes = 0;
  for (size_t t = 0; t < T; ++t) {
    Dataset::NodeFeat &nf = ds.node_feat[t];
    nf.rows = seen[t];
    const std::string ts = std::to_string(t), dim_key = "NODE_FEAT_DIM_" + ts, dt_key = "NODE_FEAT_DATA_TYPE_" + ts;
    if (!meta.count(dim_key))
      fatal(__FILE__, __LINE__, "typed_feat: meta.txt lacks " + dim_key + " (datagen.write_dataset(node_feat=[...]); 0 for a "
                                "type without features)");
    if (!meta_text.count(dt_key))
      fatal(__FILE__, __LINE__, "typed_feat: meta.txt lacks " + dt_key + " (F32, F16 or BF16)");
    nf.dim = meta.at(dim_key);
    const std::string &name = meta_text.at(dt_key);
    if (!kFeatDtypeNames.count(name) || !ggms::is_float_dtype(kFeatDtypeNames.at(name)))
      fatal(__FILE__, __LINE__, "typed_feat with " + dt_key + " = " + name + " is not built: a typed table is F32, F16 or "
                                "BF16; FP8 and Q8ROW typed tables are a follow-up");
    nf.dtype = kFeatDtypeNames.at(name);
    if (nf.dim == 0) continue;
    const std::string file = "node_feat_" + ts + ".bin";
    struct stat st;
    if (stat((cfg.dataset_path + file).c_str(), &st) != 0)
      fatal(__FILE__, __LINE__, "typed_feat: " + cfg.dataset_path + file + " is missing (" + std::to_string(nf.rows) +
                                " rows of " + dim_key + " = " + std::to_string(nf.dim) + " " + name + " elements, one per "
                                "node of type " + ts + " in ascending node id)");
    const size_t want = nf.rows * nf.row_bytes();
    if ((size_t)st.st_size != want)
      fatal(__FILE__, __LINE__, "typed_feat: " + file + " has " + std::to_string((size_t)st.st_size) + " bytes, (nodes of type " +
                                ts + ") x " + dim_key + " x the element size is " + std::to_string(nf.rows) + " x " +
                                std::to_string(nf.dim) + " x " + std::to_string(ggms_dtype_bytes(nf.dtype)) + " = " +
                                std::to_string(want));
    if (want) nf.file = MapFile(file, want, false);
    table_bytes += want;
  }
  if (!sorted) ds.node_rank.swap(rank);
  log_info("typed_feat: " + std::to_string(T) + " tables, " + std::to_string(table_bytes) + " bytes of HBM; " +
           (sorted ? std::string("node_type.bin is non-decreasing in the node id: no rank table (row = node - the type's "
                                 "first id)")
                   : "a rank table of 4 x NUM_NODE = " + std::to_string(4 * ds.num_node) + " bytes is uploaded"));
}

// ------------------------------------------------------------------ device graph (GGMS topology)
static void *dev_upload(const void *host, size_t bytes, hipStream_t s) {
  void *d = nullptr;
  // shards are published to the other workers with hipIpc: sized so that a peer can open them (include/ggms.h)
  SAM_HIP(hipMalloc(&d, ggms_ipc_safe_bytes(std::max<size_t>(bytes, 16))));
  if (bytes) SAM_HIP(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, s));
  return d;
}

static const void *map_host(void *host, size_t bytes) {
  // cudaHostRegister(..., ReadOnly) + zero-copy reads (dist_engine.cc:217-241)
  if (bytes == 0) return nullptr;
  SAM_HIP(hipHostRegister(host, bytes, hipHostRegisterMapped));
  void *d = nullptr;
  SAM_HIP(hipHostGetDevicePointer(&d, host, 0));
  return d;
}

void Engine::UploadGraph() {
  const uint32_t *indptr = (const uint32_t *)ds.indptr.ptr, *indices = (const uint32_t *)ds.indices.ptr;
  std::memset(&graph_, 0, sizeof(graph_));
  graph_.num_node = (uint32_t)ds.num_node;
  if (!cfg.use_dist_graph) { // dist_engine.cc:203-216 / cuda_engine: whole CSR on this GPU
    d_indptr_ = (uint32_t *)dev_upload(indptr, ds.indptr.bytes, stream_);
    d_indices_ = (uint32_t *)dev_upload(indices, ds.indices.bytes, stream_);
    graph_.indptr = d_indptr_;
    graph_.indices = d_indices_;
    SAM_HIP(hipStreamSynchronize(stream_));
    AttachListHeads();
    return;
  }
  // DistGraph::GraphLoad, cuda/dist_graph.cu:309-385
  const uint32_t P = (uint32_t)cfg.num_worker, p = (uint32_t)worker_id_;
  const uint32_t num_cache_edge = (uint32_t)(ds.num_edge * cfg.dist_graph_percentage); // dist_engine.cc:225
  uint32_t num_cache_node = 0;
  while (num_cache_node < ds.num_node && indptr[num_cache_node] < num_cache_edge) ++num_cache_node;
  // _DatasetPartition :228-272: shard p = nodes v == p (mod P), v < num_cache_node
  const size_t isz = num_cache_node / P + (p < num_cache_node % P ? 1 : 0) + 1;
  std::vector<uint32_t> pip(isz);
  size_t ecount = 0;
  for (uint32_t v = p; v < num_cache_node; v += P) ecount += indptr[v + 1] - indptr[v];
  std::vector<uint32_t> pix(std::max<size_t>(ecount, 1));
  uint32_t cnt = 0;
  for (uint32_t v = p; v < num_cache_node; v += P) {
    const uint32_t ne = indptr[v + 1] - indptr[v];
    pip[v / P] = cnt;
    std::memcpy(&pix[cnt], &indices[indptr[v]], ne * 4ull);
    cnt += ne;
  }
  pip[isz - 1] = cnt;
  part_indptr_.assign(P + 1, nullptr);
  part_indices_.assign(P + 1, nullptr);
  part_indptr_[p] = dev_upload(pip.data(), isz * 4, stream_);
  part_indices_[p] = dev_upload(pix.data(), ecount * 4, stream_);
  SAM_HIP(hipStreamSynchronize(stream_));
  // _DataIpcShare :274-307: publish, barrier, open peers, barrier
  if (P > 1) {
    SAM_HIP(hipIpcGetMemHandle(&shared_->graph_indptr[p], part_indptr_[p]));
    SAM_HIP(hipIpcGetMemHandle(&shared_->graph_indices[p], part_indices_[p]));
    shared_->indptr_words[p] = isz;
    shared_->indices_words[p] = ecount;
    Barrier("graph shards published");
    for (uint32_t q = 0; q < P; ++q) {
      if (q == p) continue;
      part_indptr_[q] = OpenPeer(shared_->graph_indptr[q], q, shared_->indptr_words[q] * 4, "graph indptr shard");
      part_indices_[q] = OpenPeer(shared_->graph_indices[q], q, shared_->indices_words[q] * 4, "graph indices shard");
    }
    Barrier("graph shards opened");
  }
  // slot P: the whole CSR, :367-381.  Its neighbour lists stay in (device-mapped) host memory as in the reference; its
  // `indptr` -- 4 B per node, 0.44 GB at papers100M size against 288 GB of HBM -- is kept on the GPU: a seed beyond
  // num_cache_node then pays ONE PCIe round trip (its sampled positions) instead of two dependent ones (list head, then
  // positions), and 40 % fewer PCIe reads per batch.  The layout of slot P is not observable through the interface.
  part_indptr_[P] = dev_upload(ds.indptr.ptr, ds.indptr.bytes, stream_);
  SAM_HIP(hipStreamSynchronize(stream_));
  part_indices_[P] = (void *)map_host(ds.indices.ptr, ds.indices.bytes);
  // the P + 1 pointers stay on the host: ggms_sample_batch hands them to its kernels by value (include/ggms.h)
  SAM_CHECK(P <= GGMS_MAX_PARTS, "use_dist_graph: at most GGMS_MAX_PARTS topology shards");
  graph_.part_indptr = (const ggms_id_t *const *)part_indptr_.data();
  graph_.part_indices = (const ggms_id_t *const *)part_indices_.data();
  graph_.num_part = P;
  graph_.num_cache_node = num_cache_node;
}

// Config key inline_heads: one 64-byte record per node (degree + the whole list up to degree 15, include/ggms.h), built by
// one streaming kernel over the CSR that was just uploaded and attached to graph_; khop3 reads it where it read indptr.
// The CSR is static for the engine's life, so the table is too.  The decision is logged once.
void Engine::AttachListHeads() {
  if (cfg.arch != kArch1 || cfg.inline_heads == 0 || ds.num_node == 0) return;
  const size_t bytes = ggms_list_heads_bytes(ds.num_node);
  if (cfg.inline_heads < 0) {
    if (cfg.sample_type != GGMS_KHOP3) return; // the other samplers do not look at it
    size_t free_b = 0, total_b = 0;
    SAM_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b / 4) {
      std::fprintf(stderr, "[samgraph-amd] inline_heads = auto: not built (%zu bytes needed, %zu free: more than a quarter)\n",
                   bytes, free_b);
      return;
    }
  }
  SAM_HIP(hipMalloc(&d_heads_, bytes));
  SAM_GGMS(ggms_list_heads_build(&graph_, d_heads_, bytes, stream_));
  SAM_HIP(hipStreamSynchronize(stream_));
  SAM_GGMS(ggms_list_heads_attach(&graph_, d_heads_));
  std::fprintf(stderr, "[samgraph-amd] inline_heads = %s: %zu bytes of list heads for %zu nodes attached\n",
               cfg.inline_heads < 0 ? "auto" : "1", bytes, (size_t)ds.num_node);
}

// ------------------------------------------------------------------ init
// the batch bounds every buffer of a batch (and arch5's queue slot) is sized to
void Engine::ComputeBounds() {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  // first batch of arch6 is x1.25 (dist_shuffler_aligned.cc:137-140): size every buffer for it
  max_seeds_ = (size_t)(cfg.batch_size * 1.25) + 1;
  // link_prediction: the seed list is the endpoints and negatives of batch_size positive edges
  if (cfg.link_prediction) max_seeds_ = cfg.batch_size * (2 + cfg.num_negative);
  max_input_.resize(L);
  max_edges_.resize(L);
  SAM_GGMS(ggms_sample_batch_capacity(max_seeds_, cfg.fanout.data(), L, max_input_.data(), max_edges_.data(), &max_unique_));
  if (cfg.arch == kArch4) // the superset: min(N, k + the k largest degrees), within the edge budget
    SAM_GGMS(ggms_sample_batch_prefetch_capacity(max_seeds_, cfg.fanout.data(), L, (const ggms_id_t *)ds.indptr.ptr,
                                                 ds.num_node, cfg.prefetch_max_edges, &max_prefetch_edges_, &max_unique_));
}

void Engine::SampleInit(int worker_id, const std::string &ctx) {
  SAM_CHECK(data_ready_, "samgraph_data_init first");
  if (cfg.arch == kArch5) {
    SAM_CHECK(role_ == kRoleNone, "arch5: a process is one sampler or one trainer (one sample_init or one train_init)");
    SAM_CHECK(worker_id >= 0 && (size_t)worker_id < cfg.num_sample_worker, "arch5: sample_init(worker_id) with 0 <= "
              "worker_id < num_sample_worker = " + std::to_string(cfg.num_sample_worker));
    role_ = kRoleSampler;
  }
  worker_id_ = worker_id;
  device_ = parse_device(ctx);
  trainer_device_ = Dedicated() ? cfg.trainer_device : device_;
  if (trainer_device_ != device_) EnablePeerAccess();
  SAM_HIP(hipSetDevice(device_));
  SAM_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  // the extract streams belong to the trainer GPU (the same device except under arch3): no stream is added for arch3
  // (an arch5 sampler gathers nothing: it has none)
  if (cfg.arch != kArch5) {
    SAM_HIP(hipSetDevice(trainer_device_));
    SAM_HIP(hipStreamCreateWithFlags(&stream_extract_, hipStreamNonBlocking));
    if (cfg.extract_streams > 1) SAM_HIP(hipStreamCreateWithFlags(&stream_extract2_, hipStreamNonBlocking));
    SAM_HIP(hipSetDevice(device_));
  }
  UploadGraph();
  ShufflerInit();
  const uint32_t L = (uint32_t)cfg.fanout.size();
  ComputeBounds();
  // OrderedHashTable(PredictNumNodes(...)) dist_engine.cc:423-424; direct layout by default
  std::memset(&ht_, 0, sizeof(ht_));
  ht_.direct = cfg.direct_table ? 1 : 0;
  ht_.o2n_size = cfg.direct_table ? ds.num_node : ggms_hashtable_num_buckets(max_unique_);
  ht_.n2o_size = max_unique_;
  SAM_HIP(hipMalloc(&ht_.o2n, ht_.o2n_size * (cfg.direct_table ? 8 : 16)));
  SAM_HIP(hipMalloc((void **)&ht_.n2o, max_unique_ * 4));
  SAM_HIP(hipMalloc((void **)&ht_.num_items_dev, 16));
  SAM_GGMS(ggms_hashtable_init(&ht_, stream_));
  std::memset(&extra_, 0, sizeof(extra_));
  if (cfg.sample_type == GGMS_WEIGHTED_KHOP || cfg.sample_type == GGMS_WEIGHTED_KHOP_HASH_DEDUP) { // dist_engine.cc:210-213
    d_prob_ = dev_upload(ds.prob_table.ptr, ds.prob_table.bytes, stream_);
    d_alias_ = dev_upload(ds.alias_table.ptr, ds.alias_table.bytes, stream_);
    extra_.prob_table = (const float *)d_prob_;
    extra_.alias_table = (const ggms_id_t *)d_alias_;
  }
  if (cfg.sample_type == GGMS_WEIGHTED_KHOP_PREFIX) {
    d_prob_ = dev_upload(ds.prob_table.ptr, ds.prob_table.bytes, stream_);
    extra_.prob_table = (const float *)d_prob_;
  }
  extra_.random_walk_length = cfg.random_walk_length;
  extra_.random_walk_restart_prob = cfg.random_walk_restart_prob;
  extra_.num_random_walk = cfg.num_random_walk;
  // GPURandomStates dist_engine.cc:432-433; seed = wall clock unless the "seed" key is given
  if (cfg.sample_type == GGMS_KHOP_LABOR || cfg.Temporal() || cfg.Typed()) { // stateless: their variates are hashes of (node id, salt) -- no RNG pool
    num_states_ = 0;
    states_ = nullptr;
  } else {
    num_states_ = ggms_random_states_count(cfg.sample_type, cfg.fanout.data(), L, max_seeds_, cfg.num_random_walk);
    size_t max_in = 0;
    for (auto v : max_input_) max_in = std::max(max_in, v);
    num_states_ = std::max(num_states_, (max_in + 127) / 128 * 8);
    num_states_ = std::max(num_states_, (max_in + 1023) / 1024 * 256); // khop2: one stream per thread of a 1024-seed tile
    if (cfg.sample_type == GGMS_RANDOM_WALK)
      num_states_ = std::max(num_states_, ggms_random_walk_num_states(max_in, cfg.num_random_walk));
    SAM_HIP(hipMalloc(&states_, num_states_ * GGMS_RNG_STATE_BYTES));
    const uint64_t seed = cfg.has_seed ? cfg.seed + 1000003ull * worker_id
                                       : (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
    SAM_GGMS(ggms_random_states_init(states_, num_states_, seed, stream_));
  }
  ws_bytes_ = cfg.arch == kArch4 ? ggms_sample_batch_prefetch_workspace_bytes(cfg.sample_type, max_seeds_, cfg.fanout.data(),
                                                                          L, &extra_, max_prefetch_edges_)
                                 : ggms_sample_batch_workspace_bytes(cfg.sample_type, max_seeds_, cfg.fanout.data(), L, &extra_);
  if (cfg.Typed()) // the boundary words follow NUM_EDGE_TYPE, which the generic function sizes at its maximum
    ws_bytes_ = ggms_sample_batch_typed_workspace_bytes(max_seeds_, cfg.fanout.data(), L, cfg.num_edge_type, &extra_);
  SAM_HIP(hipMalloc(&ws_, ws_bytes_));
  // pipeline 0 = {stream_, ht_, ws_}; the others get their own stream, table and workspace
  pipes_.assign(cfg.pipelines, Pipe{});
  for (size_t p = 0; p < pipes_.size(); ++p) {
    Pipe &P = pipes_[p];
    SAM_HIP(hipEventCreateWithFlags(&P.rng_done, hipEventDisableTiming));
    if (p == 0) {
      P.stream = stream_;
      P.ht = ht_;
      P.ws = ws_;
      continue;
    }
    SAM_HIP(hipStreamCreateWithFlags(&P.stream, hipStreamNonBlocking));
    P.ht = ht_;
    SAM_HIP(hipMalloc(&P.ht.o2n, ht_.o2n_size * (cfg.direct_table ? 8 : 16)));
    SAM_HIP(hipMalloc((void **)&P.ht.n2o, max_unique_ * 4));
    SAM_HIP(hipMalloc((void **)&P.ht.num_items_dev, 16));
    SAM_GGMS(ggms_hashtable_init(&P.ht, stream_));
    SAM_HIP(hipMalloc(&P.ws, ws_bytes_));
  }
  if (cfg.link_prediction && cfg.exclude_seed_edges) { // the edge filter's workspace, one per pipeline
    drop_ws_bytes_ = ggms_drop_pair_edges_workspace_bytes(cfg.batch_size, max_edges_.data(), L);
    SAM_CHECK(drop_ws_bytes_ > 0, "exclude_seed_edges: the batch bounds are out of ggms_drop_pair_edges' range");
    for (Pipe &P : pipes_) SAM_HIP(hipMalloc(&P.drop_ws, drop_ws_bytes_));
  }
  if (cfg.Temporal()) { // one cut table per pipeline: 8 B x num_node, zeroed once; stamps 1, 2, 3, ... per batch
    for (Pipe &P : pipes_) {
      SAM_HIP(hipMalloc((void **)&P.cut_table, std::max<size_t>(ds.num_node, 1) * 8));
      SAM_HIP(hipMemsetAsync(P.cut_table, 0, std::max<size_t>(ds.num_node, 1) * 8, stream_));
    }
  }
  if (cfg.Typed()) { // the edge types in HBM, beside the topology the sampler reads
    SAM_HIP(hipMalloc((void **)&d_edge_type_, std::max<size_t>(ds.num_edge, 16)));
    SAM_HIP(hipMemcpyAsync(d_edge_type_, ds.edge_type.ptr, ds.num_edge, hipMemcpyHostToDevice, stream_));
    SAM_HIP(hipStreamSynchronize(stream_));
  }
  if (cfg.edge_ids && !cfg.SamplerEmitsEdgeIds()) { // the long-list queue of ggms_edge_positions, one per pipeline
    eid_ws_bytes_ = ggms_edge_positions_workspace_bytes(max_edges_.data(), L);
    SAM_CHECK(eid_ws_bytes_ > 0, "edge_ids: the batch bounds are out of ggms_edge_positions' range");
    for (Pipe &P : pipes_) SAM_HIP(hipMalloc(&P.eid_ws, eid_ws_bytes_));
  }
  if (cfg.hetero) { // the node types in HBM; one workspace per pipeline, shared by the two calls (they follow each other)
    SAM_HIP(hipMalloc((void **)&d_node_type_, std::max<size_t>(ds.num_node, 16)));
    SAM_HIP(hipMemcpyAsync(d_node_type_, ds.node_type.ptr, ds.num_node, hipMemcpyHostToDevice, stream_));
    SAM_HIP(hipStreamSynchronize(stream_));
    hetero_ws_bytes_ = std::max(ggms_hetero_nodes_workspace_bytes(max_unique_, ds.num_node_type),
                                ggms_hetero_edges_workspace_bytes(max_edges_.data(), L, cfg.num_edge_type));
    SAM_CHECK(ggms_hetero_nodes_workspace_bytes(max_unique_, ds.num_node_type) > 0 &&
                  ggms_hetero_edges_workspace_bytes(max_edges_.data(), L, cfg.num_edge_type) > 0,
              "hetero_batch: the batch bounds are out of ggms_hetero_nodes' / ggms_hetero_edges' range");
    for (Pipe &P : pipes_) SAM_HIP(hipMalloc(&P.hetero_ws, hetero_ws_bytes_));
  }
  if (cfg.induced) { // one membership map (4 B x num_node, filled once: every call restores it) and one workspace per pipeline
    induced_ws_bytes_ = ggms_induced_edges_workspace_bytes(max_unique_, ds.num_edge);
    for (Pipe &P : pipes_) {
      SAM_HIP(hipMalloc((void **)&P.induced_map, std::max<size_t>(ds.num_node, 1) * 4));
      SAM_GGMS(ggms_induced_map_init(P.induced_map, ds.num_node, stream_));
      SAM_HIP(hipMalloc(&P.induced_ws, induced_ws_bytes_));
    }
  }
  SAM_HIP(hipStreamSynchronize(stream_));
  prof.Resize(cfg.num_epoch, num_global_step_);
  if (cfg.UsePresample()) { // dist_engine.cc:455-466: worker 0 ranks the nodes, everybody waits
    auto t0 = std::chrono::steady_clock::now();
    if (worker_id_ == 0) Presample();
    if (cfg.arch == kArch5) { // sampler 0 publishes the ranking (shared pages); the other samplers wait for it
      if (worker_id_ == 0) PublishRanking();
      else WaitRankingReady();
    } else {
      Barrier("presample ranking");
    }
    prof.LogInit(/*kLogInitL2Presample*/ 8, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  if (cfg.arch == kArch5) { // the sampler's own batch buffers: it samples into them and packs them into a queue slot
    sbatch_ = std::make_unique<Batch>();
    Batch *b = sbatch_.get();
    b->sampler.Alloc(max_edges_, max_unique_, max_seeds_, cfg.sample_type == GGMS_RANDOM_WALK);
    SAM_HIP(hipEventCreateWithFlags(&b->ev_sampled, hipEventDisableTiming));
    SAM_HIP(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
    QueueMap();
  }
  sample_ready_ = true;
}

// arch3 with two distinct GPUs: the hand-off kernel runs on the trainer GPU T and reads the sampler GPU S's memory in
// place (ggms_batch_handoff), so T must reach S.  A pair that cannot is refused here, named -- there is no fallback.
void Engine::EnablePeerAccess() {
  int can = 0;
  SAM_HIP(hipDeviceCanAccessPeer(&can, trainer_device_, device_));
  if (!can)
    fatal(__FILE__, __LINE__, "arch3: GPU " + std::to_string(trainer_device_) + " (trainer_ctx) cannot access GPU " +
                                  std::to_string(device_) + " (sampler_ctx) (hipDeviceCanAccessPeer): the trainer GPU "
                                  "reads each sampled batch from the sampler GPU's memory, which needs peer access");
  SAM_HIP(hipSetDevice(trainer_device_));
  const hipError_t e = hipDeviceEnablePeerAccess(device_, 0);
  if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
  else SAM_HIP(e);
  SAM_HIP(hipSetDevice(device_));
  log_info("arch3: peer access GPU " + std::to_string(trainer_device_) + " -> GPU " + std::to_string(device_) + " enabled");
}

// PreSampler (dist/pre_sampler.cc:39-139): sample `presample_epoch` epochs of the WHOLE train set with a
// GPUShuffler of its own, count how often each node is an input node, rank by (freq << 32 | id) descending.
// Counting happens on the device (one atomicAdd per input node) instead of D2H copy + OpenMP loop.
// presample_static (GPUEngine's pre-sampler, cuda/pre_sampler.cc:58-111): the same epochs, but a batch counts its
// whole L-hop closure (ggms_khop_closure, each node once per batch) instead of its sampled input nodes; no RNG state
// is consumed, so the training batches that follow are those of a run without presample.
void Engine::Presample() {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  const size_t n_train = ds.num_train;
  const size_t steps = (n_train + cfg.batch_size - 1) / cfg.batch_size; // drop_last = false, :41-42
  const bool closure = cfg.cache_policy == 4 /*kCacheByPreSampleStatic*/;
  std::vector<uint32_t> data((const uint32_t *)ds.train_set.ptr, (const uint32_t *)ds.train_set.ptr + n_train);
  uint32_t *d_train = nullptr, *d_freq = nullptr;
  uint64_t *d_counts = nullptr;
  SAM_HIP(hipMalloc((void **)&d_train, std::max<size_t>(n_train, 1) * 4));
  SAM_HIP(hipMalloc((void **)&d_freq, ds.num_node * 4));
  SAM_HIP(hipMalloc((void **)&d_counts, CountsBytes(L)));
  SAM_HIP(hipMemsetAsync(d_freq, 0, ds.num_node * 4, stream_));
  // presample_static: visit stamps + the closure + its workspace, about 3 x 4 B x num_node, freed before BuildCache
  uint32_t *d_visit = nullptr, *d_closure = nullptr;
  void *d_cws = nullptr;
  const size_t cws_bytes = closure ? ggms_khop_closure_workspace_bytes(ds.num_node) : 0;
  if (closure) {
    SAM_HIP(hipMalloc((void **)&d_visit, ds.num_node * 4));
    SAM_HIP(hipMalloc((void **)&d_closure, ds.num_node * 4));
    SAM_HIP(hipMalloc(&d_cws, cws_bytes));
    SAM_HIP(hipMemsetAsync(d_visit, 0, ds.num_node * 4, stream_));
  }
  std::vector<uint32_t *> row(closure ? 0 : L), col(closure ? 0 : L), dat(closure ? 0 : L, nullptr);
  for (uint32_t i = 0; i < row.size(); ++i) {
    SAM_HIP(hipMalloc((void **)&row[i], std::max<size_t>(max_edges_[i], 4) * 4));
    SAM_HIP(hipMalloc((void **)&col[i], std::max<size_t>(max_edges_[i], 4) * 4));
    if (cfg.sample_type == GGMS_RANDOM_WALK) SAM_HIP(hipMalloc((void **)&dat[i], std::max<size_t>(max_edges_[i], 4) * 4));
  }
  uint32_t stamp = 0; // closure k of the presample: stamp k, so `visit` is zeroed once
  for (size_t e = 0; e < cfg.presample_epoch; ++e) {
    const uint64_t seed = cfg.has_seed ? cfg.seed + 0x5a5a5aull + e
                                       : (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
    auto g = std::default_random_engine(seed); // GPUShuffler::ReShuffle, cuda_shuffler.cc:89-110
    for (size_t i = 0; n_train && i < n_train - 1; i++) {
      std::uniform_int_distribution<size_t> d(i, n_train - 1);
      std::swap(data[i], data[d(g)]);
    }
    SAM_HIP(hipMemcpyAsync(d_train, data.data(), n_train * 4, hipMemcpyHostToDevice, stream_));
    for (size_t s = 0; s < steps; ++s) {
      const size_t off = s * cfg.batch_size, size = std::min(cfg.batch_size, n_train - off);
      if (closure) { // DoGPUSampleAllNeighbour + the count (cuda/pre_sampler.cc:58-111); the hop offsets go to d_counts
        SAM_GGMS(ggms_khop_closure(&graph_, d_train + off, size, L, d_visit, ++stamp, d_freq, d_closure, d_counts, d_cws,
                                   cws_bytes, stream_));
        continue;
      }
      ggms_sample_extra_t extra = extra_;
      extra.data = dat.data();
      extra.seeds_distinct = train_distinct_ ? 1u : 0u; // slices of a permutation of the train set
      extra.labor_salt = ggms::labor_batch_salt(cfg.labor_seed, e, s); // the training rule, on the presample's own epochs
      // pipeline 0's table: its version stamp keeps counting when the training batches follow
      SAM_GGMS(ggms_sample_batch(cfg.sample_type, &graph_, d_train + off, size, cfg.fanout.data(), L, &pipes_[0].ht,
                                 states_, num_states_, row.data(), col.data(), d_counts, &extra, ws_, ws_bytes_, stream_));
      SAM_GGMS(ggms_count_nodes(d_freq, pipes_[0].ht.n2o, max_unique_, d_counts + GGMS_COUNT_INPUT(L), stream_));
    }
    SAM_HIP(hipStreamSynchronize(stream_)); // `data` is reshuffled on the host next
  }
  if (closure) { // the closures' scans report a bound they hit in the device's status word
    uint32_t st = 0;
    SAM_GGMS(ggms_device_status(&st, 1));
    SAM_CHECK(st == 0, "presample_static: a closure's scan reported device status " + std::to_string(st));
    (void)hipFree(d_visit); (void)hipFree(d_closure); (void)hipFree(d_cws);
  }
  std::vector<uint32_t> freq(ds.num_node);
  SAM_HIP(hipMemcpy(freq.data(), d_freq, ds.num_node * 4, hipMemcpyDeviceToHost));
  std::vector<uint64_t> keys(ds.num_node);
  for (size_t i = 0; i < ds.num_node; ++i) keys[i] = ((uint64_t)freq[i] << 32) | (uint64_t)i; // :45-50
  std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());                            // :113-119
  uint32_t *rank = (uint32_t *)ds.ranking_nodes.ptr;
  for (size_t i = 0; i < ds.num_node; ++i) rank[i] = (uint32_t)keys[i]; // GetRankNode :141-151
  for (size_t i = 0; i < row.size(); ++i) { (void)hipFree(row[i]); (void)hipFree(col[i]); if (dat[i]) (void)hipFree(dat[i]); }
  (void)hipFree(d_train); (void)hipFree(d_freq); (void)hipFree(d_counts);
}

// Config key feat_store_dtype: the table of the dataset (F32 or F16, a mapped file) is encoded into the store type by
// the trainer GPU, 64 MB-class chunks through two sets of pinned staging buffers -- the host cores fill one while the
// GPU works on the other -- and lands in an anonymous host table that takes the place of ds.feat.  After this the
// dataset is what a meta.txt naming the store type would have loaded; BuildCache and everything behind it see no
// difference.
void Engine::QuantizeStore() {
  const auto t0 = std::chrono::steady_clock::now();
  const int store = cfg.feat_store_dtype;
  const size_t src_row = ds.feat_row_bytes(), dst_row = ggms_row_bytes(store, ds.feat_dim), n = ds.num_node;
  hipStream_t bs = BatchSampledElsewhere() ? stream_extract_ : stream_;
  HostArray q;
  q.bytes = n * dst_row;
  q.ptr = mmap(nullptr, std::max<size_t>(q.bytes, 1), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  SAM_CHECK(q.ptr != MAP_FAILED, "feat_store_dtype: mmap of the quantised table failed");
  q.shared_anon = true;
  const size_t step = std::max<size_t>(1, (64u << 20) / src_row);
  char *in[2], *out[2], *d_in[2], *d_out[2];
  hipEvent_t done[2];
  size_t first[2] = {0, 0}, rows[2] = {0, 0}; // the chunk whose codes out[k] receives
  for (int k = 0; k < 2; ++k) {
    SAM_HIP(hipHostMalloc((void **)&in[k], step * src_row));
    SAM_HIP(hipHostMalloc((void **)&out[k], step * dst_row));
    SAM_HIP(hipMalloc((void **)&d_in[k], step * src_row));
    SAM_HIP(hipMalloc((void **)&d_out[k], step * dst_row));
    SAM_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
  }
  uint64_t *d_bad = nullptr, bad = ~0ull;
  SAM_HIP(hipMalloc((void **)&d_bad, sizeof(uint64_t)));
  SAM_HIP(hipMemcpyAsync(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice, bs));
  SAM_HIP(hipStreamSynchronize(bs));
  Team team((int)std::max<size_t>(1, cfg.omp_thread_num));
  const char *feat = (const char *)ds.feat.ptr;
  auto collect = [&](int k) { // chunk in out[k] -> its place in the new table
    SAM_HIP(hipEventSynchronize(done[k]));
    std::memcpy((char *)q.ptr + first[k] * dst_row, out[k], rows[k] * dst_row);
    rows[k] = 0;
  };
  size_t c = 0;
  for (size_t lo = 0; lo < n; lo += step, ++c) {
    const int k = (int)(c & 1);
    const size_t m = std::min(step, n - lo);
    if (rows[k]) collect(k); // (also: the copy that last read in[k] is done)
    team.ParallelFor(m, [&](size_t a, size_t b, int) { std::memcpy(in[k] + a * src_row, feat + (lo + a) * src_row, (b - a) * src_row); });
    SAM_HIP(hipMemcpyAsync(d_in[k], in[k], m * src_row, hipMemcpyHostToDevice, bs));
    SAM_GGMS(ggms_quantize_rows(d_out[k], store, d_in[k], ds.feat_dtype, m, ds.feat_dim, lo, d_bad, bs));
    SAM_HIP(hipMemcpyAsync(out[k], d_out[k], m * dst_row, hipMemcpyDeviceToHost, bs));
    SAM_HIP(hipEventRecord(done[k], bs));
    first[k] = lo;
    rows[k] = m;
  }
  for (int k = 0; k < 2; ++k)
    if (rows[(c + k) & 1]) collect((int)((c + k) & 1)); // the older chunk first
  SAM_HIP(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; ++k) {
    (void)hipHostFree(in[k]); (void)hipHostFree(out[k]); (void)hipFree(d_in[k]); (void)hipFree(d_out[k]);
    (void)hipEventDestroy(done[k]);
  }
  (void)hipFree(d_bad);
  if (bad != ~0ull)
    fatal(__FILE__, __LINE__, "feat_store_dtype = Q8ROW: row " + std::to_string(bad) + " of feat.bin holds NaN or inf: a "
                              "row-scaled table has no code for either");
  const size_t before = ds.feat.bytes;
  if (ds.feat.ptr && ds.feat.bytes) munmap(ds.feat.ptr, ds.feat.bytes); // the mapped file (arch1 / arch3 / arch4: never shared)
  ds.feat = q;
  ds.feat_dtype = store;
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  prof.LogInit(/*extension slot: quantise the feature store*/ 41, s);
  std::fprintf(stderr, "[samgraph-amd] feat_store_dtype = %s: feature table quantised on GPU %d in %.3f s, %zu -> %zu bytes\n",
               cfg.raw["feat_store_dtype"].c_str(), trainer_device_, s, before, q.bytes);
}

void Engine::BuildCache() {
  const size_t row_bytes = ds.feat_row_bytes();
  const char *feat = (const char *)ds.feat.ptr;
  // the cache and the label table live on the trainer GPU: uploaded through a stream of that device (arch3: the
  // extract stream; the other deployments have one device, and the sampling stream as before)
  hipStream_t bs = BatchSampledElsewhere() ? stream_extract_ : stream_;
  // labels are 8 B x N: always resident on the device (the reference keeps them on the host and
  // gathers through zero-copy in gpu_extract mode, dist_loops.cc:938-974)
  label_src_ = dev_upload(ds.label.ptr, ds.label.bytes, bs);
  if (!cfg.UseGPUCache()) {
    if (cfg.arch == kArch6 && !cfg.gpu_extract) {
      // cache 0 without gpu_extract: the table stays in host memory and every row takes the host-staged path
      // (DoIdCopy + DoCPUFeatureExtract + DoFeatureCopy, dist_loops_arch6.cc:111-133; StagedExtract)
      feat_src_ = nullptr;
    } else if (cfg.arch == kArch1) {
      // arch1: the whole table lives in HBM and is gathered directly (cuda_loops_arch1.cc:61)
      if (cfg.typed_feat) { // one table per node type in place of the one table, and the rank table where one is needed
        const size_t T = ds.num_node_type;
        d_node_feat_.assign(T, nullptr);
        typed_tables_.assign(T, ggms_typed_table_t{});
        for (size_t t = 0; t < T; ++t) {
          const Dataset::NodeFeat &nf = ds.node_feat[t];
          // (a type that has a width but no node: dev_upload of 0 bytes is still an allocation, so the leaf gets a table
          // base and 0 rows -- every rank lies beyond it -- and not the null pointer it refuses)
          if (nf.dim) d_node_feat_[t] = dev_upload(nf.file.ptr, nf.file.bytes, bs);
          typed_tables_[t] = ggms_typed_table_t{d_node_feat_[t], nf.rows, (uint32_t)nf.dim, nf.dtype,
                                                typed_feat_dtype(t), nf.first_node};
        }
        if (!ds.node_rank.empty()) d_node_rank_ = (uint32_t *)dev_upload(ds.node_rank.data(), ds.node_rank.size() * 4, bs);
      } else {
        d_feat_ = dev_upload(feat, ds.feat.bytes, bs);
        feat_src_ = d_feat_;
      }
      if (cfg.edge_feat) d_edge_feat_ = dev_upload(ds.edge_feat.ptr, ds.edge_feat.bytes, bs); // the edge table, beside it
      if (cfg.Temporal()) d_edge_time_ = (uint32_t *)dev_upload(ds.edge_time.ptr, ds.edge_time.bytes, bs); // and the times
      if (cfg.feat_learnable >= 0) { // the upload is the learnable table's initial value; Adagrad's accumulator starts at 0
        if (cfg.feat_learnable == GGMS_UPDATE_ADAGRAD) {
          SAM_HIP(hipMalloc(&d_feat_state_, std::max<size_t>(ds.feat.bytes, 16)));
          SAM_HIP(hipMemsetAsync(d_feat_state_, 0, ds.feat.bytes, bs));
        }
        SAM_HIP(hipEventCreateWithFlags(&ev_grad_, hipEventDisableTiming));
        SAM_HIP(hipEventCreateWithFlags(&ev_updated_, hipEventDisableTiming));
      }
    } else {
      feat_src_ = map_host(ds.feat.ptr, ds.feat.bytes); // cache 0 %: DoGPUFeatureExtract from host, dist_loops.cc:585-634
    }
    SAM_HIP(hipStreamSynchronize(bs));
    return;
  }
  // GPUCacheManager ctor: cuda_cache_manager_host.cc:61-130 (replicated) / :133-254 (partition)
  const uint32_t *rank_in = (const uint32_t *)ds.ranking_nodes.ptr;
  num_cached_nodes_ = (size_t)(ds.num_node * cfg.cache_percentage);
  std::vector<uint32_t> rank(rank_in, rank_in + ds.num_node);
  const uint32_t P = cfg.part_cache ? (uint32_t)cfg.num_worker : 1, p = cfg.part_cache ? (uint32_t)worker_id_ : 0;
  // hybrid store: slots [0, R) = the hottest cached nodes, a copy on every GPU; slots [R, num_cached) sharded
  num_replica_ = cfg.part_cache ? (size_t)(num_cached_nodes_ * cfg.replicate_percentage) : 0;
  SAM_CHECK(num_replica_ == 0 || cfg.gpu_extract, "replicate_percentage needs gpu_extract (one fused gather over all tiers)");
  const size_t R = num_replica_;
  if (cfg.part_cache) { // load balance across shards: :169-171 (the replicated prefix keeps its rank order)
    std::mt19937 eg((uint32_t)num_cached_nodes_);
    std::shuffle(rank.begin() + R, rank.begin() + num_cached_nodes_, eg);
  }
  // Everything cached (cache_percentage 1.0; 288 GB of HBM hold every BASELINE feature table): rows stay in NODE
  // order, slot = node id -- no id -> slot table and no table read per gathered row (ggms_extract_cached with
  // table == NULL).  The reference ranks and shuffles even then; the layout is not observable through its interface.
  const bool full_cache = num_cached_nodes_ == ds.num_node && R == 0;
  if (full_cache) {
    for (size_t i = 0; i < ds.num_node; ++i) rank[i] = (uint32_t)i;
    cache_table_ = nullptr;
  } else {
    std::vector<uint32_t> table(ds.num_node, GGMS_EMPTY_KEY);
    for (size_t i = 0; i < num_cached_nodes_; ++i) table[rank[i]] = (uint32_t)i; // :197-229
    cache_table_ = (uint32_t *)dev_upload(table.data(), ds.num_node * 4, bs);
  }
  // Rows are staged through a bounded host buffer (64 MB at a time), never through a host copy of the whole replica
  // or shard: at papers100M size a replica is 46 GB, and eight workers of one node would hold eight of them at once.
  // ... gathered by the host team (omp_thread_num threads) into TWO pinned buffers: the cores fill one while the copy
  // engine drains the other (one thread and one pageable buffer took a minute per 46-GB replica).
  Team team((int)std::max<size_t>(1, cfg.omp_thread_num));
  const size_t step = std::max<size_t>(1, (64u << 20) / row_bytes);
  char *stage[2] = {nullptr, nullptr};
  hipEvent_t drained[2];
  for (int k = 0; k < 2; ++k) {
    SAM_HIP(hipHostMalloc((void **)&stage[k], step * row_bytes + 16));
    SAM_HIP(hipEventCreateWithFlags(&drained[k], hipEventDisableTiming));
  }
  auto upload_rows = [&](size_t first, size_t stride, size_t count) -> void * {
    void *d = nullptr;
    // shards are published to the other workers with hipIpc: sized so that a peer can open them (include/ggms.h)
    SAM_HIP(hipMalloc(&d, ggms_ipc_safe_bytes(std::max<size_t>(count * row_bytes, 16))));
    if (ds.feat_is_zero) {
      // rows of a table that is known to be all zero need no gather: touching them in rank order would fault in every
      // page of the untouched anonymous mapping once per worker (two minutes of page faults at papers100M size)
      SAM_HIP(hipMemsetAsync(d, 0, count * row_bytes, bs));
      SAM_HIP(hipStreamSynchronize(bs));
      return d;
    }
    size_t k = 0;
    for (size_t lo = 0; lo < count; lo += step, ++k) {
      const size_t m = std::min(step, count - lo);
      char *buf = stage[k & 1];
      if (k >= 2) SAM_HIP(hipEventSynchronize(drained[k & 1])); // the copy that last read this buffer is done
      team.ParallelFor(m, [&](size_t a, size_t b, int) {
        for (size_t i = a; i < b; ++i)
          std::memcpy(buf + i * row_bytes, feat + (size_t)(rank[first + (lo + i) * stride] & ds.feat_mask) * row_bytes, row_bytes);
      });
      SAM_HIP(hipMemcpyAsync((char *)d + lo * row_bytes, buf, m * row_bytes, hipMemcpyHostToDevice, bs));
      SAM_HIP(hipEventRecord(drained[k & 1], bs));
    }
    SAM_HIP(hipStreamSynchronize(bs));
    return d;
  };
  if (R) d_replica_ = upload_rows(0, 1, R); // this GPU's copy of the hottest rows
  // DistGraph::FeatureLoad / _PartitionFeature, dist_graph.cu:493-521: rows rank[i], (i - R) == p (mod P)
  const size_t sharded = num_cached_nodes_ - R;
  const size_t my_rows = sharded / P + (p < sharded % P ? 1 : 0);
  cache_parts_.assign(P, nullptr);
  cache_parts_[p] = upload_rows(R + p, P, my_rows);
  SAM_HIP(hipStreamSynchronize(bs));
  if (P > 1) { // _DataIpcShare
    SAM_HIP(hipIpcGetMemHandle(&shared_->feat_part[p], cache_parts_[p]));
    shared_->feat_rows[p] = my_rows;
    Barrier("feature shards published");
    for (uint32_t q = 0; q < P; ++q)
      if (q != p) cache_parts_[q] = OpenPeer(shared_->feat_part[q], q, shared_->feat_rows[q] * row_bytes, "feature shard");
    Barrier("feature shards opened");
  }
  SAM_CHECK(P <= GGMS_MAX_PARTS, "part_cache: at most GGMS_MAX_PARTS feature shards");
  num_cache_part_ = cfg.part_cache ? P : 0;
  for (int k = 0; k < 2; ++k) {
    (void)hipHostFree(stage[k]);
    (void)hipEventDestroy(drained[k]);
  }
  // miss tier: pinned host memory read by the gather kernel itself (GPUExtractMissData, :573-625); the host-staged
  // path (`gpu_extract` off) reads the table with the host cores instead and needs no device mapping of it
  // (arch3 and arch5 gather their misses the gpu_extract way: zero-copy by the trainer GPU, no CPU-staged path)
  const bool host_tier =
      cfg.gpu_extract || (BatchSampledElsewhere() && (num_cached_nodes_ < ds.num_node || ds.feat_mask != 0xffffffffu));
  feat_src_ = host_tier ? map_host(ds.feat.ptr, ds.feat.bytes) : nullptr;
  SAM_HIP(hipStreamSynchronize(bs));
}

void BatchArrays::Alloc(const std::vector<size_t> &max_edges, size_t max_unique, size_t max_seeds, bool with_data) {
  const size_t L = max_edges.size();
  row.resize(L); col.resize(L); data.assign(L, nullptr);
  for (size_t i = 0; i < L; ++i) {
    SAM_HIP(hipMalloc((void **)&row[i], std::max<size_t>(max_edges[i], 4) * 4));
    SAM_HIP(hipMalloc((void **)&col[i], std::max<size_t>(max_edges[i], 4) * 4));
    if (with_data) SAM_HIP(hipMalloc((void **)&data[i], std::max<size_t>(max_edges[i], 4) * 4));
  }
  SAM_HIP(hipMalloc((void **)&input_nodes, max_unique * 4));
  SAM_HIP(hipMalloc((void **)&output_nodes, max_seeds * 4));
  SAM_HIP(hipMalloc((void **)&counts_dev, CountsBytes(L)));
  SAM_HIP(hipMemset(counts_dev, 0, CountsBytes(L)));
}

ggms_queue_batch_t BatchArrays::View() const {
  SAM_CHECK(row.size() <= GGMS_QUEUE_MAX_LAYERS, "at most GGMS_QUEUE_MAX_LAYERS layers");
  ggms_queue_batch_t v{};
  for (size_t i = 0; i < row.size(); ++i) {
    v.row[i] = row[i];
    v.col[i] = col[i];
    v.data[i] = data[i];
  }
  v.input_nodes = input_nodes;
  v.output_nodes = output_nodes;
  v.counts = counts_dev;
  return v;
}

void Engine::TrainInit(int worker_id, const std::string &ctx) {
  if (cfg.arch == kArch5)
    Arch5TrainerInit(worker_id, ctx);
  else
    SAM_CHECK(sample_ready_, "samgraph_sample_init first");
  if (Dedicated())
    SAM_CHECK(parse_device(ctx) == trainer_device_, "arch3 / arch4: train_init on the config's trainer_ctx");
  else
    SAM_CHECK(parse_device(ctx) == device_, "arch6: sampler and trainer share the GPU (cuda_cache_manager_host.cc:152-155)");
  SAM_HIP(hipSetDevice(trainer_device_));
  if (cfg.feat_store_dtype >= 0) QuantizeStore();
  auto t0 = std::chrono::steady_clock::now();
  BuildCache();
  prof.LogInit(/*kLogInitL2BuildCache*/ 10, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (getenv("SAMGRAPH_LOG_NODE_ACCESS") || getenv("SAMGRAPH_LOG_NODE_ACCESS_SIMPLE")) { // run_config.cc:118-124
    SAM_HIP(hipMalloc((void **)&node_access_dev_, ds.num_node * 4));
    SAM_HIP(hipMemset(node_access_dev_, 0, ds.num_node * 4));
  }
  // batch slots (GraphPool(max_copying_jobs), cuda_engine.cc:151): buffers sized once at their bounds
  const uint32_t L = (uint32_t)cfg.fanout.size();
  const size_t row_bytes = ds.feat_row_bytes();
  size_t nslots = 2;
  if (cfg.raw.count("max_copying_jobs")) nslots = std::max<size_t>(2, std::min<size_t>(4, std::stoull(cfg.raw["max_copying_jobs"]) + 1));
  nslots = std::max(nslots, 2 + cfg.lookahead); // the trainer's batch + the one asked for + the ones enqueued ahead
  if (cfg.dynamic_cache) { // + the previous batch, held until the next gather has read its rows (dyn_hold)
    nslots += 1;
    SAM_CHECK(ds.feat_mask == 0xffffffffu, "arch4: dynamic_cache with SAMGRAPH_EMPTY_FEAT (a mock feature table) is not built");
    SAM_HIP(hipMalloc((void **)&dyn_stamps_, std::max<size_t>(ds.num_node, 1) * 8));
    SAM_GGMS(ggms_dynamic_cache_reset(dyn_stamps_, ds.num_node, stream_extract_));
    SAM_HIP(hipStreamSynchronize(stream_extract_));
  }
  for (size_t s = 0; s < nslots; ++s) {
    auto b = std::make_unique<Batch>();
    b->slot = (int)s;
    b->trainer.Alloc(max_edges_, max_unique_, max_seeds_, cfg.sample_type == GGMS_RANDOM_WALK);
    if (cfg.typed_feat) { // per-type blocks, every one 16-byte aligned; the T + 1 offsets and their host copy
      typed_feat_bytes_ = ggms_gather_typed_out_bytes(typed_tables_.data(), ds.num_node_type, max_unique_);
      SAM_CHECK(typed_feat_bytes_ > 0, "typed_feat: the batch bound is out of ggms_gather_typed's range");
      SAM_HIP(hipMalloc(&b->feat, typed_feat_bytes_));
      SAM_HIP(hipMalloc((void **)&b->het_off_dev, (ds.num_node_type + 1) * 8));
      SAM_HIP(hipMemset(b->het_off_dev, 0, (ds.num_node_type + 1) * 8));
      SAM_HIP(hipHostMalloc((void **)&b->het_off, (ds.num_node_type + 1) * 8));
      std::memset(b->het_off, 0, (ds.num_node_type + 1) * 8);
    } else {
      SAM_HIP(hipMalloc(&b->feat, max_unique_ * batch_feat_row_bytes())); // rows as delivered
    }
    SAM_HIP(hipMalloc((void **)&b->label, max_seeds_ * 8));
    if (cfg.link_prediction) {
      SAM_HIP(hipMalloc((void **)&b->edge_ids, cfg.batch_size * 4));
      SAM_HIP(hipMalloc((void **)&b->seed_ids, max_seeds_ * 4));
      if (cfg.exclude_seed_edges) { // the dropped count of every layer: its own words, not counts words
        SAM_HIP(hipMalloc((void **)&b->excluded_dev, L * 8));
        SAM_HIP(hipHostMalloc((void **)&b->excluded, L * 8));
        std::memset(b->excluded, 0, L * 8);
      }
    }
    if (cfg.edge_ids) { // per layer: the edges' CSR positions and, with edge_feat, the edge table's rows under them
      b->eid.assign(L, nullptr);
      b->efeat.assign(L, nullptr);
      for (uint32_t i = 0; i < L; ++i) {
        SAM_HIP(hipMalloc((void **)&b->eid[i], std::max<size_t>(max_edges_[i], 4) * 4));
        if (cfg.edge_feat) SAM_HIP(hipMalloc(&b->efeat[i], std::max<size_t>(max_edges_[i] * ds.edge_feat_row_bytes(), 16)));
      }
    }
    if (cfg.induced) { // the induced COO, its positions, with edge_feat its rows; the count words and their host copy
      const size_t cap = std::max<size_t>(induced_max_edges_, 4);
      for (uint32_t **p : {&b->ind_row, &b->ind_col, &b->ind_eid}) {
        SAM_HIP(hipMalloc((void **)p, cap * 4));
        SAM_HIP(hipMemset(*p, 0, cap * 4));
      }
      if (cfg.edge_feat) SAM_HIP(hipMalloc(&b->ind_efeat, std::max<size_t>(cap * ds.edge_feat_row_bytes(), 16)));
      SAM_HIP(hipMalloc((void **)&b->ind_counts_dev, 4 * 8));
      SAM_HIP(hipMemset(b->ind_counts_dev, 0, 4 * 8));
      SAM_HIP(hipHostMalloc((void **)&b->ind_counts, 2 * 8));
      std::memset(b->ind_counts, 0, 2 * 8);
    }
    if (cfg.hetero) { // the typed view: four node arrays, three arrays per layer, the small words and their host copy
      const size_t nu = std::max<size_t>(max_unique_, 4);
      SAM_HIP(hipMalloc((void **)&b->het_ntype, std::max<size_t>(nu, 16)));
      for (uint32_t **p : {&b->het_local, &b->het_slot, &b->het_typed}) SAM_HIP(hipMalloc((void **)p, nu * 4));
      b->het_row.assign(L, nullptr);
      b->het_col.assign(L, nullptr);
      b->het_eid.assign(L, nullptr);
      for (uint32_t i = 0; i < L; ++i)
        for (uint32_t **p : {&b->het_row[i], &b->het_col[i], &b->het_eid[i]})
          SAM_HIP(hipMalloc((void **)p, std::max<size_t>(max_edges_[i], 4) * 4));
      SAM_HIP(hipMalloc((void **)&b->het_words_dev, HetWords() * 4));
      SAM_HIP(hipMemset(b->het_words_dev, 0, HetWords() * 4));
      SAM_HIP(hipHostMalloc((void **)&b->het_words, HetWords() * 4));
      std::memset(b->het_words, 0, HetWords() * 4);
    }
    if (cfg.Temporal()) {
      SAM_HIP(hipMalloc((void **)&b->seed_time, std::max<size_t>(max_seeds_, 4) * 4));
      SAM_HIP(hipMalloc((void **)&b->node_cut, std::max<size_t>(max_unique_, 4) * 4));
      b->etime.assign(L, nullptr);
      for (uint32_t i = 0; i < L; ++i) SAM_HIP(hipMalloc((void **)&b->etime[i], std::max<size_t>(max_edges_[i], 4) * 4));
    }
    if (cfg.Typed()) {
      b->etype.assign(L, nullptr);
      for (uint32_t i = 0; i < L; ++i) SAM_HIP(hipMalloc((void **)&b->etype[i], std::max<size_t>(max_edges_[i], 16)));
    }
    if (StagedHostTier()) { // index arrays of GetMissCacheIndex + pinned / device staging of the miss rows
      if (cache_table_) { // (no cache: no split, and the rows land in the batch's feature buffer directly)
        for (uint32_t **p : {&b->miss_src, &b->miss_dst, &b->hit_src, &b->hit_dst}) SAM_HIP(hipMalloc((void **)p, max_unique_ * 4));
        SAM_HIP(hipMalloc(&b->idx_ws, ggms_cache_index_workspace_bytes(max_unique_)));
        SAM_HIP(hipMalloc(&b->miss_rows_dev, max_unique_ * row_bytes));
      }
      SAM_HIP(hipEventCreateWithFlags(&b->ev_ids, hipEventDisableTiming));
      SAM_HIP(hipHostMalloc(&b->miss_rows_host, max_unique_ * row_bytes));
      SAM_HIP(hipHostMalloc((void **)&b->miss_ids_host, max_unique_ * 4));
    }
    SAM_HIP(hipHostMalloc((void **)&b->counts, CountsBytes(L)));
    std::memset(b->counts, 0, CountsBytes(L));
    SAM_HIP(hipEventCreateWithFlags(&b->ev_seeds, hipEventDisableTiming));
    SAM_HIP(hipEventCreateWithFlags(&b->ev_label, hipEventDisableTiming));
    SAM_HIP(hipEventCreate(&b->ev_xstart));
    SAM_HIP(hipEventCreate(&b->ev_done));
    SAM_GGMS(ggms_launch_timer_create(&b->gather_timer));
    if (BatchSampledElsewhere()) SAM_GGMS(ggms_launch_timer_create(&b->handoff_timer));
    if (Dedicated()) { // the sampler's side of the slot, on the sampler GPU (GetGraphFileCtx, cuda_engine.cc:437-481)
      SAM_HIP(hipSetDevice(device_));
      b->sampler.Alloc(max_edges_, max_unique_, max_seeds_, cfg.sample_type == GGMS_RANDOM_WALK);
    } else {
      b->sampler = b->trainer;
    }
    SAM_HIP(hipEventCreate(&b->ev_start)); // both recorded on the sampling stream
    SAM_HIP(hipEventCreate(&b->ev_sampled));
    if (cfg.arch == kArch4) {
      SAM_HIP(hipEventCreate(&b->ev_expand));
      SAM_HIP(hipEventCreate(&b->ev_final));
    }
    SAM_HIP(hipSetDevice(trainer_device_));
    slots_.push_back(std::move(b));
  }
  train_ready_ = true;
}

void Engine::Init() { // samgraph_init, single process
  if (cfg.arch == kArch0) {
    CpuInit();
    return;
  }
  DataInit();
  const std::string ctx = "cuda:" + std::to_string(cfg.sampler_device);
  SampleInit(0, ctx);
  TrainInit(0, "cuda:" + std::to_string(cfg.trainer_device));
}

// GPUEngine::Start (cuda/cuda_engine.cc:292-317): arch3 starts its background sample + hand-off + extract loop, and the
// caller only asks for batches (get_next_batch).  The other deployments start theirs with extract_start, or not at all.
void Engine::Start() {
  if (Dedicated()) ExtractStart(0);
}

void Engine::Shutdown() {
  shutdown_ = true;
  bg_stop_ = true;
  pool_cv_.notify_all();
  if (bg_.joinable()) bg_.join();
  if (cfg.arch == kArch0) CpuShutdown();
  for (auto &P : pipes_)
    if (P.stream) (void)hipStreamSynchronize(P.stream);
  if (stream_) (void)hipStreamSynchronize(stream_);
  if (stream_extract_) (void)hipStreamSynchronize(stream_extract_);
  if (stream_extract2_) (void)hipStreamSynchronize(stream_extract2_);
  if (d_heads_) (void)ggms_list_heads_detach(&graph_); // the handle goes back; device memory stays until the process ends
}

// ------------------------------------------------------------------ hot loop
Batch *Engine::AcquireSlot(bool background) {
  for (;;) {
    {
      std::lock_guard<std::mutex> lk(pool_mu_);
      for (auto &b : slots_)
        if (!b->in_use && b->refs.load() == 0) { b->in_use = true; return b.get(); }
    }
    if (bg_stop_) return nullptr;
    // GraphPool full (cuda_loops_arch1.cc:45-48): the foreground call returns without sampling,
    // the background thread backs off and retries
    if (!background) return nullptr;
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// samgraph_sample_once: the batches come out in shuffler order whoever asks, so the foreground call keeps
// `lookahead` more of them enqueued than it was asked for -- batch k+1 samples while batch k's rows are gathered and
// while the caller trains on batch k.  The pool hands them out in the same order (GetNextBatch).
void Engine::RunSampleOnce(bool background) {
  if (IsArch5Sampler()) { // dist_loops_arch5.cc RunSampleSubLoopOnce: sample one batch and send it
    SendOne();
    return;
  }
  // the role is an argument, never inferred from the std::thread member (the new thread would read it while
  // ExtractStart is still assigning it)
  if (background) { // background loop: one per iteration
    (void)EnqueueOne(true);
    return;
  }
  ++fg_calls_;
  while (fg_enqueued_ < fg_calls_ + cfg.lookahead && EnqueueOne(false)) ++fg_enqueued_;
  // a call that found the pool full (cuda_loops_arch1.cc:45-48) stays owed: a later call catches up
}

// RunArch1LoopsOnce (cuda/cuda_loops_arch1.cc:43-86) / RunArch6LoopsOnce (dist/dist_loops_arch6.cc:236-243):
// shuffle -> sample -> extract, all enqueued with no host round trip.  false: no free slot, or training finished.
bool Engine::EnqueueOne(bool background) {
  if (cfg.arch == kArch0) return CpuEnqueueOne(background);
  SAM_CHECK(train_ready_, "engine not initialised");
  // arch3: sample_once() runs on the caller's training thread, whose current device is the trainer GPU (torch's
  // streams, events and allocations follow it) -- it is left as the caller had it, on every way out of here
  struct RestoreDevice {
    int dev = -1;
    ~RestoreDevice() { if (dev >= 0) (void)hipSetDevice(dev); }
  } restore;
  if (Dedicated()) SAM_HIP(hipGetDevice(&restore.dev));
  SAM_HIP(hipSetDevice(device_));
  Batch *b = AcquireSlot(background);
  if (!b) return false;
  if (cfg.arch == kArch5) { // a trainer: the next message from the queue instead of a batch of its own
    if (!Receive(b)) {
      std::lock_guard<std::mutex> lk(pool_mu_);
      b->in_use = false;
      return false;
    }
    ++enq_count_;
    EnqueueGather(b, nullptr);
    return true;
  }
  // Consecutive batches go to the sampling pipelines round-robin; a batch's seeds are copied on ITS pipeline's
  // stream (not behind another pipeline's queued sampling).
  Pipe &P = pipes_[enq_count_ % pipes_.size()];
  hipStream_t ss = P.stream;
  if (!ShufflerNext(b, ss)) { // training finished
    std::lock_guard<std::mutex> lk(pool_mu_);
    b->in_use = false;
    return false;
  }
  ++enq_count_;
  SAM_HIP(hipEventRecord(b->ev_start, ss));
  SampleInto(b, P);
  EnqueueGather(b, ss);
  return true;
}

void Engine::SampleInto(Batch *b, Pipe &P) {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  const BatchArrays &s = b->sampler;
  ggms_sample_extra_t extra = extra_;
  extra.data = s.data.data();
  extra.seeds_distinct = BatchSeedsDistinct(cur_step_ * cfg.batch_size, b->num_seeds) ? 1u : 0u;
  // The RNG pool -- and khop2's CSR -- is handed from batch to batch through rng_wait / rng_done, so the results
  // are those of the one-batch-at-a-time loop.
  // khop_labor: the salt follows the batch's key -- (epoch, global index in the epoch) -- not the order of enqueueing
  extra.labor_salt = ggms::labor_batch_salt(cfg.labor_seed, b->key / num_global_step_, b->key % num_global_step_);
  if (cfg.link_prediction) {
    // edge ids -> sources, destinations, negatives, straight into the batch's output nodes.  The salt follows the
    // batch's key like khop_labor's: a batch is a function of its key, whatever pipeline draws it.  The forced count
    // travels to the host with the counts.
    uint64_t *forced = s.counts_dev + GGMS_COUNT_LINK_FORCED(L);
    SAM_HIP(hipMemsetAsync(forced, 0, 8, P.stream));
    const uint32_t salt = ggms::fmix32(extra.labor_salt ^ 0x6c696e6bu);
    SAM_GGMS(ggms_link_seeds(&graph_, b->edge_ids, b->num_pos, cfg.num_negative, cfg.negative_mode, salt, s.output_nodes,
                             forced, P.stream));
    extra.seeds_distinct = 0;
    // khop_temporal: every entry of the seed list is sampled before the time of its positive edge
    if (cfg.Temporal())
      SAM_GGMS(ggms_link_seed_times(d_edge_time_, ds.num_edge, b->edge_ids, b->num_pos, cfg.num_negative, b->seed_time,
                                    P.stream));
  }
  if (pipes_.size() > 1 && cfg.sample_type != GGMS_KHOP0 && cfg.sample_type != GGMS_KHOP_LABOR && !cfg.Temporal() &&
      !cfg.Typed()) {
    extra.rng_wait = last_rng_done_;
    extra.rng_done = P.rng_done;
    last_rng_done_ = P.rng_done;
  }
  // input nodes = the table's unique list (task->input_nodes, dist_loops.cc:357).  The table struct is plain data and
  // its n2o buffer the caller's: the batch builds the list directly in its slot (a later batch uses another slot)
  ggms_hashtable_t ht = P.ht;
  ht.n2o = s.input_nodes;
  ht.n2o_size = max_unique_;
  if (cfg.arch == kArch4) // DoGPUSampleDyCache: the input set is final at ev_final, before the last layer
    SAM_GGMS(ggms_sample_batch_prefetch(cfg.sample_type, &graph_, s.output_nodes, b->num_seeds, cfg.fanout.data(), L, &ht,
                                        states_, num_states_, s.row.data(), s.col.data(), s.counts_dev, &extra,
                                        max_prefetch_edges_, (ggms_event_t)b->ev_expand, (ggms_event_t)b->ev_final, P.ws,
                                        ws_bytes_, P.stream));
  else if (cfg.Temporal()) {
    // the pipeline's own cut table and stamp counter; a wrapped stamp zeroes the table on the pipeline's stream, in
    // front of the batch that starts again from 1.  The sampler fills the batch's eid buffers itself.
    if (P.stamp == 0xffffffffu) {
      SAM_HIP(hipMemsetAsync(P.cut_table, 0, std::max<size_t>(ds.num_node, 1) * 8, P.stream));
      P.stamp = 0;
    }
    const ggms_temporal_t t{d_edge_time_, P.cut_table, ++P.stamp, (uint32_t)cfg.temporal_pick};
    SAM_GGMS(ggms_sample_batch_temporal(&graph_, s.output_nodes, b->seed_time, b->num_seeds, cfg.fanout.data(), L, &ht,
                                        s.row.data(), s.col.data(), b->eid.data(), b->node_cut, s.counts_dev, &t, &extra, P.ws,
                                        ws_bytes_, P.stream));
  } else if (cfg.Typed()) {
    // the sampler fills the batch's eid and etype buffers itself, on the pipeline's stream like everything else here
    const ggms_typed_t t{d_edge_type_, cfg.num_edge_type, cfg.type_fanout.data()};
    SAM_GGMS(ggms_sample_batch_typed(&graph_, s.output_nodes, b->num_seeds, cfg.fanout.data(), L, &ht, s.row.data(),
                                     s.col.data(), b->eid.data(), b->etype.data(), s.counts_dev, &t, &extra, P.ws, ws_bytes_,
                                     P.stream));
  } else
    SAM_GGMS(ggms_sample_batch(cfg.sample_type, &graph_, s.output_nodes, b->num_seeds, cfg.fanout.data(), L, &ht, states_,
                               num_states_, s.row.data(), s.col.data(), s.counts_dev, &extra, P.ws, ws_bytes_, P.stream));
  P.ht.version = ht.version; // the batch bumped the table's version stamp
  if (cfg.link_prediction) { // the pair ids: out of the workspace, which the pipeline's next batch rewrites
    const ggms_id_t *ids = nullptr;
    SAM_GGMS(ggms_sample_batch_seed_ids(cfg.sample_type, b->num_seeds, cfg.fanout.data(), L, &extra, P.ws, &ids));
    SAM_HIP(hipMemcpyAsync(b->seed_ids, ids, b->num_seeds * 4, hipMemcpyDeviceToDevice, P.stream));
    if (cfg.exclude_seed_edges) {
      // The positives leave the layers before anything reads them: pair i is (ids[i], ids[B + i]), the batch's own seed
      // ids in the sampling workspace (local ids, the id space of row / col); the filter works in P.drop_ws.  The layers'
      // edge counts are replaced on the device, in front of ev_sampled: the counts that go to the host, the COO the
      // trainer is handed and the blocks built from it all see the filtered layers.
      SAM_HIP(hipMemsetAsync(b->excluded_dev, 0, L * 8, P.stream));
      SAM_GGMS(ggms_drop_pair_edges(ids, ids + b->num_pos, b->num_pos, cfg.exclude_seed_edges, s.row.data(), s.col.data(),
                                    max_edges_.data(), L, s.counts_dev, b->excluded_dev, P.drop_ws, drop_ws_bytes_,
                                    P.stream));
      SAM_HIP(hipMemcpyAsync(b->excluded, b->excluded_dev, L * 8, hipMemcpyDeviceToHost, P.stream));
    }
  }
  if (cfg.edge_ids && !cfg.SamplerEmitsEdgeIds()) {
    // Which edge of the graph every sampled edge is: a post-pass over the finished layers (behind the filter: the ids of
    // the edges that are left), with the batch's own input nodes as the local -> global map.  Same stream, no new one
    // (EnqueueGather's note on the four hardware queues), in front of ev_sampled like everything that writes the batch.
    SAM_GGMS(ggms_edge_positions(&graph_, ds.num_edge, s.input_nodes, max_unique_, s.row.data(), s.col.data(),
                                 b->eid.data(), max_edges_.data(), L, s.counts_dev, P.eid_ws, eid_ws_bytes_, P.stream));
  }
  if (cfg.induced) {
    // Every edge of the graph among the batch's input nodes: a post-pass over the finished node list, on the pipeline's
    // map and workspace, same stream, in front of ev_sampled like everything that writes the batch.  The two counts go to
    // the host here, behind the call: whichever stream completes the batch (ev_done) is ordered behind ev_sampled.
    SAM_GGMS(ggms_induced_edges(&graph_, ds.num_edge, s.input_nodes, max_unique_, s.counts_dev + GGMS_COUNT_INPUT(L),
                                P.induced_map, b->ind_row, b->ind_col, b->ind_eid, induced_max_edges_, b->ind_counts_dev,
                                P.induced_ws, induced_ws_bytes_, P.stream));
    SAM_HIP(hipMemcpyAsync(b->ind_counts, b->ind_counts_dev, 2 * 8, hipMemcpyDeviceToHost, P.stream));
    if (cfg.edge_feat) // the rows the gather may read: never more than were written, whatever M says
      SAM_GGMS(ggms_induced_kept(b->ind_counts_dev, induced_max_edges_, b->ind_counts_dev + 2, P.stream));
  }
  if (cfg.hetero) {
    // The typed view of the finished batch: the nodes grouped by type -- one `local` array serves every layer, the
    // layers' source sets being nested prefixes of the input nodes; the cuts are the layers' source counts and the last
    // layer's destination count -- then every layer's edges grouped by relation and renumbered through it.  Same stream,
    // the pipeline's workspace, in front of ev_sampled like everything that writes the batch; the small words go to the
    // host behind the calls, as the induced counts do.
    uint32_t cut_words[GGMS_HETERO_MAX_CUTS];
    for (uint32_t i = 0; i < L; ++i) cut_words[i] = GGMS_COUNT_SRC(i);
    cut_words[L] = GGMS_COUNT_DST(L - 1);
    SAM_GGMS(ggms_hetero_nodes(d_node_type_, ds.num_node, ds.num_node_type, s.input_nodes, max_unique_,
                               s.counts_dev + GGMS_COUNT_INPUT(L), s.counts_dev, cut_words, L + 1, b->het_ntype, b->het_local,
                               b->het_slot, b->het_typed, b->het_words_dev + HetBaseAt(), b->het_words_dev + HetCutsAt(),
                               P.hetero_ws, hetero_ws_bytes_, P.stream));
    SAM_GGMS(ggms_hetero_edges(s.row.data(), s.col.data(), b->eid.data(), b->etype.data(), max_edges_.data(), L,
                               cfg.num_edge_type, s.counts_dev, b->het_local, max_unique_, b->het_row.data(),
                               b->het_col.data(), b->het_eid.data(), b->het_words_dev + HetOffsetsAt(), P.hetero_ws,
                               hetero_ws_bytes_, P.stream));
    SAM_HIP(hipMemcpyAsync(b->het_words, b->het_words_dev, HetWords() * 4, hipMemcpyDeviceToHost, P.stream));
  }
  SAM_HIP(hipMemsetAsync(s.counts_dev + GGMS_COUNT_MISS(L), 0, 8, P.stream)); // the trainer's miss count starts at 0
  SAM_HIP(hipEventRecord(b->ev_sampled, P.stream));
}

// the labels and the feature rows of batch b, sampled on stream ss; then b goes to the pool
void Engine::EnqueueGather(Batch *b, hipStream_t ss) {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  uint64_t *n_in = b->trainer.counts_dev + GGMS_COUNT_INPUT(L), *n_miss = b->trainer.counts_dev + GGMS_COUNT_MISS(L);
  // arch3: everything from here on runs on the trainer GPU, on the batch's extract stream -- hand-off, labels, rows,
  // counts -- and the sampling stream is left to the sampler.  arch5: the same on the trainer's GPU, starting with the
  // unpack of the batch's queue slot (there is no sampling stream)
  const bool remote = BatchSampledElsewhere();
  // DoGPULabelExtract (dist_loops.cc:938-974) needs the seeds only: it rides behind the batch on its sampling stream, not
  // between two gathers on the extract stream, which bounds the step.  (Not on a stream of its own: HIP streams share 4
  // hardware queues, and a fifth stream serialises streams that have nothing to do with each other.)
  if (!remote) SAM_GGMS(ggms_extract(b->label, label_src_, b->trainer.output_nodes, b->num_seeds, 1, GGMS_I64, ss));
  const bool mock = ds.feat_mask != 0xffffffffu; // SAMGRAPH_EMPTY_FEAT: host rows are node & mask
  // The extract stream bounds the step, and every event record / wait / small copy on it is a packet the command
  // processor works through between two gathers -- 28 us of dead time per 0.7-ms step with six of them
  // (profiles/r05_ab_extract_stream.txt).  LEAN batch: the gather writes nothing the host reads (no miss / tier
  // counters, no visit counts), so the batch's counts go to the host behind the label gather on the SAMPLING stream,
  // which has the slack, and the extract stream carries one wait and the gather -- whose start / end timestamps and
  // "rows are out" event ride on its own dispatch packet (b->gather_timer).  Otherwise the sequence the counters need.
  // (no row can miss when every node is cached: the miss count stays the zero the sampling stream wrote, and the
  // per-tier row counts, which nothing on the host reads, are not taken)
  const bool can_miss = num_cached_nodes_ < ds.num_node;
  const bool gather_counts = cfg.UseGPUCache() && (mock || ((num_replica_ || cache_table_) && can_miss));
  static const bool lean_off = [] { const char *e = getenv("SAMGRAPH_LEAN_EXTRACT"); return e && e[0] == '0'; }(); // A/B hook
  // (typed_feat: the gather is one launch per chunk class and writes offset words the host reads -- a timer on its first
  // launch does not say "the rows are out", so such a batch takes the event sequence)
  b->lean = !lean_off && !StagedHostTier() && !gather_counts && !node_access_dev_ && !cfg.typed_feat;
  if (!remote && b->lean) {
    SAM_HIP(hipMemcpyAsync(b->counts, b->trainer.counts_dev, CountsBytes(L), hipMemcpyDeviceToHost, ss));
    SAM_HIP(hipEventRecord(b->ev_done, ss)); // labels and counts are out; the rows: gather_timer
  } else if (!remote) {
    SAM_HIP(hipEventRecord(b->ev_label, ss));
  }
  // The gather is HBM-bound, the sampler latency-bound: they run on separate streams so that batch k's
  // extract overlaps batch k+1's sampling (the reference serialises them, dist_loops_arch6.cc:248-251)
  hipStream_t xs = (b->lean && stream_extract2_ && (enq_count_ & 1)) ? stream_extract2_ : stream_extract_;
  if (remote) SAM_HIP(hipSetDevice(trainer_device_));
  const bool arch4 = cfg.arch == kArch4;
  if (cfg.arch == kArch5) Unpack(b, xs); // the batch's arrays, queue slot -> T (the slot is free again when it returns)
  else SAM_HIP(hipStreamWaitEvent(xs, arch4 ? b->ev_final : b->ev_sampled, 0)); // arch4: as soon as the input set is final
  if (remote) {
    if (cfg.arch == kArch3) Handoff(b, xs); // the batch's arrays, S -> T; the gather below reads the input nodes and their count on T
    if (arch4) { // input nodes + their count and the seeds now; the miss count starts at 0 on T (the sampler's comes later)
      Handoff(b, xs, kHandoffIds);
      SAM_HIP(hipMemsetAsync(n_miss, 0, 8, xs));
    }
    SAM_GGMS(ggms_extract(b->label, label_src_, b->trainer.output_nodes, b->num_seeds, 1, GGMS_I64, xs));
  }
  // edge_feat: the edge table's rows under the layers' edge ids, table[eid], with the plain row gather and the device
  // edge count.  On the node rows' stream and IN FRONT of their gather: a lean batch is complete when that gather's
  // own packet says so (gather_timer), and stream order then covers these.
  if (cfg.edge_feat)
    for (uint32_t i = 0; i < L; ++i)
      SAM_GGMS(ggms_gather_scatter(b->efeat[i], d_edge_feat_, b->eid[i], nullptr, max_edges_[i],
                                   b->trainer.counts_dev + GGMS_COUNT_EDGES(i), ds.edge_feat_dim, ds.edge_feat_dtype, xs));
  if (cfg.edge_feat && cfg.induced) // ... and once more over the induced edges' ids (the count: min(M, capacity))
    SAM_GGMS(ggms_gather_scatter(b->ind_efeat, d_edge_feat_, b->ind_eid, nullptr, induced_max_edges_, b->ind_counts_dev + 2,
                                 ds.edge_feat_dim, ds.edge_feat_dtype, xs));
  // khop_temporal: the sampled edges' times, edge_time[eid], beside the edge rows (dim 1, the device edge count)
  if (cfg.Temporal())
    for (uint32_t i = 0; i < L; ++i)
      SAM_GGMS(ggms_gather_scatter(b->etime[i], d_edge_time_, b->eid[i], nullptr, max_edges_[i],
                                   b->trainer.counts_dev + GGMS_COUNT_EDGES(i), 1, GGMS_I32, xs));
  if (b->lean) SAM_GGMS(ggms_launch_timer_arm(b->gather_timer));
  else SAM_HIP(hipEventRecord(b->ev_xstart, xs)); // the extract's own start: behind the previous batch's extract on xs
  // the rows are delivered in the batch's dtype (config key feat_out_dtype; the table's own without the key, which is
  // the plain gather: a *_convert call with one dtype IS its plain namesake)
  const int out_dtype = batch_feat_dtype();
  // hetero_batch: the rows are gathered in the grouped order -- the same count, the same kernel, another id list -- so a
  // type's rows are one contiguous slice of the batch's feature buffer and there is no second pass over the rows
  const uint32_t *const gather_nodes = cfg.hetero ? b->het_typed : b->trainer.input_nodes;
  uint32_t dyn_seq = 0;
  if (cfg.dynamic_cache) { // batch order on one extract stream; seq wraps: the table starts again from zero
    if (++dyn_seq_ == 0) {
      SAM_GGMS(ggms_dynamic_cache_reset(dyn_stamps_, ds.num_node, xs));
      dyn_seq_ = 1;
    }
    dyn_seq = dyn_seq_;
  }
  if (cfg.typed_feat) {
    // one table per node type: the grouped list and its base words, as ggms_hetero_nodes wrote them, in place of the
    // one-table gather; the blocks' offsets go to the host behind it
    SAM_GGMS(ggms_gather_typed(b->feat, typed_feat_bytes_, typed_tables_.data(), ds.num_node_type, b->het_typed,
                               b->het_words_dev + HetBaseAt(), max_unique_, d_node_rank_, ds.num_node, b->het_off_dev, xs));
    SAM_HIP(hipMemcpyAsync(b->het_off, b->het_off_dev, (ds.num_node_type + 1) * 8, hipMemcpyDeviceToHost, xs));
  } else if (StagedHostTier()) {
    StagedExtract(b, ss, xs);
  } else if (cfg.dynamic_cache) { // DoDynamicCacheFeatureCopy (cuda/cuda_loops.cc:1073-1215) as one gather
    SAM_GGMS(ggms_extract_dynamic(b->feat, b->trainer.input_nodes, max_unique_, n_in, dyn_stamps_, dyn_seq,
                                  dyn_prev_ ? dyn_prev_->feat : nullptr, feat_src_, ds.feat_dim, ds.feat_dtype, n_miss, xs));
  } else if (cfg.UseGPUCache() && (mock || num_replica_)) { // every tier in one gather; rows per tier counted
    if (gather_counts) SAM_HIP(hipMemsetAsync(n_miss, 0, GGMS_NUM_TIERS * 8, xs)); // every GGMS_COUNT_TIER word
    ggms_feature_tiers_t tiers{};
    tiers.table = cache_table_;
    tiers.replica = d_replica_;
    tiers.num_replica = num_replica_;
    tiers.parts = (const void *const *)cache_parts_.data();
    tiers.num_part = std::max<uint32_t>(1, num_cache_part_);
    tiers.my_part = cfg.part_cache ? (uint32_t)worker_id_ : 0;
    tiers.host_feat = feat_src_;
    tiers.host_row_mask = mock ? ds.feat_mask : 0;
    SAM_GGMS(ggms_extract_tiered_convert(b->feat, gather_nodes, max_unique_, n_in, &tiers, ds.feat_dim,
                                         ds.feat_dtype, out_dtype, gather_counts ? n_miss : nullptr, xs));
  } else if (cfg.UseGPUCache()) {
    // DoArch6GetCacheMissIndex + DoArch6GPUCacheFeatureCopy (dist_loops.cc:1015-1285) in one pass; everything cached in
    // node order (no table): no row can miss, the count stays the zero the sampling stream wrote
    SAM_GGMS(ggms_extract_cached_convert(b->feat, gather_nodes, max_unique_, n_in, cache_table_,
                                         (const void *const *)cache_parts_.data(), num_cache_part_, feat_src_, ds.feat_dim,
                                         ds.feat_dtype, out_dtype, (cache_table_ && can_miss) ? n_miss : nullptr, xs));
  } else {
    // DoGPUFeatureExtract (cuda/cuda_loops.cc, dist_loops.cc:585-634); with SAMGRAPH_EMPTY_FEAT GPUMockExtract
    // (cuda_loops.cc:692-700 / dist_loops.cc:608-616): row = node & mask (all ones otherwise)
    SAM_GGMS(ggms_gather_scatter_convert(b->feat, feat_src_, gather_nodes, nullptr, max_unique_, n_in,
                                         ds.feat_dim, ds.feat_dtype, out_dtype, ds.feat_mask, xs));
  }
  if (cfg.dynamic_cache) { // the next batch finds these rows in b->feat; b holds the batch it read until it is finished
    SAM_GGMS(ggms_dynamic_cache_publish(dyn_stamps_, b->trainer.input_nodes, max_unique_, n_in, dyn_seq, xs));
    b->dyn_hold = dyn_prev_;
    if (dyn_prev_) dyn_prev_->refs.fetch_add(1);
    dyn_prev_ = b;
  }
  if (arch4) { // the COO once the sampler is done (DoGraphCopy)
    SAM_HIP(hipStreamWaitEvent(xs, b->ev_sampled, 0));
    Handoff(b, xs, kHandoffGraph);
  }
  if (!b->lean) {
    if (node_access_dev_) // Profiler::LogNodeAccess (profiler.cc:570-575): visits per node, counted on the device
      SAM_GGMS(ggms_count_nodes(node_access_dev_, b->trainer.input_nodes, max_unique_, n_in, xs));
    if (!remote) SAM_HIP(hipStreamWaitEvent(xs, b->ev_label, 0)); // the batch is complete when its labels are, too
    SAM_HIP(hipMemcpyAsync(b->counts, b->trainer.counts_dev, CountsBytes(L), hipMemcpyDeviceToHost, xs));
    SAM_HIP(hipEventRecord(b->ev_done, xs));
  } else if (remote) { // counts of T (the gather may have added to them) to the host behind the rows
    SAM_HIP(hipMemcpyAsync(b->counts, b->trainer.counts_dev, CountsBytes(L), hipMemcpyDeviceToHost, xs));
    SAM_HIP(hipEventRecord(b->ev_done, xs));
  }
  {
    std::lock_guard<std::mutex> lk(pool_mu_);
    pool_.push_back(b); // graph_pool->Submit
  }
  pool_cv_.notify_all();
}

// arch3: DoGraphCopy + DoIdCopy (cuda/cuda_loops.cc:600-655) as one launch on the trainer GPU's extract stream.  Every
// length is read by the kernel from the sampler's counts words (the output nodes' from the host: the shuffler knows
// it), so the batch is still enqueued without a host round trip.  The counts words themselves are the last segment:
// the status word and the zeroed miss count travel with them.
// arch4 splits it: kHandoffIds (input nodes, their count, the seeds) at "input set final", kHandoffGraph (the COO and the
// other counts words, the trainer's miss count left alone) at the sampler's end.
void Engine::Handoff(Batch *b, hipStream_t xs, HandoffPart part) {
  const uint32_t L = (uint32_t)cfg.fanout.size();
  ggms_copy_seg_t segs[GGMS_HANDOFF_MAX_SEGS];
  uint32_t n = 0;
  auto add = [&](const void *src, void *dst, const uint64_t *count_dev, uint64_t count_host, uint64_t max_count,
                 uint32_t elem_bytes) {
    SAM_CHECK(n < GGMS_HANDOFF_MAX_SEGS, "arch3: too many hand-off segments");
    segs[n++] = ggms_copy_seg_t{src, dst, count_dev, count_host, max_count, elem_bytes, 0};
  };
  const BatchArrays &s = b->sampler, &t = b->trainer;
  // counts words [first, last]; a segment starts 16-byte aligned: at the even word at or before `first`, so one word
  // more may travel -- each call says why that word is harmless
  auto add_counts = [&](uint32_t first, uint32_t last) {
    const uint32_t w = first & ~1u;
    add(s.counts_dev + w, t.counts_dev + w, nullptr, last + 1 - w, last + 1 - w, 8);
  };
  if (part == kHandoffIds) {
    add(s.input_nodes, t.input_nodes, s.counts_dev + GGMS_COUNT_INPUT(L), 0, max_unique_, 4);
    add(s.output_nodes, t.output_nodes, nullptr, b->num_seeds, max_seeds_, 4);
    add_counts(GGMS_COUNT_INPUT(L), GGMS_COUNT_INPUT(L)); // (the word before it is GGMS_COUNT_DST(L - 1) = |seeds|)
    SAM_GGMS(ggms_batch_handoff(segs, n, xs));
    return;
  }
  for (uint32_t i = 0; i < L; ++i) {
    add(s.row[i], t.row[i], s.counts_dev + GGMS_COUNT_EDGES(i), 0, max_edges_[i], 4);
    add(s.col[i], t.col[i], s.counts_dev + GGMS_COUNT_EDGES(i), 0, max_edges_[i], 4);
    if (s.data[i]) add(s.data[i], t.data[i], s.counts_dev + GGMS_COUNT_EDGES(i), 0, max_edges_[i], 4);
  }
  if (part == kHandoffGraph) { // what the sampler wrote (status included) and the expansion's edge count
    add_counts(0, GGMS_COUNT_STATUS(L));
    add_counts(GGMS_COUNT_EXPANSION(L), GGMS_COUNT_EXPANSION(L)); // (the word before it is a tier counter arch4 does not use)
  } else {
    add(s.input_nodes, t.input_nodes, s.counts_dev + GGMS_COUNT_INPUT(L), 0, max_unique_, 4);
    add(s.output_nodes, t.output_nodes, nullptr, b->num_seeds, max_seeds_, 4);
    add_counts(0, GGMS_COUNTS_WORDS(L) - 1);
  }
  SAM_GGMS(ggms_launch_timer_arm(b->handoff_timer)); // kLogL2GraphCopyTime: the hand-off's own time
  SAM_GGMS(ggms_batch_handoff(segs, n, xs));
}

// a kernel of the batch hit a bound it must not hit (include/ggms.h, device status word): the reference CHECK-aborts in
// these places (logging.cc:69-73), and so does the engine
void Engine::CheckBatchStatus(uint64_t status, uint64_t key) const {
  if (status == 0) return;
  const std::string where = IsArch5Sampler() ? " on sampler " + std::to_string(worker_id_) : "";
  fprintf(stderr, "[samgraph] FATAL: device status %#llx after batch %llu%s (%s%s): results are invalid\n",
          (unsigned long long)status, (unsigned long long)key, where.c_str(),
          (status & GGMS_STATUS_SCAN_SPIN) ? "ordered scan: look-back gave up " : "",
          (status & GGMS_STATUS_TABLE_FULL) ? "hashed dedup table full" : "");
  abort();
}

// block until the batch is complete, publish sizes, log the items the scripts read
// prev: the batch handed out before this one (still owned by the caller: its timer has not been re-armed)
void Engine::Finish(Batch *b, Batch *prev) {
  if (cfg.arch == kArch0) return; // complete (and logged) when it was enqueued
  SAM_HIP(hipEventSynchronize(b->ev_done));
  double us_gather = 0; // a lean batch's rows: complete when its gather is (the timer's end event)
  double us_busy = 0;   // ... and what it added to the extract streams' busy time
  if (b->lean) {
    SAM_GGMS(ggms_launch_timer_elapsed_us(b->gather_timer, &us_gather));
    us_busy = us_gather;
    // Two extract streams: this gather may have started while the previous batch's was still running.  The epoch's
    // copy time (kLogEpochCopyTime: bytes / time = the extract rate the scripts print) counts every moment once:
    // this batch adds  min(own duration, its end - the previous gather's end).
    if (stream_extract2_ && prev && prev->lean) {
      double us_span = 0, us_prev = 0; // previous start -> this end; previous duration
      if (ggms_launch_timer_span_us(prev->gather_timer, b->gather_timer, &us_span) == GGMS_OK &&
          ggms_launch_timer_elapsed_us(prev->gather_timer, &us_prev) == GGMS_OK)
        us_busy = std::min(us_gather, std::max(0.0, us_span - us_prev));
    }
  }
  const uint32_t L = (uint32_t)cfg.fanout.size();
  b->num_input = b->counts[GGMS_COUNT_INPUT(L)];
  b->num_miss = b->counts[GGMS_COUNT_MISS(L)];
  if (b->dyn_hold) { // this batch's gather is complete: the batch it read may go
    b->dyn_hold->refs.fetch_sub(1);
    b->dyn_hold = nullptr;
  }
  if (cfg.arch == kArch4 && (b->counts[GGMS_COUNT_STATUS(L)] & GGMS_STATUS_PREFETCH_FULL))
    fatal(__FILE__, __LINE__, "arch4: batch " + std::to_string(b->key) + ": the expansion needed " +
                                  std::to_string(b->counts[GGMS_COUNT_EXPANSION(L)]) + " edges, capacity " +
                                  std::to_string(max_prefetch_edges_) + " (config key prefetch_max_edges)");
  if (cfg.induced && b->ind_counts[0] > induced_max_edges_)
    fatal(__FILE__, __LINE__, "induced_subgraph: batch " + std::to_string(b->key) + ": its " + std::to_string(b->num_input) +
                                  " input nodes induce " + std::to_string(b->ind_counts[0]) + " edges, capacity " +
                                  std::to_string(induced_max_edges_) + " (config key induced_max_edges: at least " +
                                  std::to_string(b->ind_counts[0]) + ")");
  CheckBatchStatus(b->counts[GGMS_COUNT_STATUS(L)], b->key);
  if (cfg.link_prediction) { // negatives whose eight candidates were all rejected, per epoch
    link_forced_ += b->counts[GGMS_COUNT_LINK_FORCED(L)];
    for (uint32_t i = 0; b->excluded && i < L; ++i) link_excluded_ += b->excluded[i];
    if (b->key % num_global_step_ == num_global_step_ - 1) {
      log_info("link_prediction: epoch " + std::to_string(b->key / num_global_step_) + ": " + std::to_string(link_forced_) +
               " forced negatives of " + std::to_string(ds.num_train_edge * cfg.num_negative));
      if (cfg.exclude_seed_edges)
        log_info("link_prediction: epoch " + std::to_string(b->key / num_global_step_) + ": " +
                 std::to_string(link_excluded_) + " sampled edges excluded (exclude_seed_edges = " +
                 (cfg.exclude_seed_edges == GGMS_DROP_FORWARD ? "self" : "both") + ")");
      link_forced_ = 0;
      link_excluded_ = 0;
    }
  }
  if (cfg.arch == kArch4 && !cfg.dynamic_cache) b->num_miss = b->num_input; // every row is read from host memory
  float ms_sample = 0, ms_copy = 0;
  if (cfg.arch != kArch5) (void)hipEventElapsedTime(&ms_sample, b->ev_start, b->ev_sampled); // (arch5: sampled elsewhere)
  if (b->lean) ms_copy = (float)(us_gather * 1e-3); // the gather kernel's own time
  else (void)hipEventElapsedTime(&ms_copy, b->ev_xstart, b->ev_done); // not from ev_sampled: that would add the queueing behind the previous extract
  const double s_copy_epoch = b->lean ? us_busy * 1e-6 : ms_copy * 1e-3;
  uint64_t edges = 0;
  for (uint32_t i = 0; i < L; ++i) edges += b->counts[GGMS_COUNT_EDGES(i)];
  // feature bytes: what the gather wrote to the batch (rows in the delivered dtype); miss bytes: what it read from the
  // host tier (rows in the table's dtype)
  const double out_row_bytes = (double)batch_feat_row_bytes();
  // (typed_feat: the rows differ in width by type; what the gather wrote is the end of the last block)
  const double feature_bytes = cfg.typed_feat ? (double)b->het_off[ds.num_node_type] : b->num_input * out_row_bytes;
  const double row_bytes = (double)ds.feat_row_bytes();
  // item codes: profiler.h:58-140 (kLogL1NumSample = 0, kLogL1NumNode = 1, kLogL1SampleTime = 3,
  // kLogL1CopyTime = 6, kLogL1FeatureBytes = 9, kLogL1MissBytes = 13; epoch items :119-137)
  prof.LogStep(b->key, 0, (double)edges);
  prof.LogStep(b->key, 1, (double)b->num_input);
  prof.LogStep(b->key, 3, ms_sample * 1e-3);
  prof.LogStep(b->key, 6, ms_copy * 1e-3);
  prof.LogStep(b->key, 9, feature_bytes);
  prof.LogStep(b->key, 13, b->num_miss * row_bytes);
  prof.LogEpochAdd(b->key, 0 /*kLogEpochSampleTime*/, ms_sample * 1e-3);
  prof.LogEpochAdd(b->key, 8 /*kLogEpochCopyTime*/, s_copy_epoch);
  prof.LogEpochAdd(b->key, 12 /*kLogEpochFeatureBytes*/, feature_bytes);
  prof.LogEpochAdd(b->key, 13 /*kLogEpochMissBytes*/, b->num_miss * row_bytes);
  prof.LogEpochAdd(b->key, 15 /*kLogEpochNumSample*/, (double)edges);
  if (BatchSampledElsewhere()) { // what the hand-off (arch5: the unpack) moved and its time
    double us_handoff = 0;       // (DoGraphCopy / DoIdCopy, cuda/cuda_loops.cc:629,653)
    SAM_GGMS(ggms_launch_timer_elapsed_us(b->handoff_timer, &us_handoff));
    const double per_edge = cfg.sample_type == GGMS_RANDOM_WALK ? 12.0 : 8.0; // row + col (+ data)
    prof.LogStep(b->key, 12 /*kLogL1GraphBytes*/, edges * per_edge);
    prof.LogStep(b->key, 11 /*kLogL1IdBytes*/, (b->num_input + b->num_seeds) * 4.0);
    prof.LogStep(b->key, 22 /*kLogL2GraphCopyTime*/, us_handoff * 1e-6);
    if (cfg.arch == kArch4) { // the expansion's own time, and how far ahead of the sampler's end the gather could start
      float ms_nb = 0, ms_adv = 0;
      (void)hipEventElapsedTime(&ms_nb, b->ev_expand, b->ev_final);
      (void)hipEventElapsedTime(&ms_adv, b->ev_final, b->ev_sampled);
      prof.LogStep(b->key, 15 /*kLogL1GetNeighbourTime*/, ms_nb * 1e-3);
      prof.LogStep(b->key, 14 /*kLogL1PrefetchAdvanced*/, ms_adv * 1e-3);
      if (cfg.dynamic_cache) prof.LogStep(b->key, 26 /*kLogL2CacheCopyTime*/, ms_copy * 1e-3);
    }
    if (cfg.arch == kArch5) { // RunCacheDataCopySubLoopOnce: copy time = recv + graph copy + feature copy
      prof.LogStep(b->key, 5 /*kLogL1RecvTime*/, b->recv_s);
      prof.LogStepAdd(b->key, 6 /*kLogL1CopyTime*/, b->recv_s + us_handoff * 1e-6);
      prof.LogEpochAdd(b->key, 8 /*kLogEpochCopyTime*/, b->recv_s + us_handoff * 1e-6);
    }
  }
}

uint64_t Engine::GetNextBatch() { // operation.cc:366-378 + GraphPool::GetGraphBatch graph_pool.cc:31-49
  // the engine drops its own reference to the previous batch (:370) -- once the next one's gather has been measured
  // against it (Finish): until then its slot, and with it its launch timer, is not handed to the sampler again
  Batch *prev = current_;
  current_ = nullptr;
  Batch *b = nullptr;
  {
    std::unique_lock<std::mutex> lk(pool_mu_);
    if (pool_.empty() && !bg_running_.load())
      fatal(__FILE__, __LINE__, "get_next_batch with nothing sampled: call sample_once() or extract_start() first");
    pool_cv_.wait(lk, [&] { return !pool_.empty() || bg_stop_.load() || !bg_running_.load(); });
    if (pool_.empty())
      fatal(__FILE__, __LINE__, bg_stop_.load() ? "engine shut down while waiting for a batch"
                                                : "get_next_batch: the extract loop handled its count (extract_start) and ended");
    b = pool_.front();
    pool_.pop_front();
  }
  Finish(b, prev);
  if (prev) {
    std::lock_guard<std::mutex> lk(pool_mu_);
    prev->in_use = false;
  }
  current_ = b;
  return b->key;
}

// samgraph_update_graph_feat (config key feat_learnable).  Gathers and updates share the one extract stream, so they are
// totally ordered by the order of the calls that enqueue them: this update is seen by every batch a LATER sample_once
// enqueues and by none enqueued before.  No host synchronisation: two events tie the caller's stream in.
// (No stream of its own: see the note on the 4 hardware queues in EnqueueGather.)
void Engine::UpdateGraphFeat(uint64_t key, const void *grad, size_t num_rows, size_t dim, hipStream_t caller) {
  if (cfg.feat_learnable < 0) fatal(__FILE__, __LINE__, "samgraph_update_graph_feat needs the config key feat_learnable");
  SAM_CHECK(train_ready_ && d_feat_, "engine not initialised");
  Batch *b = Current(key); // the batch is still held: its input nodes and their count are read on the device
  if (num_rows != b->num_input || dim != ds.feat_dim)
    fatal(__FILE__, __LINE__, "samgraph_update_graph_feat: the gradient is (" + std::to_string(num_rows) + ", " +
                                  std::to_string(dim) + "), batch " + std::to_string(key) + " delivered (" +
                                  std::to_string(b->num_input) + ", " + std::to_string(ds.feat_dim) + ") rows");
  SAM_CHECK(grad != nullptr || num_rows == 0, "samgraph_update_graph_feat: null gradient");
  const uint32_t L = (uint32_t)cfg.fanout.size();
  SAM_HIP(hipEventRecord(ev_grad_, caller)); // the gradient is produced on the caller's stream
  SAM_HIP(hipStreamWaitEvent(stream_extract_, ev_grad_, 0));
  SAM_GGMS(ggms_update_rows(d_feat_, d_feat_state_, b->trainer.input_nodes, num_rows,
                            b->trainer.counts_dev + GGMS_COUNT_INPUT(L), grad, ds.feat_dim, cfg.feat_learnable, cfg.feat_lr,
                            cfg.feat_eps, stream_extract_));
  // the caller's stream goes on behind the update: its allocator cannot hand the gradient's memory to later work on that
  // stream before the kernel has read it
  SAM_HIP(hipEventRecord(ev_updated_, stream_extract_));
  SAM_HIP(hipStreamWaitEvent(caller, ev_updated_, 0));
}

void *Engine::StoreFeat(const char *who) const {
  if (cfg.feat_learnable < 0) fatal(__FILE__, __LINE__, std::string(who) + " needs the config key feat_learnable");
  SAM_CHECK(d_feat_ != nullptr, "engine not initialised");
  return d_feat_;
}

void *Engine::StoreState(const char *who) const {
  if (cfg.feat_learnable != GGMS_UPDATE_ADAGRAD)
    fatal(__FILE__, __LINE__, std::string(who) + " needs the config key feat_learnable = adagrad (SGD keeps no state)");
  SAM_CHECK(d_feat_state_ != nullptr, "engine not initialised");
  return d_feat_state_;
}

void Engine::ExtractStart(int count) { // dist_engine.cc StartExtract: one background sample+extract thread
  if (cfg.feat_learnable >= 0)
    fatal(__FILE__, __LINE__, "extract_start with feat_learnable: a background thread would make the updates a batch "
                              "sees a matter of timing; call sample_once()");
  if (cfg.arch == kArch5) { // DataCopySubLoop(count), dist_loops_arch5.cc: `count` messages, then the thread ends
    SAM_CHECK(role_ == kRoleTrainer && train_ready_, "arch5: extract_start on a trainer, after train_init");
    SAM_CHECK(count >= 0, "arch5: extract_start(count >= 0)");
    if (bg_.joinable()) bg_.join(); // the previous call's loop (the scripts call it once per epoch)
    bg_running_ = true;
    bg_ = std::thread([this, count] {
      SAM_HIP(hipSetDevice(device_));
      for (int i = 0; i < count && !bg_stop_; ++i)
        if (!EnqueueOne(true)) break; // only when shutting down
      {
        std::lock_guard<std::mutex> lk(pool_mu_);
        bg_running_ = false;
      }
      pool_cv_.notify_all();
    });
    return;
  }
  SAM_CHECK(!bg_running_.load(), "extract thread already running");
  bg_running_ = true; // set before the thread exists: nothing the thread runs looks at bg_ itself
  bg_ = std::thread([this] {
    SAM_HIP(hipSetDevice(device_));
    while (!bg_stop_) {
      const size_t before_epoch = cur_epoch_;
      RunSampleOnce(true);
      if (cur_epoch_ >= cfg.num_epoch && before_epoch >= cfg.num_epoch) break;
      if (cur_epoch_ >= cfg.num_epoch) break;
    }
  });
}

// samgraph_report_node_access, the _SIMPLE report (profiler.cc:795-860): nodes by visit count, descending --
//   node_access_optimal_cache_bin<t>.txt       u32 node ids in that order (usable as a cache rank file)
//   node_access_optimal_cache_freq_bin<t>.txt  f32 visits per epoch, same order
//   node_access_frequency<t>.txt               "rate\tvisits per epoch of the node at that percentile"
//   node_access_optimal_cache_hit<t>.txt       "rate\thit rate of a cache holding the top rate % of the nodes"
void Engine::ReportNodeAccess() {
  if (!node_access_dev_) return;
  SAM_HIP(hipDeviceSynchronize());
  std::vector<uint32_t> freq(ds.num_node);
  SAM_HIP(hipMemcpy(freq.data(), node_access_dev_, ds.num_node * 4, hipMemcpyDeviceToHost));
  std::vector<std::pair<uint64_t, uint32_t>> rec(ds.num_node);
  for (uint32_t v = 0; v < ds.num_node; ++v) rec[v] = {freq[v], v};
  std::sort(rec.begin(), rec.end(), std::greater<std::pair<uint64_t, uint32_t>>());
  const std::string t = std::to_string((unsigned long long)std::chrono::system_clock::now().time_since_epoch().count());
  FILE *f_freq = fopen(("node_access_frequency" + t + ".txt").c_str(), "w");
  FILE *f_bin = fopen(("node_access_optimal_cache_bin" + t + ".txt").c_str(), "wb");
  FILE *f_hit = fopen(("node_access_optimal_cache_hit" + t + ".txt").c_str(), "w");
  FILE *f_fbin = fopen(("node_access_optimal_cache_freq_bin" + t + ".txt").c_str(), "wb");
  SAM_CHECK(f_freq && f_bin && f_hit && f_fbin, "cannot write the node access files");
  const double epochs = (double)std::max<size_t>(1, cfg.num_epoch);
  uint64_t sum = 0;
  for (auto &p : rec) {
    const float avg = (float)(p.first / epochs);
    fwrite(&p.second, 4, 1, f_bin);
    fwrite(&avg, 4, 1, f_fbin);
    sum += p.first;
    p.first = sum; // running sum, as the reference keeps it
  }
  const size_t n = rec.size();
  for (int rate = 0; rate <= 100; ++rate) {
    size_t idx = rate == 0 ? 0 : ((uint64_t)rate * n - 1) / 100;
    fprintf(f_freq, "%d\t%g\n", rate, idx == 0 ? 0.0 : (double)(rec[idx].first - rec[idx - 1].first) / epochs);
    fprintf(f_hit, "%d\t%g\n", rate, idx == 0 || sum == 0 ? 0.0 : (double)rec[idx].first / (double)sum);
  }
  fclose(f_freq); fclose(f_bin); fclose(f_hit); fclose(f_fbin);
}

Batch *Engine::Current(uint64_t key) {
  SAM_CHECK(current_ != nullptr, "no current batch");
  SAM_CHECK(current_->key == key, "key is not the current batch key (adapter.cc:68)");
  return current_;
}

void Engine::Retain(uint64_t key) { Current(key)->refs.fetch_add(1); }

// batch keys are unique over a run (epoch * steps + step), and a slot is only reused once its refs are back to 0,
// so a key names at most one live slot
void Engine::Release(uint64_t key) {
  for (auto &b : slots_)
    if (b->key == key && b->refs.load() > 0) { b->refs.fetch_sub(1); return; }
}

} // namespace sam
