// operation.cc -- extern "C" samgraph_* entry points (include/samgraph.h).
// Reference: samgraph/common/operation.cc:49-584 and samgraph/torch/adapter.cc:62-193.
#include <sys/wait.h>

#include <chrono>
#include <cstring>

#include "engine.h"

using sam::Engine;

static uint64_t now_us() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
             std::chrono::system_clock::now().time_since_epoch()).count();
}

static void fill(samgraph_tensor_t *t, void *data, int64_t d0, int64_t d1, int ndim, int dtype, int dev_type, int dev_id) {
  t->data = data; t->shape[0] = d0; t->shape[1] = d1; t->ndim = ndim; t->dtype = dtype;
  t->device_type = dev_type; t->device_id = dev_id;
}

extern "C" {

void samgraph_config(const char **keys, const char **values, const size_t n) {
  std::unordered_map<std::string, std::string> kv;
  for (size_t i = 0; i < n; ++i) kv[keys[i]] = values[i];
  Engine::Get().Configure(kv);
}
void samgraph_init(void) { Engine::Get().Init(); }
void samgraph_start(void) { Engine::Get().Start(); }
void samgraph_shutdown(void) { Engine::Get().Shutdown(); }
void samgraph_data_init(void) { Engine::Get().DataInit(); }
void samgraph_sample_init(int worker_id, const char *ctx) { Engine::Get().SampleInit(worker_id, ctx); }
void samgraph_train_init(int worker_id, const char *ctx) { Engine::Get().TrainInit(worker_id, ctx); }
void samgraph_extract_start(int count) { Engine::Get().ExtractStart(count); }
void samgraph_forward_barrier(void) { Engine::Get().Barrier(); }
void samgraph_um_sample_init(int) { sam::fatal(__FILE__, __LINE__, "arch9 (unified-memory sampling) is not part of this build"); }
void samgraph_switch_init(int, const char *, double) { sam::fatal(__FILE__, __LINE__, "the switcher (arch5 with have_switcher) is not part of this build"); }

int samgraph_wait_one_child(void) { // operation.cc:573-584
  int st = 0;
  pid_t pid = waitpid(-1, &st, 0);
  (void)pid;
  if (WIFSIGNALED(st)) return 1;
  if (WEXITSTATUS(st) != 0) return 1;
  return 0;
}

size_t samgraph_num_epoch(void) { return Engine::Get().NumEpoch(); }
size_t samgraph_steps_per_epoch(void) { return Engine::Get().NumStep(); }
size_t samgraph_num_local_step(void) { return Engine::Get().NumLocalStep(); }
size_t samgraph_num_class(void) { return Engine::Get().ds.num_class; }
size_t samgraph_feat_dim(void) { return Engine::Get().ds.feat_dim; }
size_t samgraph_feat_row_bytes(int delivered) {
  auto &E = Engine::Get();
  return delivered ? E.batch_feat_row_bytes() : E.ds.feat_row_bytes();
}
uint64_t samgraph_get_next_batch(void) { return Engine::Get().GetNextBatch(); }
void samgraph_sample_once(void) { Engine::Get().RunSampleOnce(); }

size_t samgraph_get_graph_num_src(uint64_t key, int g) { return Engine::Get().Current(key)->counts[GGMS_COUNT_SRC(g)]; }
size_t samgraph_get_graph_num_dst(uint64_t key, int g) { return Engine::Get().Current(key)->counts[GGMS_COUNT_DST(g)]; }
size_t samgraph_get_graph_num_edge(uint64_t key, int g) { return Engine::Get().Current(key)->counts[GGMS_COUNT_EDGES(g)]; }

void samgraph_log_step(uint64_t e, uint64_t s, int item, double v) { auto &E = Engine::Get(); E.prof.LogStep(E.BatchKey(e, s), item, v); }
void samgraph_log_step_by_key(uint64_t key, int item, double v) { Engine::Get().prof.LogStep(key, item, v); }
void samgraph_log_step_add(uint64_t e, uint64_t s, int item, double v) { auto &E = Engine::Get(); E.prof.LogStepAdd(E.BatchKey(e, s), item, v); }
void samgraph_log_epoch_add(uint64_t e, int item, double v) { auto &E = Engine::Get(); E.prof.LogEpochAdd(E.BatchKey(e, 0), item, v); }
double samgraph_get_log_init_value(int item) { return (item >= 0 && item < sam::Profiler::kMaxInit) ? Engine::Get().prof.GetInit(item) : 0.0; }
double samgraph_get_log_step_value(uint64_t e, uint64_t s, int item) { auto &E = Engine::Get(); return E.prof.GetStep(E.BatchKey(e, s), item); }
double samgraph_get_log_step_value_by_key(uint64_t key, int item) { return Engine::Get().prof.GetStep(key, item); }
double samgraph_get_log_epoch_value(uint64_t e, int item) { return Engine::Get().prof.GetEpoch(e, item); }
void samgraph_report_init(void) {
  auto &p = Engine::Get().prof;
  std::printf("[Init] load dataset %.4f s | build cache %.4f s\n", p.GetInit(6), p.GetInit(10));
  std::fflush(stdout);
}
void samgraph_report_step(uint64_t e, uint64_t s) { Engine::Get().prof.ReportStep(e, s); }
void samgraph_report_step_average(uint64_t e, uint64_t s) { Engine::Get().prof.ReportStep(e, s); std::fflush(stdout); }
void samgraph_report_epoch(uint64_t e) { Engine::Get().prof.ReportEpoch(e); }
void samgraph_report_epoch_average(uint64_t e) { Engine::Get().prof.ReportEpoch(e); std::fflush(stdout); }
void samgraph_report_node_access(void) { Engine::Get().ReportNodeAccess(); } // operation.cc:472-480
void samgraph_trace_step_begin(uint64_t key, int item, uint64_t ts) { Engine::Get().prof.Trace(key, item, ts, true); }
void samgraph_trace_step_end(uint64_t key, int item, uint64_t ts) { Engine::Get().prof.Trace(key, item, ts, false); }
void samgraph_trace_step_begin_now(uint64_t key, int item) { Engine::Get().prof.Trace(key, item, now_us(), true); }
void samgraph_trace_step_end_now(uint64_t key, int item) { Engine::Get().prof.Trace(key, item, now_us(), false); }
void samgraph_dump_trace(void) { Engine::Get().prof.DumpTrace(); }

// ---- tensor hand-off (adapter.cc:62-193) ------------------------------------------------------
void samgraph_get_graph_feat(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (E.cfg.typed_feat)
    sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_feat with typed_feat = on: there is no single feature matrix, the types' "
                                   "rows differ in width and dtype; samgraph_get_graph_feat_of_type(key, t) hands out each block");
  auto *b = E.Current(key);
  fill(out, b->feat, (int64_t)b->num_input, (int64_t)E.ds.feat_dim, 2, E.batch_feat_dtype(), E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_label(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->label, (int64_t)b->num_seeds, 1, 1, GGMS_I64, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_row(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->trainer.row[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_col(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->trainer.col[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_data(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->trainer.data[l], b->trainer.data[l] ? (int64_t)b->counts[GGMS_COUNT_EDGES(l)] : 0, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_dataset_feat(samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (E.ds.feat_dtype == GGMS_Q8ROW) { // no element type: the stored rows as bytes, (rows, stride) of U8
    fill(out, E.ds.feat.ptr, (int64_t)E.ds.feat_rows, (int64_t)E.ds.feat_row_bytes(), 2, GGMS_U8, 0, 0);
    return;
  }
  fill(out, E.ds.feat.ptr, (int64_t)E.ds.feat_rows, (int64_t)E.ds.feat_dim, 2, E.ds.feat_dtype, 0, 0);
}
void samgraph_get_dataset_label(samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  fill(out, E.ds.label.ptr, (int64_t)E.ds.num_node, 1, 1, GGMS_I64, 0, 0);
}
void samgraph_get_graph_input_nodes(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->trainer.input_nodes, (int64_t)b->num_input, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_output_nodes(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  fill(out, b->trainer.output_nodes, (int64_t)b->num_seeds, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
// task = link_prediction: the local id of every entry of the batch's seed list (output nodes), i.e. the pair ids
void samgraph_get_graph_seed_ids(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (!E.cfg.link_prediction) sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_seed_ids needs task = link_prediction");
  auto *b = E.Current(key);
  fill(out, b->seed_ids, (int64_t)b->num_seeds, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
// exclude_seed_edges: the edges the filter took out of this batch's layers, all layers together (0 without the key)
size_t samgraph_get_graph_num_excluded(uint64_t key) {
  auto &E = Engine::Get();
  auto *b = E.Current(key);
  size_t total = 0;
  for (size_t i = 0; b->excluded && i < E.cfg.fanout.size(); ++i) total += b->excluded[i];
  return total;
}
// config keys edge_ids / edge_feat: layer l's edge ids (CSR positions; the uint32 bits in get_graph_row's dtype) and the
// edge table's rows under them, (num_edge(l), EDGE_FEAT_DIM) in the table's dtype
void samgraph_get_graph_edge_ids(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (!E.cfg.edge_ids) sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_edge_ids needs the config key edge_ids = on (or edge_feat = on)");
  auto *b = E.Current(key);
  SAM_CHECK(l >= 0 && (size_t)l < b->eid.size(), "samgraph_get_graph_edge_ids: no such layer");
  fill(out, b->eid[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_edge_feat(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (!E.cfg.edge_feat) sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_edge_feat needs the config key edge_feat = on");
  auto *b = E.Current(key);
  SAM_CHECK(l >= 0 && (size_t)l < b->efeat.size(), "samgraph_get_graph_edge_feat: no such layer");
  fill(out, b->efeat[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], (int64_t)E.ds.edge_feat_dim, 2, E.ds.edge_feat_dtype,
       E.batch_device_type(), E.trainer_device());
}
// config key induced_subgraph: the subgraph the batch's input nodes induce -- num_induced edges (row = the neighbour,
// col = the node whose list was read; local ids, rows of get_graph_feat), their CSR positions, and with edge_feat the edge
// table's rows under those
static sam::Batch *induced_batch(uint64_t key, const char *who, bool need_feat = false) {
  auto &E = Engine::Get();
  if (!E.cfg.induced) sam::fatal(__FILE__, __LINE__, std::string(who) + " needs the config key induced_subgraph = on");
  if (need_feat && !E.cfg.edge_feat)
    sam::fatal(__FILE__, __LINE__, std::string(who) + " needs the config key edge_feat = on (beside induced_subgraph = on)");
  return E.Current(key);
}
size_t samgraph_get_graph_num_induced(uint64_t key) {
  return induced_batch(key, "samgraph_get_graph_num_induced")->ind_counts[0];
}
void samgraph_get_graph_induced_row(uint64_t key, samgraph_tensor_t *out) {
  auto *b = induced_batch(key, "samgraph_get_graph_induced_row");
  auto &E = Engine::Get();
  fill(out, b->ind_row, (int64_t)b->ind_counts[0], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_induced_col(uint64_t key, samgraph_tensor_t *out) {
  auto *b = induced_batch(key, "samgraph_get_graph_induced_col");
  auto &E = Engine::Get();
  fill(out, b->ind_col, (int64_t)b->ind_counts[0], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_induced_edge_ids(uint64_t key, samgraph_tensor_t *out) {
  auto *b = induced_batch(key, "samgraph_get_graph_induced_edge_ids");
  auto &E = Engine::Get();
  fill(out, b->ind_eid, (int64_t)b->ind_counts[0], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_induced_edge_feat(uint64_t key, samgraph_tensor_t *out) {
  auto *b = induced_batch(key, "samgraph_get_graph_induced_edge_feat", true);
  auto &E = Engine::Get();
  fill(out, b->ind_efeat, (int64_t)b->ind_counts[0], (int64_t)E.ds.edge_feat_dim, 2, E.ds.edge_feat_dtype,
       E.batch_device_type(), E.trainer_device());
}
// task = link_prediction: the batch's positive edge ids (CSR positions, the id space of the edge ids above)
void samgraph_get_graph_link_edge_ids(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (!E.cfg.link_prediction) sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_link_edge_ids needs task = link_prediction");
  auto *b = E.Current(key);
  fill(out, b->edge_ids, (int64_t)b->num_pos, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
// _sample_type 9 (khop_temporal): the time of every edge of layer l (edge_time[edge_ids]), the final cut-off of every input
// node, the times of the batch's positive edges -- uint32 bits in get_graph_row's dtype
static sam::Batch *temporal_batch(uint64_t key, const char *who) {
  auto &E = Engine::Get();
  if (!E.cfg.Temporal()) sam::fatal(__FILE__, __LINE__, std::string(who) + " needs _sample_type 9 (khop_temporal)");
  return E.Current(key);
}
void samgraph_get_graph_edge_time(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = temporal_batch(key, "samgraph_get_graph_edge_time");
  SAM_CHECK(l >= 0 && (size_t)l < b->etime.size(), "samgraph_get_graph_edge_time: no such layer");
  fill(out, b->etime[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_node_cut(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = temporal_batch(key, "samgraph_get_graph_node_cut");
  fill(out, b->node_cut, (int64_t)b->counts[GGMS_COUNT_INPUT(E.cfg.fanout.size())], 1, 1, GGMS_I32, E.batch_device_type(),
       E.trainer_device());
}
void samgraph_get_graph_link_time(uint64_t key, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = temporal_batch(key, "samgraph_get_graph_link_time");
  fill(out, b->seed_time, (int64_t)b->num_pos, 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
// _sample_type 10 (khop_typed): the type of every edge of layer l, edge_type[edge_ids], as the sampler wrote it -- uint8
void samgraph_get_graph_edge_type(uint64_t key, int l, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  if (!E.cfg.Typed()) sam::fatal(__FILE__, __LINE__, "samgraph_get_graph_edge_type needs _sample_type 10 (khop_typed)");
  auto *b = E.Current(key);
  SAM_CHECK(l >= 0 && (size_t)l < b->etype.size(), "samgraph_get_graph_edge_type: no such layer");
  fill(out, b->etype[l], (int64_t)b->counts[GGMS_COUNT_EDGES(l)], 1, 1, GGMS_U8, E.batch_device_type(), E.trainer_device());
}
// config key hetero_batch: the batch's heterogeneous view.  The small words (Batch::het_words: base | cuts | offsets) are
// on the host with the counts; every tensor below is a zero-copy view, the per-type and per-relation ones slices
static sam::Batch *hetero_batch(uint64_t key, const char *who) {
  auto &E = Engine::Get();
  if (!E.cfg.hetero) sam::fatal(__FILE__, __LINE__, std::string(who) + " needs the config key hetero_batch = on");
  return E.Current(key);
}
static void hetero_need(const char *who) {
  if (!Engine::Get().cfg.hetero) sam::fatal(__FILE__, __LINE__, std::string(who) + " needs the config key hetero_batch = on");
}
static uint32_t hetero_type(int t, const char *who) {
  SAM_CHECK(t >= 0 && (size_t)t < Engine::Get().ds.num_node_type, std::string(who) + ": no such node type");
  return (uint32_t)t;
}
static const uint32_t *hetero_offsets(sam::Batch *b, int l, int r, const char *who) { // &off[l][r]
  auto &E = Engine::Get();
  SAM_CHECK(l >= 0 && (size_t)l < E.cfg.fanout.size(), std::string(who) + ": no such layer");
  SAM_CHECK(r >= 0 && (uint32_t)r < E.cfg.num_edge_type, std::string(who) + ": no such relation");
  return b->het_words + E.HetOffsetsAt() + (size_t)l * (E.cfg.num_edge_type + 1) + (size_t)r;
}
static void hetero_nodes_tensor(uint64_t key, const char *who, int which, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, who);
  void *p = which == 0 ? (void *)b->het_ntype : which == 1 ? (void *)b->het_local : (void *)b->het_slot;
  fill(out, p, (int64_t)b->num_input, 1, 1, which == 0 ? GGMS_U8 : GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_node_type(uint64_t key, samgraph_tensor_t *out) { hetero_nodes_tensor(key, "samgraph_get_graph_node_type", 0, out); }
void samgraph_get_graph_node_local(uint64_t key, samgraph_tensor_t *out) { hetero_nodes_tensor(key, "samgraph_get_graph_node_local", 1, out); }
void samgraph_get_graph_node_slot(uint64_t key, samgraph_tensor_t *out) { hetero_nodes_tensor(key, "samgraph_get_graph_node_slot", 2, out); }
void samgraph_get_graph_typed_nodes(uint64_t key, int t, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, "samgraph_get_graph_typed_nodes");
  const uint32_t *base = b->het_words + E.HetBaseAt() + hetero_type(t, "samgraph_get_graph_typed_nodes");
  fill(out, b->het_typed + base[0], (int64_t)(base[1] - base[0]), 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_feat_of_type(uint64_t key, int t, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, "samgraph_get_graph_feat_of_type");
  const uint32_t *base = b->het_words + E.HetBaseAt() + hetero_type(t, "samgraph_get_graph_feat_of_type");
  if (E.cfg.typed_feat) { // the type's block of the buffer, at its offset word: (cnt_t, dim_t) in the type's delivered dtype
    fill(out, (char *)b->feat + b->het_off[t], (int64_t)(base[1] - base[0]), (int64_t)E.ds.node_feat[t].dim, 2,
         E.typed_feat_dtype((size_t)t), E.batch_device_type(), E.trainer_device());
    return;
  }
  fill(out, (char *)b->feat + (size_t)base[0] * E.batch_feat_row_bytes(), (int64_t)(base[1] - base[0]), (int64_t)E.ds.feat_dim, 2,
       E.batch_feat_dtype(), E.batch_device_type(), E.trainer_device());
}
size_t samgraph_get_graph_num_src_of_type(uint64_t key, int l, int t) {
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, "samgraph_get_graph_num_src_of_type");
  SAM_CHECK(l >= 0 && (size_t)l < E.cfg.fanout.size(), "samgraph_get_graph_num_src_of_type: no such layer");
  return b->het_words[E.HetCutsAt() + (size_t)l * E.ds.num_node_type + hetero_type(t, "samgraph_get_graph_num_src_of_type")];
}
size_t samgraph_get_graph_num_dst_of_type(uint64_t key, int l, int t) { // num_dst(l) = num_src(l + 1); the last: its own cut
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, "samgraph_get_graph_num_dst_of_type");
  SAM_CHECK(l >= 0 && (size_t)l < E.cfg.fanout.size(), "samgraph_get_graph_num_dst_of_type: no such layer");
  return b->het_words[E.HetCutsAt() + (size_t)(l + 1) * E.ds.num_node_type + hetero_type(t, "samgraph_get_graph_num_dst_of_type")];
}
static void hetero_rel_tensor(uint64_t key, int l, int r, const char *who, int which, samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  auto *b = hetero_batch(key, who);
  const uint32_t *off = hetero_offsets(b, l, r, who);
  uint32_t *p = (which == 0 ? b->het_row : which == 1 ? b->het_col : b->het_eid)[l];
  fill(out, p + off[0], (int64_t)(off[1] - off[0]), 1, 1, GGMS_I32, E.batch_device_type(), E.trainer_device());
}
void samgraph_get_graph_rel_row(uint64_t key, int l, int r, samgraph_tensor_t *out) { hetero_rel_tensor(key, l, r, "samgraph_get_graph_rel_row", 0, out); }
void samgraph_get_graph_rel_col(uint64_t key, int l, int r, samgraph_tensor_t *out) { hetero_rel_tensor(key, l, r, "samgraph_get_graph_rel_col", 1, out); }
void samgraph_get_graph_rel_edge_ids(uint64_t key, int l, int r, samgraph_tensor_t *out) { hetero_rel_tensor(key, l, r, "samgraph_get_graph_rel_edge_ids", 2, out); }
size_t samgraph_get_graph_rel_num_edges(uint64_t key, int l, int r) {
  auto *b = hetero_batch(key, "samgraph_get_graph_rel_num_edges");
  const uint32_t *off = hetero_offsets(b, l, r, "samgraph_get_graph_rel_num_edges");
  return off[1] - off[0];
}
// config key typed_feat: one feature table per node type
static size_t typed_feat_type(int t, const char *who) {
  auto &E = Engine::Get();
  if (!E.cfg.typed_feat) sam::fatal(__FILE__, __LINE__, std::string(who) + " needs the config key typed_feat = on");
  SAM_CHECK(t >= 0 && (size_t)t < E.ds.node_feat.size(), std::string(who) + ": no such node type");
  return (size_t)t;
}
size_t samgraph_feat_dim_of_type(int t) { return Engine::Get().ds.node_feat[typed_feat_type(t, "samgraph_feat_dim_of_type")].dim; }
int samgraph_feat_dtype_of_type(int t) { return Engine::Get().typed_feat_dtype(typed_feat_type(t, "samgraph_feat_dtype_of_type")); }
size_t samgraph_num_node_type(void) {
  hetero_need("samgraph_num_node_type");
  return Engine::Get().ds.num_node_type;
}
int samgraph_relation_src_type(int r) {
  hetero_need("samgraph_relation_src_type");
  auto &E = Engine::Get();
  SAM_CHECK(r >= 0 && (size_t)r < E.ds.rel_src_type.size(), "samgraph_relation_src_type: no such relation");
  return E.ds.rel_src_type[r];
}
int samgraph_relation_dst_type(int r) {
  hetero_need("samgraph_relation_dst_type");
  auto &E = Engine::Get();
  SAM_CHECK(r >= 0 && (size_t)r < E.ds.rel_dst_type.size(), "samgraph_relation_dst_type: no such relation");
  return E.ds.rel_dst_type[r];
}
// config key feat_learnable: the gradient of the current batch's rows moves the table; the live table and its state
void samgraph_update_graph_feat(uint64_t key, const void *grad, size_t num_rows, size_t dim, void *caller_stream) {
  Engine::Get().UpdateGraphFeat(key, grad, num_rows, dim, (hipStream_t)caller_stream);
}
void samgraph_get_store_feat(samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  fill(out, E.StoreFeat("samgraph_get_store_feat"), (int64_t)E.ds.num_node, (int64_t)E.ds.feat_dim, 2, GGMS_F32, 2, E.trainer_device());
}
void samgraph_get_store_state(samgraph_tensor_t *out) {
  auto &E = Engine::Get();
  fill(out, E.StoreState("samgraph_get_store_state"), (int64_t)E.ds.num_node, (int64_t)E.ds.feat_dim, 2, GGMS_F32, 2, E.trainer_device());
}
size_t samgraph_num_negative(void) { return Engine::Get().cfg.link_prediction ? Engine::Get().cfg.num_negative : 0; }
void samgraph_batch_retain(uint64_t key) { Engine::Get().Retain(key); }
void samgraph_batch_release(uint64_t key) { Engine::Get().Release(key); }

} // extern "C"
