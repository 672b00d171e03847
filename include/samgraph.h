/*
 * samgraph.h -- engine-level C ABI: the `samgraph_*` surface the reference's
 * Python packages bind (ctypes in samgraph/common/__init__.py:279-537, pybind11
 * in samgraph/torch/adapter.cc:195-206), exported by the same libggms_hip.so.
 *
 * Same names, argument meaning and error behaviour as
 * /root/reference/samgraph/common/operation.h:30-115 (citations below are
 * relative to /root/reference/samgraph/): configuration is a string map,
 * failures print and abort() the process (logging.cc:69-73), the engine is a
 * process-wide singleton with one "current batch".
 *
 * What differs, on purpose:
 *   - the nine pybind11 functions that returned torch::Tensor (adapter.cc:62-193)
 *     are plain C here: they fill a samgraph_tensor_t {pointer, shape, dtype,
 *     device}; the Python side wraps it zero-copy (__cuda_array_interface__).
 *     No torch type crosses the boundary;
 *   - batch buffers are reference counted explicitly (samgraph_batch_retain /
 *     _release) instead of through a captured shared_ptr (adapter.cc:70-73);
 *   - extra config keys (all optional): "seed" (RNG + shuffler seed; default =
 *     wall clock like the reference), "hash_table" = "direct" | "hashed".
 */
#ifndef SAMGRAPH_ABI_H
#define SAMGRAPH_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- configuration / lifecycle: common/operation.h:30-43, 96-113 --------- */
void samgraph_config(const char **config_keys, const char **config_values,
                     const size_t num_config_items);   /* operation.cc:49-62  */
void samgraph_init(void);                               /* :328-335 (single process: arch1) */
void samgraph_start(void);                              /* :337-345 */
void samgraph_shutdown(void);                           /* :392-398 */
void samgraph_data_init(void);                          /* :509-533 (parent, before fork)   */
void samgraph_sample_init(int worker_id, const char *ctx);  /* :535-540 */
void samgraph_train_init(int worker_id, const char *ctx);   /* :549-554 */
void samgraph_extract_start(int count);                     /* :556-559 */
int samgraph_wait_one_child(void);                          /* :573-584 */
void samgraph_forward_barrier(void);                        /* :507     */
/* Entry points of deployments this build does not carry (arch9 unified-memory sampling, arch5 switcher;
 * operation.cc:541-547,561-571): exported so that the reference's loader binds, they abort with a message
 * like any unsupported configuration (logging.cc:69-73). */
void samgraph_um_sample_init(int num_workers);
void samgraph_switch_init(int worker_id, const char *ctx, double cache_percentage);

/* ---- queries: operation.h:45-63 ------------------------------------------ */
size_t samgraph_num_epoch(void);
size_t samgraph_steps_per_epoch(void);
size_t samgraph_num_local_step(void);
size_t samgraph_num_class(void);
size_t samgraph_feat_dim(void);
/* an extension: bytes of one feature row -- delivered == 0: as STORED in the table, the cache, its shards and replicas
 * (feat_dim x the table's element bytes; a Q8ROW row's codes, pad and trailer); else as DELIVERED in a batch
 * (feat_dim x the batch dtype's element bytes: feat_out_dtype, or the table's dtype without the key) */
size_t samgraph_feat_row_bytes(int delivered);
uint64_t samgraph_get_next_batch(void);                 /* :366-378 */
void samgraph_sample_once(void);                        /* :380     */
size_t samgraph_get_graph_num_src(uint64_t key, int graph_id);
size_t samgraph_get_graph_num_dst(uint64_t key, int graph_id);
size_t samgraph_get_graph_num_edge(uint64_t key, int graph_id);

/* ---- profiler / trace: operation.h:65-94; item codes = common/profiler.h:30-163
 * (mirrored by name in xgnn_amd/common.py) -------------------------------- */
void samgraph_log_step(uint64_t epoch, uint64_t step, int item, double val);
void samgraph_log_step_by_key(uint64_t key, int item, double val);
void samgraph_log_step_add(uint64_t epoch, uint64_t step, int item, double val);
void samgraph_log_epoch_add(uint64_t epoch, int item, double val);
double samgraph_get_log_init_value(int item);
double samgraph_get_log_step_value(uint64_t epoch, uint64_t step, int item);
double samgraph_get_log_step_value_by_key(uint64_t key, int item);
double samgraph_get_log_epoch_value(uint64_t epoch, int item);
void samgraph_report_init(void);
void samgraph_report_step(uint64_t epoch, uint64_t step);
void samgraph_report_step_average(uint64_t epoch, uint64_t step);
void samgraph_report_epoch(uint64_t epoch);
void samgraph_report_epoch_average(uint64_t epoch);
void samgraph_report_node_access(void);
void samgraph_trace_step_begin(uint64_t key, int item, uint64_t ts);
void samgraph_trace_step_end(uint64_t key, int item, uint64_t ts);
void samgraph_trace_step_begin_now(uint64_t key, int item);
void samgraph_trace_step_end_now(uint64_t key, int item);
void samgraph_dump_trace(void);

/* ---- tensor hand-off: torch/adapter.cc:62-193 ---------------------------- */
typedef struct {
  void *data;
  int64_t shape[2];
  int32_t ndim;
  int32_t dtype;       /* ggms_dtype / DataType code (common/common.h:38-46) */
  int32_t device_type; /* 0 = host, 2 = GPU (DeviceType, common.h:48)       */
  int32_t device_id;
} samgraph_tensor_t;

/* each checks key == current batch key like CHECK_EQ(key, graph_batch->key) (adapter.cc:68) */
void samgraph_get_graph_feat(uint64_t key, samgraph_tensor_t *out);              /* :62-77; dtype: config key feat_out_dtype, else the table's */
void samgraph_get_graph_label(uint64_t key, samgraph_tensor_t *out);             /* :79-92   */
void samgraph_get_graph_row(uint64_t key, int layer_idx, samgraph_tensor_t *out);/* :94-106  */
void samgraph_get_graph_col(uint64_t key, int layer_idx, samgraph_tensor_t *out);/* :108-120 */
void samgraph_get_graph_data(uint64_t key, int layer_idx, samgraph_tensor_t *out);/* :122-134 */
void samgraph_get_dataset_feat(samgraph_tensor_t *out);                          /* :136-152 */
void samgraph_get_dataset_label(samgraph_tensor_t *out);                         /* :154-167 */
void samgraph_get_graph_input_nodes(uint64_t key, samgraph_tensor_t *out);       /* :169-180 */
void samgraph_get_graph_output_nodes(uint64_t key, samgraph_tensor_t *out);      /* :182-193 */
/* Extensions for config key task = link_prediction (arch1; keys num_negative = 1 .. 64, negative_mode = uniform |
 * exclude).  A batch is B = batch_size positive edges of the shuffled train edge set (train_edge_set.bin: uint32
 * positions in indices.bin; absent: every edge) with K = num_negative negative destinations each (ggms_link_seeds,
 * include/ggms.h).  Its output nodes are the B (2 + K) endpoints: [0, B) sources, [B, 2 B) destinations,
 * [2 B + i K + j] negative j of positive i.  samgraph_get_graph_seed_ids gives the LOCAL id of each of them (uint32
 * ids as I32, B (2 + K) entries, same layout): the ids the first sampled layer's col uses, rows of the batch's input
 * nodes and of its feature tensor.  samgraph_num_negative: K, or 0 for a node_classification run.
 * Config key exclude_seed_edges = none | self | both (read with the task only): the batch's positive edges (u -> v), and
 * with `both` their mirrors (v -> u), are removed from every sampled layer on the device (ggms_drop_pair_edges) before
 * the batch is handed out: samgraph_get_graph_row / _col / _num_edge show the filtered layers, num_src / num_dst and the
 * node lists are unchanged.  samgraph_get_graph_num_excluded: the edges removed from this batch, all layers together
 * (0 without the key). */
void samgraph_get_graph_seed_ids(uint64_t key, samgraph_tensor_t *out);
size_t samgraph_num_negative(void);
size_t samgraph_get_graph_num_excluded(uint64_t key);
/* Extensions for config key feat_learnable = sgd | adagrad (arch1, FEAT_DATA_TYPE F32; with it feat_lr: required,
 * finite; feat_eps: Adagrad only, default 1e-10, > 0).  The table on the device is LEARNABLE: it starts as feat.bin, and
 *   samgraph_update_graph_feat(key, grad, num_rows, dim, caller_stream)   applies ggms_update_rows' rule (include/ggms.h)
 *     to the table rows of the CURRENT batch's input nodes: grad is device memory, F32, (num_rows, dim) contiguous, row i
 *     the gradient of row i of samgraph_get_graph_feat(key), produced on caller_stream (a hipStream_t).  Another shape
 *     than (the batch's num_input, feat_dim) is fatal.  Nothing waits on the host: caller_stream is tied in by events on
 *     both sides, so the gradient's memory may be released to a stream-ordered allocator right after the call.
 * Gathers and updates run on ONE stream (extract_streams is forced to 1), in the order of the calls that enqueue them:
 * a batch's rows reflect exactly the updates whose call came before the samgraph_sample_once call that enqueued the
 * batch.  With lookahead = h and the loop {sample_once; get_next_batch; train; update}, batch j sees the updates of
 * batches 0 .. j-h-1; lookahead = 0 is fully synchronous.  A row is never torn.  samgraph_extract_start is fatal with
 * the key (a background thread would make that a matter of timing).
 *   samgraph_get_store_feat / samgraph_get_store_state   the live table and the Adagrad accumulator, (num_node, dim) F32
 *     on the trainer GPU, zero-copy; fatal without the key (the state: without adagrad).  samgraph_get_dataset_feat
 *     keeps returning the mapped file. */
void samgraph_update_graph_feat(uint64_t key, const void *grad, size_t num_rows, size_t dim, void *caller_stream);
void samgraph_get_store_feat(samgraph_tensor_t *out);
void samgraph_get_store_state(samgraph_tensor_t *out);
/* Extensions for config keys edge_ids = on and edge_feat = on (arch1, one CSR; refused by name with every other
 * deployment, use_dist_graph, random_walk and khop2; edge_feat implies edge_ids).  Behind the sampler -- and behind
 * exclude_seed_edges' filter -- ggms_edge_positions (include/ggms.h) computes for every edge of every layer its position
 * in indices.bin: the id edge data is stored under, and the id space of train_edge_set.bin.
 *   samgraph_get_graph_edge_ids(key, layer)    num_edge(layer) positions, uint32 bits in samgraph_get_graph_row's dtype;
 *     indices[id] is the global id of the edge's row node, the edge lies in the list of its col node.  Parallel edges all
 *     carry the first copy's position.
 *   samgraph_get_graph_edge_feat(key, layer)   with edge_feat: (num_edge(layer), EDGE_FEAT_DIM) rows of edge_feat.bin
 *     (NUM_EDGE rows in CSR order, uploaded to the GPU at init; meta.txt: EDGE_FEAT_DIM and, optionally,
 *     EDGE_FEAT_DATA_TYPE -- F32 without it, any element type, not Q8ROW), row k = table[edge_ids[k]], in the table's
 *     dtype: feat_out_dtype does not apply.  A missing file or meta key and a file of another size are fatal at init.
 *   samgraph_get_graph_link_edge_ids(key)      task = link_prediction (no other key needed): the batch's B positive
 *     edge ids, what a rating or label per positive is looked up with.
 * Without the keys nothing runs and nothing is allocated; the first two accessors are then fatal. */
void samgraph_get_graph_edge_ids(uint64_t key, int layer_idx, samgraph_tensor_t *out);
void samgraph_get_graph_edge_feat(uint64_t key, int layer_idx, samgraph_tensor_t *out);
void samgraph_get_graph_link_edge_ids(uint64_t key, samgraph_tensor_t *out);
/* Extensions for config key induced_subgraph = on (arch1, one CSR, both tasks, any number of pipelines, both table
 * layouts; refused by name with every other deployment, use_dist_graph, khop2, khop_temporal and exclude_seed_edges other
 * than none).  Behind the sampler, ggms_induced_edges (include/ggms.h) computes the subgraph the batch's input nodes
 * induce: EVERY edge of the graph with both ends among them (ShaDow-GNN, GraphSAINT's node sampler, Cluster-GCN), one COO
 * over the batch's local ids -- rows of samgraph_get_graph_feat, like every layer's -- in (col, CSR position) order.
 *   samgraph_get_graph_num_induced(key)          M, the number of induced edges
 *   samgraph_get_graph_induced_row / _col(key)   M local ids each: row = the neighbour, col = the node whose list holds
 *     the edge (samgraph_get_graph_row's convention and dtype).  Parallel edges are each there, self-loops too.
 *   samgraph_get_graph_induced_edge_ids(key)     M CSR positions (each edge its own), the id space of edge_ids
 *   samgraph_get_graph_induced_edge_feat(key)    with edge_feat = on as well: (M, EDGE_FEAT_DIM), row k = table[ids[k]]
 * induced_max_edges (optional, 1 .. 2^32 - 1025): the capacity of a batch's induced arrays.  Default: the sum of the
 * layers' edge capacities (what the sampled layers could hold at most), capped at NUM_EDGE -- a capacity, not a
 * measurement.  A batch that induces more is fatal, with the key and the count it needed.
 * Without the key nothing runs and nothing is allocated; the accessors are then fatal. */
size_t samgraph_get_graph_num_induced(uint64_t key);
void samgraph_get_graph_induced_row(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_induced_col(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_induced_edge_ids(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_induced_edge_feat(uint64_t key, samgraph_tensor_t *out);
/* Extensions for _sample_type 9 (khop_temporal; config key temporal_pick = uniform | recent; arch1 with task =
 * link_prediction and one CSR -- every other deployment, task = node_classification, use_dist_graph and
 * exclude_seed_edges other than none are refused by name).  The dataset carries edge_time.bin: NUM_EDGE uint32, one per
 * position of indices.bin, non-decreasing inside every node's list (size and order are checked at init, fatal with the
 * node).  Every entry of a batch's seed list is sampled strictly BEFORE the time of its positive edge, a node reached
 * under several times before the smallest of them (ggms_sample_batch_temporal, include/ggms.h).  edge_ids is implied:
 * the sampler emits the positions itself -- parallel edges carry their OWN position -- and edge_feat gathers under them.
 *   samgraph_get_graph_edge_time(key, layer)   num_edge(layer) times, edge_time[edge_ids[k]]
 *   samgraph_get_graph_node_cut(key)           one cut-off per input node (the final one): what a time encoding of an
 *                                              edge, cut[col] - edge_time, is taken against
 *   samgraph_get_graph_link_time(key)          the times of the batch's B positive edges
 * All three: uint32 bits in samgraph_get_graph_row's dtype; fatal with every other sample type. */
void samgraph_get_graph_edge_time(uint64_t key, int layer_idx, samgraph_tensor_t *out);
void samgraph_get_graph_node_cut(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_link_time(uint64_t key, samgraph_tensor_t *out);
/* Extension for _sample_type 10 (khop_typed; config key type_fanout = num_layer x NUM_EDGE_TYPE integers, layer-major, each
 * 0 .. 127, no all-zero row; `fanout` must hold the rows' sums -- the Python front-end fills it in from a list of lists).
 * arch1 with one CSR, task = node_classification or link_prediction, 1 or 2 pipelines; every other deployment,
 * use_dist_graph and exclude_seed_edges other than none are refused by name.  The dataset carries edge_type.bin
 * (NUM_EDGE uint8, one per position of indices.bin, non-decreasing inside every node's list) and the meta key
 * NUM_EDGE_TYPE (1 .. 32); size, order and range are checked at init, fatal with the node.  Every layer samples
 * min(k_r, e_r) edges of every relation r per node (ggms_sample_batch_typed, include/ggms.h).  edge_ids is implied: the
 * sampler emits the positions itself -- parallel edges of different relations carry their OWN position -- and edge_feat
 * gathers under them.
 *   samgraph_get_graph_edge_type(key, layer)   num_edge(layer) types (uint8), edge_type[edge_ids[k]]
 * Fatal with every other sample type. */
void samgraph_get_graph_edge_type(uint64_t key, int layer_idx, samgraph_tensor_t *out);
/* Extensions for config key hetero_batch = on (arch1 with _sample_type 10, both tasks, 1 or 2 pipelines, both table
 * layouts; refused by name with every other deployment, every other sample type, edge_feat, induced_subgraph,
 * feat_learnable and use_dist_graph).  The dataset carries node_type.bin (NUM_NODE uint8, one per node id) and the meta key
 * NUM_NODE_TYPE = T (1 .. 32); a missing file, another size and a value >= T are fatal at init, and so is a relation whose
 * edges disagree about (source type, destination type) -- named with both signatures.  Behind the sampler,
 * ggms_hetero_nodes and ggms_hetero_edges (include/ggms.h) group the batch's input nodes by type and every layer's edges
 * by relation; an edge's ends become ranks inside their types' groups.  Direction as everywhere: col is the edge's
 * destination (the node whose list was read), row its source.
 * THE FEATURE ROWS FOLLOW THE GROUPED ORDER: with the key, row s of samgraph_get_graph_feat belongs to
 * typed_nodes[s] -- the gather is handed the grouped list in place of the input nodes, same count, same kernel, no second
 * pass over the rows -- so a type's rows are one contiguous slice.  Labels, pair ids and the homogeneous row / col /
 * edge_ids / edge_type are untouched and keep indexing the input nodes; node_slot maps an input-node index to its feature
 * row, node_local to its rank inside its type.
 *   samgraph_get_graph_node_type(key)             one uint8 per input node
 *   samgraph_get_graph_node_local / _slot(key)    one id per input node: the rank inside its type; base[type] + that rank
 *   samgraph_get_graph_typed_nodes(key, t)        the global ids of type t, in batch order (a slice of the grouped list)
 *   samgraph_get_graph_feat_of_type(key, t)       their rows: a VIEW of samgraph_get_graph_feat's buffer, not a copy
 *   samgraph_get_graph_num_src_of_type / _num_dst_of_type(key, layer, t)   how many of the layer's source / destination
 *     nodes have type t: they are the first that many of the type's group (the layers' node sets are nested prefixes)
 *   samgraph_get_graph_rel_row / _rel_col / _rel_edge_ids(key, layer, r)   relation r's edges of the layer in the
 *     sampler's order: source ranks, destination ranks, CSR positions (slices of the partitioned arrays)
 *   samgraph_get_graph_rel_num_edges(key, layer, r)
 *   samgraph_num_node_type(), samgraph_relation_src_type(r), samgraph_relation_dst_type(r)   T and the relation table
 *     derived at init (255 / 255 for a relation without an edge)
 * Without the key nothing runs and nothing is allocated; every accessor above is then fatal. */
void samgraph_get_graph_node_type(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_node_local(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_node_slot(uint64_t key, samgraph_tensor_t *out);
void samgraph_get_graph_typed_nodes(uint64_t key, int node_type, samgraph_tensor_t *out);
void samgraph_get_graph_feat_of_type(uint64_t key, int node_type, samgraph_tensor_t *out);
size_t samgraph_get_graph_num_src_of_type(uint64_t key, int layer_idx, int node_type);
size_t samgraph_get_graph_num_dst_of_type(uint64_t key, int layer_idx, int node_type);
void samgraph_get_graph_rel_row(uint64_t key, int layer_idx, int relation, samgraph_tensor_t *out);
void samgraph_get_graph_rel_col(uint64_t key, int layer_idx, int relation, samgraph_tensor_t *out);
void samgraph_get_graph_rel_edge_ids(uint64_t key, int layer_idx, int relation, samgraph_tensor_t *out);
size_t samgraph_get_graph_rel_num_edges(uint64_t key, int layer_idx, int relation);
size_t samgraph_num_node_type(void);
int samgraph_relation_src_type(int relation);
int samgraph_relation_dst_type(int relation);
/* Extensions for config key typed_feat = on (needs hetero_batch = on, and through it arch1 with _sample_type 10): the
 * feature store is one table PER NODE TYPE.  The dataset carries, for every type t below NUM_NODE_TYPE, the meta keys
 * NODE_FEAT_DIM_<t> (0: the type has no features) and NODE_FEAT_DATA_TYPE_<t> (F32, F16 or BF16), and node_feat_<t>.bin
 * for every type with a table: one row per node of the type, row k that of the type's k-th node in ascending node id
 * (datagen.write_dataset(node_feat=[...])).  A missing key or file and a file of another size than (nodes of type t) x
 * dim x element size are fatal at init, by name and with both numbers.  feat.bin is neither mapped nor uploaded.  Refused
 * by name: typed_feat without hetero_batch, with feat_learnable, with feat_store_dtype, with SAMGRAPH_EMPTY_FEAT /
 * SAMGRAPH_FAKE_FEAT_DIM, and a table type outside the three.  A batch's rows are gathered by ggms_gather_typed
 * (include/ggms.h) over the grouped node list into per-type blocks of ONE buffer, every block 16-byte aligned;
 * feat_out_dtype sets every type's delivered dtype, without it every type arrives in its own.
 *   samgraph_get_graph_feat_of_type(key, t)   (nodes of type t in the batch, dim_t) in type t's delivered dtype: a VIEW of
 *     the batch's buffer at the type's offset word, not a copy; (cnt_t, 0) for a type without a table
 *   samgraph_feat_dim_of_type(t), samgraph_feat_dtype_of_type(t)   the type's row width; its delivered ggms_dtype code
 *   samgraph_get_graph_feat(key)              fatal by name: there is no single matrix
 * Without the key nothing is allocated, enqueued or changed, and the two new entry points are fatal. */
size_t samgraph_feat_dim_of_type(int node_type);
int samgraph_feat_dtype_of_type(int node_type);
/* a batch's buffers stay valid while its retain count is > 0 */
void samgraph_batch_retain(uint64_t key);
void samgraph_batch_release(uint64_t key);

#ifdef __cplusplus
}
#endif
#endif /* SAMGRAPH_ABI_H */
