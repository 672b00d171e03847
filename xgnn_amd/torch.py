"""Mirror of the reference's ``samgraph.torch`` adapter (/root/reference/samgraph/torch/adapter.py:63-218):
the same function names; tensors are zero-copy views of engine-owned device buffers.

The reference's pybind11 module returned torch::from_blob tensors whose deleter captured the buffer
(adapter.cc:62-77).  Here the C ABI hands back {pointer, shape, dtype, device}; the view goes through
``__cuda_array_interface__`` and the wrapper object holds a retain on the batch until the tensor dies.
"""
import ctypes as C

import numpy as np
import torch

from .common import *  # noqa: F401,F403  (enum mirrors, like `from samgraph.common import *`)
from .common import _basics, Tensor as _CTensor

for _name in ("init start num_class feat_dim num_epoch steps_per_epoch get_next_batch get_graph_num_src "
              "get_graph_num_dst get_graph_num_edge shutdown sample_once log_step log_step_add log_epoch_add "
              "get_log_init_value get_log_step_value get_log_epoch_value report_init report_step report_step_average "
              "report_epoch report_epoch_average report_node_access trace_step_begin trace_step_end "
              "trace_step_begin_now trace_step_end_now dump_trace forward_barrier wait_one_child log_step_by_key "
              "get_log_step_value_by_key data_init sample_init train_init extract_start num_local_step "
              "um_sample_init switch_init feat_row_bytes num_negative get_graph_num_excluded "
              "get_graph_num_induced get_graph_num_src_of_type get_graph_num_dst_of_type get_graph_rel_num_edges "
              "num_node_type relation_src_type relation_dst_type feat_dim_of_type").split():
    globals()[_name] = getattr(_basics, _name)

# DataType code -> (numpy typestr, torch dtype); common/common.h:38-46, adapter.cc:33-53
_DT = {0: ("<f4", torch.float32), 1: ("<f8", torch.float64), 2: ("<f2", torch.float16), 3: ("|u1", torch.uint8),
       4: ("<i4", torch.int32), 5: ("|i1", torch.int8), 6: ("<i8", torch.int64),
       # GGMS_BF16 (an extension): neither numpy nor the CUDA array interface has a bf16 typestr, so the buffer is
       # viewed as 16-bit integers and re-viewed as bfloat16 (_as_dtype)
       7: ("<i2", torch.bfloat16),
       # GGMS_F8E4M3 / GGMS_F8E5M2 (extensions): the OCP 8-bit floats have no typestr either -- bytes, re-viewed
       16: ("|u1", torch.float8_e4m3fn), 17: ("|u1", torch.float8_e5m2)}
# (GGMS_Q8ROW = 18 is a row format with no element type: never a batch's dtype -- the engine refuses such a table without
# feat_out_dtype -- and get_dataset_feat reports the stored rows as uint8 of shape (rows, ggms_row_bytes), code 3)
_FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)

# config key `feat_out_dtype` or `feat_store_dtype` was given (the caller chose the batch's dtype, or asked for a narrow
# store and gets its type): get_graph_feat hands the rows out as the gather delivered them
_feat_as_delivered = False


def config(run_config):
    global _feat_as_delivered
    _feat_as_delivered = "feat_out_dtype" in run_config or "feat_store_dtype" in run_config
    return _basics.config(run_config)


def _as_dtype(tensor, code):
    return tensor.view(_DT[code][1]) if code in (7, 16, 17) else tensor


class _DeviceView(object):
    """Zero-copy view of an engine buffer; keeps the batch alive (adapter.cc:70-73 deleter capture)."""

    def __init__(self, t, key):
        shape = tuple(int(t.shape[i]) for i in range(t.ndim))
        self._key = key
        self.__cuda_array_interface__ = {"shape": shape, "typestr": _DT[t.dtype][0],
                                         "data": (int(t.data or 0), False), "version": 2, "strides": None}
        if key is not None:
            _basics.C_LIB_CTYPES.samgraph_batch_retain(key)

    def __del__(self):
        if getattr(self, "_key", None) is not None:
            try:
                _basics.C_LIB_CTYPES.samgraph_batch_release(self._key)
            except Exception:
                pass


def _wrap(t, key):
    n = 1
    for i in range(t.ndim):
        n *= int(t.shape[i])
    if t.device_type == 2:
        dev = torch.device("cuda", t.device_id)
        if n == 0:
            return torch.empty(tuple(int(t.shape[i]) for i in range(t.ndim)), dtype=_DT[t.dtype][1], device=dev)
        return _as_dtype(torch.as_tensor(_DeviceView(t, key), device=dev), t.dtype)  # (a view: the retain stays with it)
    # host memory: numpy view over the mapped dataset file (GetDatasetFeature, adapter.cc:136-152)
    shape = tuple(int(t.shape[i]) for i in range(t.ndim))
    if n == 0 or not t.data:
        return torch.empty(shape, dtype=_DT[t.dtype][1])
    buf = (C.c_char * (n * np.dtype(_DT[t.dtype][0]).itemsize)).from_address(t.data)
    a = np.frombuffer(buf, dtype=_DT[t.dtype][0]).reshape(shape)
    # a batch of the CPU deployment (arch0, host trainer) lives in a slot the engine reuses: hand out a copy;
    # the dataset tensors (key None) stay zero-copy views of the mapped files
    return _as_dtype(torch.from_numpy(a.copy() if key is not None else a), t.dtype)


def _get(fn, key, *args):
    t = _CTensor()
    getattr(_basics.C_LIB_CTYPES, fn)(*((key,) if key is not None else ()), *args, C.byref(t))
    return _wrap(t, key)


def get_graph_feat(batch_key):
    batch_feat = _get("samgraph_get_graph_feat", batch_key)
    # without the key an F16 / BF16 / integer table is cast to float32 here, as the reference's adapter does; an FP8
    # table's rows stay the bytes the gather moved (decoding is the gather's job: feat_out_dtype)
    if not _feat_as_delivered and batch_feat.dtype != torch.float32 and batch_feat.dtype not in _FP8:
        batch_feat = batch_feat.float()
    return batch_feat


def get_graph_label(batch_key): return _get("samgraph_get_graph_label", batch_key)
def get_graph_row(batch_key, layer_idx): return _get("samgraph_get_graph_row", batch_key, layer_idx)
def get_graph_col(batch_key, layer_idx): return _get("samgraph_get_graph_col", batch_key, layer_idx)
def get_graph_data(batch_key, layer_idx): return _get("samgraph_get_graph_data", batch_key, layer_idx)
def get_dataset_feat(): return _get("samgraph_get_dataset_feat", None)
def get_dataset_label(): return _get("samgraph_get_dataset_label", None)
def get_graph_input_nodes(batch_key): return _get("samgraph_get_graph_input_nodes", batch_key)
def get_graph_output_nodes(batch_key): return _get("samgraph_get_graph_output_nodes", batch_key)


def get_graph_seed_ids(batch_key): return _get("samgraph_get_graph_seed_ids", batch_key)


def get_graph_edge_ids(batch_key, layer_idx):
    """Config key edge_ids (or edge_feat): the CSR position of every edge of the layer (DGL's dgl.EID, PyG's e_id), int32
    holding the uint32 bits -- the index edge data is stored under, and the id space of get_graph_link_edge_ids."""
    return _get("samgraph_get_graph_edge_ids", batch_key, layer_idx)


def get_graph_edge_feat(batch_key, layer_idx):
    """Config key edge_feat: (num_edge, EDGE_FEAT_DIM) rows of the dataset's edge table, row k that of edge k of the
    layer, in the table's dtype."""
    return _get("samgraph_get_graph_edge_feat", batch_key, layer_idx)


def get_graph_induced_row(batch_key):
    """Config key induced_subgraph: the neighbour end of every edge the batch's input nodes induce -- every edge of the
    graph with both ends among them -- as a local id (a row of get_graph_feat), get_graph_num_induced of them."""
    return _get("samgraph_get_graph_induced_row", batch_key)


def get_graph_induced_col(batch_key):
    """Config key induced_subgraph: the local id of the node whose list holds the induced edge (get_graph_col's side)."""
    return _get("samgraph_get_graph_induced_col", batch_key)


def get_graph_induced_edge_ids(batch_key):
    """Config key induced_subgraph: the CSR position of every induced edge (int32 holding the uint32 bits); parallel
    edges carry their own."""
    return _get("samgraph_get_graph_induced_edge_ids", batch_key)


def get_graph_induced_edge_feat(batch_key):
    """Config keys induced_subgraph and edge_feat: (num_induced, EDGE_FEAT_DIM) rows of the edge table, row k that of
    induced edge k."""
    return _get("samgraph_get_graph_induced_edge_feat", batch_key)


def get_graph_node_type(batch_key):
    """Config key hetero_batch: the node type of every input node (uint8)."""
    return _get("samgraph_get_graph_node_type", batch_key)


def get_graph_node_local(batch_key):
    """Config key hetero_batch: per input node its rank inside its type -- the id the per-relation blocks use."""
    return _get("samgraph_get_graph_node_local", batch_key)


def get_graph_node_slot(batch_key):
    """Config key hetero_batch: per input node the row of get_graph_feat that holds its features (with the key the rows
    are grouped by type): base[type] + node_local.  Labels, seed ids and the homogeneous row / col index input nodes;
    this maps them to the typed view."""
    return _get("samgraph_get_graph_node_slot", batch_key)


def get_graph_typed_nodes(batch_key, node_type):
    """Config key hetero_batch: the global ids of the batch's nodes of one type, in batch order."""
    return _get("samgraph_get_graph_typed_nodes", batch_key, node_type)


def get_graph_feat_of_type(batch_key, node_type):
    """Config key hetero_batch: the feature rows of get_graph_typed_nodes(key, t), a view of get_graph_feat's buffer (a
    type's rows are one contiguous slice), in the dtype the gather delivered.  With typed_feat = on: the type's own block,
    (nodes of the type, feat_dim_of_type(t)) in feat_dtype_of_type(t), a view of the batch's buffer; (n, 0) for a type
    without a table."""
    return _get("samgraph_get_graph_feat_of_type", batch_key, node_type)


def feat_dtype_of_type(node_type):
    """Config key typed_feat: the torch dtype type t's rows are delivered in (feat_out_dtype, else the table's own)."""
    return _DT[_basics.feat_dtype_code_of_type(node_type)][1]


def get_graph_rel_row(batch_key, layer_idx, relation):
    """Config key hetero_batch: the source end of every edge of one relation of the layer, as a rank inside the
    relation's source type (relation_src_type), in the sampler's order."""
    return _get("samgraph_get_graph_rel_row", batch_key, layer_idx, relation)


def get_graph_rel_col(batch_key, layer_idx, relation):
    """Config key hetero_batch: the destination end, a rank inside the relation's destination type."""
    return _get("samgraph_get_graph_rel_col", batch_key, layer_idx, relation)


def get_graph_rel_edge_ids(batch_key, layer_idx, relation):
    """Config key hetero_batch: the CSR positions of the relation's edges of the layer."""
    return _get("samgraph_get_graph_rel_edge_ids", batch_key, layer_idx, relation)


def get_graph_edge_time(batch_key, layer_idx):
    """sample_type khop_temporal: the time of every edge of the layer, edge_time[get_graph_edge_ids] (int32 holding the
    uint32 bits)."""
    return _get("samgraph_get_graph_edge_time", batch_key, layer_idx)


def get_graph_node_cut(batch_key):
    """sample_type khop_temporal: the cut-off time of every input node -- the smallest time among the positives it
    serves; node_cut[col] - edge_time is an edge's age for a time encoding (int32 holding the uint32 bits)."""
    return _get("samgraph_get_graph_node_cut", batch_key)


def get_graph_link_time(batch_key):
    """sample_type khop_temporal: the times of the batch's positive edges, in the order of get_graph_link_edge_ids."""
    return _get("samgraph_get_graph_link_time", batch_key)


def get_graph_edge_type(batch_key, layer_idx):
    """sample_type khop_typed: the relation of every edge of the layer, edge_type[get_graph_edge_ids] (uint8)."""
    return _get("samgraph_get_graph_edge_type", batch_key, layer_idx)


def get_graph_link_edge_ids(batch_key):
    """The positive edge ids (CSR positions) of a link_prediction batch, in the order of get_graph_link_pairs."""
    return _get("samgraph_get_graph_link_edge_ids", batch_key)


def get_graph_link_pairs(batch_key):
    """(pos_src, pos_dst, neg_src, neg_dst) of a link_prediction batch: views of the batch's one id tensor
    (get_graph_seed_ids), B positives and K negatives each -- pos_src, pos_dst of shape (B,), neg_src (pos_src expanded)
    and neg_dst of shape (B, K).  The values are local ids into the batch's node numbering: rows of get_graph_feat /
    get_graph_input_nodes, the ids the first sampled layer's col uses."""
    ids = get_graph_seed_ids(batch_key)
    k = num_negative()  # noqa: F405
    b = ids.numel() // (2 + k)
    pos_src, pos_dst = ids[:b], ids[b:2 * b]
    return pos_src, pos_dst, pos_src.unsqueeze(1).expand(b, k), ids[2 * b:].view(b, k)


def update_graph_feat(batch_key, grad):
    """Config key feat_learnable: the gradient of get_graph_feat(batch_key) -- row i for row i -- moves the learnable
    table's rows of the batch's input nodes (SGD or Adagrad, include/ggms.h ggms_update_rows).  `grad` is a contiguous
    float32 CUDA tensor of the delivered shape on the trainer device, produced on the current stream; the call enqueues
    and returns, and `grad` may be dropped right after it.  Batches enqueued by a LATER sample_once see the update."""
    if not (torch.is_tensor(grad) and grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous()):
        raise ValueError("update_graph_feat: grad must be a contiguous float32 CUDA tensor, got "
                         f"{getattr(grad, 'dtype', type(grad))} on {getattr(grad, 'device', '?')}"
                         f"{'' if not torch.is_tensor(grad) or grad.is_contiguous() else ' (not contiguous)'}")
    t = _CTensor()
    _basics.C_LIB_CTYPES.samgraph_get_graph_feat(batch_key, C.byref(t))
    if grad.device.index != t.device_id:
        raise ValueError(f"update_graph_feat: grad is on {grad.device}, the trainer device is cuda:{t.device_id}")
    delivered = (int(t.shape[0]), int(t.shape[1]))
    if tuple(grad.shape) != delivered:  # (the engine checks again for callers of the C entry, and aborts)
        raise ValueError(f"update_graph_feat: grad of shape {tuple(grad.shape)}, batch {batch_key} delivered {delivered}")
    _basics.C_LIB_CTYPES.samgraph_update_graph_feat(batch_key, grad.data_ptr(), grad.shape[0], grad.shape[1],
                                                    torch.cuda.current_stream(grad.device).cuda_stream)


def get_store_feat():
    """The live learnable table (config key feat_learnable): a zero-copy (num_node, feat_dim) float32 device view."""
    return _get("samgraph_get_store_feat", None)


def get_store_state():
    """The Adagrad accumulator of the learnable table (feat_learnable = adagrad), shaped like get_store_feat()."""
    return _get("samgraph_get_store_state", None)


def _create_dgl_block(data, num_src_nodes, num_dst_nodes):
    import dgl  # DGL-on-ROCm is needed only here, exactly where the reference needs it (adapter.py:131-136)
    from dgl.heterograph import DGLBlock
    row, col = data
    gidx = dgl.heterograph_index.create_unitgraph_from_coo(2, num_src_nodes, num_dst_nodes, row, col,
                                                           ['coo', 'csr', 'csc'])
    return DGLBlock(gidx, (['_N'], ['_N']), ['_E'])


def get_graph_coo(batch_key, num_layers):
    """(row, col, num_src, num_dst) per layer without DGL -- what get_dgl_blocks feeds to DGL."""
    return [(get_graph_row(batch_key, i), get_graph_col(batch_key, i),
             get_graph_num_src(batch_key, i), get_graph_num_dst(batch_key, i)) for i in range(num_layers)]  # noqa: F405


def get_dgl_blocks(batch_key, num_layers, with_feat=True):
    feat = get_graph_feat(batch_key) if with_feat else None
    label = get_graph_label(batch_key) if with_feat else None
    blocks = [_create_dgl_block((row, col), ns, nd) for row, col, ns, nd in get_graph_coo(batch_key, num_layers)]
    return blocks, feat, label


def get_dgl_blocks_with_weights(batch_key, num_layers, with_feat=True):
    blocks, feat, label = get_dgl_blocks(batch_key, num_layers, with_feat)
    for i, block in enumerate(blocks):
        block.edata['weights'] = get_graph_data(batch_key, i)
    return blocks, feat, label


def notify_sampler_ready(barrier): barrier.wait()
def wait_for_sampler_ready(barrier): barrier.wait()


def load_subtensor(batch_key, feat, label, device):
    input_nodes = get_graph_input_nodes(batch_key).to(feat.device)
    output_nodes = get_graph_output_nodes(batch_key).to(label.device)
    batch_inputs = torch.index_select(feat, 0, input_nodes.long()).to(device, dtype=torch.float32)
    batch_labels = torch.index_select(label, 0, output_nodes.long()).to(device)
    return batch_inputs, batch_labels
