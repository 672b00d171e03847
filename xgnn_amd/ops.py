"""Tensor-level wrappers over the C ABI (include/ggms.h).

PyTorch-ROCm is used for device memory and streams only; every operator below
is one or more calls into libggms_hip.so with raw device pointers.  Ids are
stored in int32 tensors (the reference hands int32 to PyTorch too,
samgraph/torch/adapter.cc:103,117) and are bit-identical to uint32.
"""
import ctypes as C

import numpy as np

import torch

from . import _lib
from ._lib import Graph as _CGraph, HashTable as _CHashTable, check, lib
from ._lib import (COUNTS_SAMPLE_WORDS, COUNTS_WORDS, COUNT_DST, COUNT_EDGES, COUNT_EXPANSION, COUNT_INPUT, COUNT_SRC,
                   COUNT_STATUS)

EMPTY_KEY = 0xFFFFFFFF

# DataType codes, samgraph/common/common.h:38-46; 7 = GGMS_BF16, 16 / 17 = GGMS_F8E4M3 / GGMS_F8E5M2 (the OCP 8-bit
# floats as TABLE types) are extensions, include/ggms.h
DTYPE_CODE = {
    torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.uint8: 3,
    torch.int32: 4, torch.int8: 5, torch.int64: 6, torch.int16: 2, torch.bfloat16: 7,
    torch.float8_e4m3fn: 16, torch.float8_e5m2: 17,
}

# GGMS_Q8ROW (include/ggms.h): a ROW format, 8-bit codes with a float32 scale and bias per row.  No torch dtype stands
# for it: such a table is a torch.uint8 tensor of shape (rows, row_bytes(Q8ROW, dim)) passed with src_dtype=Q8ROW.
Q8ROW = 18


def _dtype_code(dtype):
    """ggms_dtype code of a torch dtype, or the code itself."""
    return dtype if isinstance(dtype, int) else DTYPE_CODE[dtype]


def row_bytes(dtype, dim):
    """ggms_row_bytes: bytes from one stored row of `dim` elements to the next (dtype: a torch dtype or a code)."""
    return lib().ggms_row_bytes(_dtype_code(dtype), dim)


def _check_q8row(src, src_dtype, dim):
    if _dtype_code(src_dtype) == Q8ROW and src is not None:
        assert src.dtype == torch.uint8 and src.shape[-1] == row_bytes(Q8ROW, dim), \
            f"a Q8ROW table of dim {dim} is a uint8 tensor of (rows, {row_bytes(Q8ROW, dim)}), not {src.dtype} {tuple(src.shape)}"


KHOP0, KHOP1, WEIGHTED_KHOP, RANDOM_WALK, WEIGHTED_KHOP_PREFIX, KHOP2, WEIGHTED_KHOP_HASH_DEDUP, KHOP3 = range(8)
KHOP_LABOR = 8  # an extension: per-node shared randomness (include/ggms.h)
KHOP_TEMPORAL = 9  # an extension: sampling strictly before a per-seed cut-off time (include/ggms.h)
PICK_UNIFORM, PICK_RECENT = 0, 1  # khop_temporal's picks
KHOP_TYPED = 10  # an extension: a fanout per edge type on a type-sorted CSR (include/ggms.h)
MAX_EDGE_TYPES = 32  # GGMS_MAX_EDGE_TYPES
_STATELESS = (KHOP0, KHOP_LABOR, KHOP_TEMPORAL, KHOP_TYPED)  # samplers without an RNG pool


def _require_gpu(t):
    if not t.is_cuda:
        raise _lib.GgmsError("xgnn_amd operators need device tensors (no CPU fallback)")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(t):
    assert t.dtype == torch.int32 and t.is_contiguous(), "ids must be contiguous int32 tensors"
    return t


class DeviceGraph:
    """ggms_graph_t over device tensors: DeviceNormalGraph or DeviceDistGraph (dist_graph.h:114-180).

    inline_heads: the 64-byte-per-node table of include/ggms.h ("Inline list heads"), built once here and attached to
    the struct; khop3 then finds a frontier node's list with one request.  None (default): build it if the graph is an
    unsharded CSR on a GPU and 64 x num_node bytes are at most a quarter of the device's free memory; True: build it or
    raise; False: never.  The CSR must keep its contents while the heads are attached (khop2, which permutes `indices`,
    detaches them)."""

    def __init__(self, indptr, indices, part_indptr=None, part_indices=None, num_cache_node=0, inline_heads=None):
        self.indptr, self.indices = indptr, indices
        self.heads = None
        self._keep = [indptr, indices]
        num_node = (indptr.numel() - 1) if indptr is not None else 0
        self.c = _CGraph()
        self.c.indptr = indptr.data_ptr() if indptr is not None else None
        self.c.indices = indices.data_ptr() if indices is not None else None
        self.c.num_node = num_node
        self.c.num_part = 0
        self.c.num_cache_node = 0
        if part_indptr is not None:
            # part_* : lists of P+1 tensors (slot P = whole CSR, device memory or pinned / registered host memory);
            # the pointer tables are HOST arrays -- the kernels take the pointers by value (include/ggms.h)
            self._pip = PartTable([t.data_ptr() for t in part_indptr])
            self._pix = PartTable([t.data_ptr() for t in part_indices])
            self._keep += list(part_indptr) + list(part_indices)
            self.c.part_indptr = self._pip.ptr().value
            self.c.part_indices = self._pix.ptr().value
            self.c.num_part = len(part_indptr) - 1
            self.c.num_cache_node = num_cache_node
            self.c.num_node = part_indptr[-1].numel() - 1
        if inline_heads or inline_heads is None:
            self._build_heads(required=bool(inline_heads))

    def _build_heads(self, required):
        on_gpu = (self.c.num_part == 0 and self.indptr is not None and self.indices is not None
                  and getattr(self.indptr, "is_cuda", False) and getattr(self.indices, "is_cuda", False)
                  and self.c.num_node > 0)
        if not on_gpu:
            if required:
                raise _lib.GgmsError("inline_heads=True needs an unsharded CSR in device memory")
            return
        nbytes = lib().ggms_list_heads_bytes(self.c.num_node)
        with torch.cuda.device(self.indptr.device):
            if not required and 4 * nbytes > torch.cuda.mem_get_info()[0]:
                return
            heads = torch.empty(nbytes // 4, dtype=torch.int32, device=self.indptr.device)
            check(lib().ggms_list_heads_build(C.byref(self.c), _ptr(heads), nbytes, _stream()), "ggms_list_heads_build")
            # samplers run on streams of their own: the table is complete before anyone can look
            torch.cuda.current_stream().synchronize()
        check(lib().ggms_list_heads_attach(C.byref(self.c), _ptr(heads)), "ggms_list_heads_attach")
        self.heads = heads

    def detach_heads(self):
        """Release the handle and the table (nothing happens without one)."""
        if self.heads is not None:
            lib().ggms_list_heads_detach(C.byref(self.c))
            self.heads = None

    def __del__(self):
        try:
            self.detach_heads()
        except Exception:  # interpreter shutdown: the library may be gone already
            pass


def random_states(num_states, seed, device="cuda"):
    """GPURandomStates (cuda_random_states.cu:64-109) with an explicit seed."""
    st = torch.empty((num_states, 6), dtype=torch.int32, device=device)
    _require_gpu(st)
    check(lib().ggms_random_states_init(_ptr(st), num_states, seed, _stream()), "ggms_random_states_init")
    return st


def device_status(clear=False):
    """The device status word (include/ggms.h): 0 = ok, 1 = a scan's look-back gave up, 2 = hashed table full.
    Synchronises the device."""
    st = C.c_uint32(0)
    check(lib().ggms_device_status(C.byref(st), 1 if clear else 0), "ggms_device_status")
    return st.value


def check_device_status(what=""):
    """Raise if a kernel reported a device-side failure (the reference CHECK-aborts there, logging.cc:69-73)."""
    st = device_status(clear=True)
    if st:
        raise _lib.GgmsError(f"{what}: device status {st:#x} "
                             f"({'scan look-back gave up ' if st & 1 else ''}{'hashed dedup table full' if st & 2 else ''})")


def _workspace(nbytes, device):
    return torch.empty(max(16, (nbytes + 3) // 4), dtype=torch.int32, device=device)


def _sample(fn_name, sample_type, graph, inp, fanout, states, *tables, salt=None):
    """One leaf sampler call: (out_src, out_dst, num_out[1] on device).  tables: the device arrays the entry point takes
    between the graph and the input; states=None: a sampler without an RNG pool (khop0, khop_labor); salt: khop_labor's
    layer salt, passed behind the fanout."""
    _require_gpu(inp)
    _i32(inp)
    n = inp.numel()
    dev = inp.device
    out_src = torch.empty(max(1, n * fanout), dtype=torch.int32, device=dev)
    out_dst = torch.empty(max(1, n * fanout), dtype=torch.int32, device=dev)
    num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_sample_workspace_bytes(sample_type, n, fanout), dev)
    rng = (_ptr(states), states.shape[0]) if states is not None else ()
    salt = (C.c_uint32(salt & 0xFFFFFFFF),) if salt is not None else ()
    check(getattr(lib(), fn_name)(C.byref(graph.c), *map(_ptr, tables), _ptr(inp), n, fanout, *salt, _ptr(out_src),
                                  _ptr(out_dst), _ptr(num_out), *rng, _ptr(ws), ws.numel() * 4, _stream()), fn_name)
    return out_src, out_dst, num_out


def sample_khop3(graph, inp, fanout, states):
    """GPUSampleKHop3 (cuda_sampling_khop3.cu:234-318).  Returns (out_src, out_dst, num_out[1] on device)."""
    return _sample("ggms_sample_khop3", KHOP3, graph, inp, fanout, states)


def sample_khop0(graph, inp, fanout):
    """GPUSampleKHop0 (cuda_sampling_khop0.cu:243-335)."""
    return _sample("ggms_sample_khop0", KHOP0, graph, inp, fanout, None)


def sample_khop_labor(graph, inp, fanout, layer_salt):
    """ggms_sample_khop_labor: the min(fanout, degree) neighbours with the smallest fmix32(id ^ layer_salt), per seed."""
    return _sample("ggms_sample_khop_labor", KHOP_LABOR, graph, inp, fanout, None, salt=layer_salt)


def sample_khop_temporal(graph, edge_time, inp, inp_cut, fanout, layer_salt, pick=PICK_UNIFORM):
    """ggms_sample_khop_temporal: per seed, among the list entries with edge_time < inp_cut[i] (a prefix of the
    time-sorted list), khop_labor's selection (PICK_UNIFORM) or the last min(fanout, e) of them (PICK_RECENT).
    Returns (out_src, out_dst, out_pos, num_out[1] on device); out_pos = the edges' positions in graph.indices."""
    _require_gpu(inp)
    _i32(inp), _i32(inp_cut), _i32(edge_time)
    n = inp.numel()
    assert inp_cut.numel() == n
    dev = inp.device
    out = [torch.empty(max(1, n * fanout), dtype=torch.int32, device=dev) for _ in range(3)]
    num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_sample_workspace_bytes(KHOP_TEMPORAL, n, fanout), dev)
    check(lib().ggms_sample_khop_temporal(C.byref(graph.c), _ptr(edge_time), _ptr(inp), _ptr(inp_cut), n, fanout, pick,
                                          layer_salt & 0xFFFFFFFF, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                          _ptr(num_out), _ptr(ws), ws.numel() * 4, _stream()),
          "ggms_sample_khop_temporal")
    return out[0], out[1], out[2], num_out


def _u8(t):
    assert t.dtype == torch.uint8 and t.dim() == 1 and t.stride(0) == 1, "edge types: a dense 1-d uint8 tensor"
    return t


def sample_khop_typed(graph, edge_type, type_fanout, inp, layer_salt):
    """ggms_sample_khop_typed: per seed and edge type r (a contiguous segment of the type-sorted list), khop_labor's
    selection with fanout type_fanout[r] on the segment, one salt for all types.
    Returns (out_src, out_dst, out_pos, out_type, num_out[1] on device); out_pos = the edges' positions in
    graph.indices, out_type (uint8) their types."""
    _require_gpu(inp)
    _i32(inp), _u8(edge_type)
    n, R = inp.numel(), len(type_fanout)
    K = sum(int(k) for k in type_fanout)
    dev = inp.device
    out = [torch.empty(max(1, n * K), dtype=torch.int32, device=dev) for _ in range(3)]
    out_type = torch.empty(max(1, n * K), dtype=torch.uint8, device=dev)
    num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_sample_khop_typed_workspace_bytes(n, R), dev)
    f = (C.c_uint32 * max(R, 1))(*[int(k) for k in type_fanout])
    check(lib().ggms_sample_khop_typed(C.byref(graph.c), _ptr(edge_type), R, f, _ptr(inp), n, layer_salt & 0xFFFFFFFF,
                                       _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out_type), _ptr(num_out),
                                       _ptr(ws), ws.numel() * 4, _stream()), "ggms_sample_khop_typed")
    return out[0], out[1], out[2], out_type, num_out


def link_seed_times(edge_time, edge_ids, num_negative):
    """ggms_link_seed_times: edge_time[edge_ids[i]] for the source, the destination and every negative of positive i,
    in ggms_link_seeds' endpoint layout (an id past edge_time's end: 0)."""
    _require_gpu(edge_ids)
    _i32(edge_ids), _i32(edge_time)
    n = edge_ids.numel()
    out = torch.empty(max(1, n * (2 + max(0, num_negative))), dtype=torch.int32, device=edge_ids.device)
    check(lib().ggms_link_seed_times(_ptr(edge_time), edge_time.numel(), _ptr(edge_ids), n, num_negative, _ptr(out),
                                     _stream()), "ggms_link_seed_times")
    return out[: n * (2 + num_negative)]


NEG_UNIFORM, NEG_EXCLUDE = 0, 1  # ggms_link_seeds modes


def link_seeds(graph, edge_ids, num_negative, mode=NEG_EXCLUDE, salt=0, count_forced=True):
    """ggms_link_seeds: positive edge ids (CSR positions) -> (endpoints, num_forced[1] on device).  endpoints holds
    B sources, B destinations and B x num_negative negative destinations (include/ggms.h); num_forced counts the
    negatives of mode NEG_EXCLUDE whose eight candidates were all rejected (None with count_forced=False)."""
    _require_gpu(edge_ids)
    _i32(edge_ids)
    n = edge_ids.numel()
    out = torch.empty(max(1, n * (2 + max(0, num_negative))), dtype=torch.int32, device=edge_ids.device)
    forced = torch.zeros(1, dtype=torch.int64, device=edge_ids.device) if count_forced else None
    check(lib().ggms_link_seeds(C.byref(graph.c), _ptr(edge_ids), n, num_negative, mode, salt & 0xFFFFFFFF, _ptr(out),
                                _ptr(forced), _stream()), "ggms_link_seeds")
    return out[: n * (2 + num_negative)], forced


DROP_FORWARD, DROP_REVERSE = 1, 2  # ggms_drop_pair_edges' `which` bits


def drop_pair_edges(pair_src, pair_dst, which, rows, cols, counts, max_edges=None, num_dropped=None):
    """ggms_drop_pair_edges: drop from every layer (rows[i], cols[i], counts[COUNT_EDGES(i)] edges) the edges with
    (col, row) == (pair_src[p], pair_dst[p]) (DROP_FORWARD) and / or (pair_dst[p], pair_src[p]) (DROP_REVERSE), in
    place and stable; counts (a device int64 tensor in the batch counts layout) gets the new edge counts.  max_edges:
    the layers' bounds (default: the tensors' lengths).  Returns num_dropped, a device int64 tensor of len(rows) words
    the dropped edges are ADDED to (a fresh zeroed one unless given)."""
    L = len(rows)
    _require_gpu(counts)
    dev = counts.device
    assert counts.dtype == torch.int64 and counts.is_contiguous()
    for t in list(rows) + list(cols):
        _require_gpu(_i32(t))
    n = 0
    if pair_src is not None:
        _require_gpu(_i32(pair_src))
        _require_gpu(_i32(pair_dst))
        n = pair_src.numel()
        assert pair_dst.numel() == n
    me = [int(x) for x in max_edges] if max_edges is not None else [min(r.numel(), c.numel()) for r, c in zip(rows, cols)]
    c_me = (C.c_size_t * max(1, L))(*me)
    if num_dropped is None:
        num_dropped = torch.zeros(max(1, L), dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_drop_pair_edges_workspace_bytes(n, c_me, L), dev)
    c_rows = (C.c_void_p * max(1, L))(*[t.data_ptr() for t in rows])
    c_cols = (C.c_void_p * max(1, L))(*[t.data_ptr() for t in cols])
    check(lib().ggms_drop_pair_edges(_ptr(pair_src), _ptr(pair_dst), n, which, c_rows, c_cols, c_me, L, _ptr(counts),
                                     _ptr(num_dropped), _ptr(ws), ws.numel() * 4, _stream()), "ggms_drop_pair_edges")
    return num_dropped


def edge_positions(graph, rows, cols, counts, id_map=None, max_edges=None, eids=None, num_edge=None):
    """ggms_edge_positions: for every edge k < counts[COUNT_EDGES(i)] of every layer (rows[i], cols[i]) the CSR position of
    the edge (s -> t), s = id_map[cols[i][k]], t = id_map[rows[i][k]] (the ids themselves without id_map): the smallest p
    in s's list with indices[p] == t, EMPTY_KEY (-1 as int32) where there is none or an id is no node.  counts: a device
    int64 tensor in the batch counts layout.  max_edges: the layers' bounds (default: the tensors' lengths).  eids: the
    output tensors (entries behind the count are left alone; fresh ones unless given).  num_edge: indptr[-1] (default:
    indices' length).  Returns eids."""
    L = len(rows)
    _require_gpu(counts)
    dev = counts.device
    assert counts.dtype == torch.int64 and counts.is_contiguous()
    for t in list(rows) + list(cols):
        _require_gpu(_i32(t))
    me = [int(x) for x in max_edges] if max_edges is not None else [min(r.numel(), c.numel()) for r, c in zip(rows, cols)]
    if eids is None:
        eids = [torch.empty(max(1, m), dtype=torch.int32, device=dev) for m in me]
    for t, m in zip(eids, me):
        _require_gpu(_i32(t))
        assert t.numel() >= m, "edge_positions: an eid tensor is shorter than its layer's bound"
    if id_map is not None:
        _require_gpu(_i32(id_map))
    c_me = (C.c_size_t * max(1, L))(*me)
    ws = _workspace(lib().ggms_edge_positions_workspace_bytes(c_me, L), dev)
    c_rows = (C.c_void_p * max(1, L))(*[t.data_ptr() for t in rows])
    c_cols = (C.c_void_p * max(1, L))(*[t.data_ptr() for t in cols])
    c_eids = (C.c_void_p * max(1, L))(*[t.data_ptr() for t in eids])
    ne = int(num_edge) if num_edge is not None else graph.indices.numel()
    check(lib().ggms_edge_positions(C.byref(graph.c), ne, _ptr(id_map), id_map.numel() if id_map is not None else 0,
                                    c_rows, c_cols, c_eids, c_me, L, _ptr(counts), _ptr(ws), ws.numel() * 4, _stream()),
          "ggms_edge_positions")
    return eids


def induced_map(num_node, device="cuda"):
    """The membership map of ggms_induced_edges: num_node int32 words, all EMPTY_KEY (ggms_induced_map_init).  Every
    call leaves it as it found it, so one map serves every call on a graph (one call at a time)."""
    m = torch.empty(max(1, num_node), dtype=torch.int32, device=device)
    _require_gpu(m)
    check(lib().ggms_induced_map_init(_ptr(m), m.numel(), _stream()), "ggms_induced_map_init")
    return m


def induced_edges(graph, nodes, local_of, max_edges, num_nodes_dev=None, want_eid=True, num_edge=None, out=None,
                  counts=None, max_nodes=None):
    """ggms_induced_edges: every edge of the graph with both ends among nodes[0, n), as (row, col, eid) over positions of
    `nodes` (row: the neighbour, col: the node whose list was read, eid: the CSR position) in (col, position) order; a
    repeated id counts at its first position only.  n = num_nodes_dev[0] (a device int64 tensor) or len(nodes).  Returns
    (row, col, eid, counts): the first min(M, max_edges) entries are written, counts (device int64[2]) = [M, list entries
    walked]; eid is None without want_eid.  num_edge: indptr[-1] (default: indices' length).  out: (row, col, eid)
    tensors to write into (fresh ones unless given); counts: the count words' tensor."""
    _require_gpu(_i32(nodes))
    _require_gpu(_i32(local_of))
    dev = nodes.device
    mn = int(max_nodes) if max_nodes is not None else nodes.numel()
    if out is None:
        out = tuple(torch.empty(max(1, max_edges), dtype=torch.int32, device=dev) for _ in range(3))
    row, col, eid = out
    if not want_eid:
        eid = None
    for t in (row, col, eid):
        if t is not None:
            _require_gpu(_i32(t))
            assert t.numel() >= max_edges, "induced_edges: an output tensor is shorter than max_edges"
    if counts is None:
        counts = torch.empty(2, dtype=torch.int64, device=dev)
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= 2
    if num_nodes_dev is not None:
        assert num_nodes_dev.dtype == torch.int64 and num_nodes_dev.is_cuda
    ne = int(num_edge) if num_edge is not None else graph.indices.numel()
    ws = _workspace(lib().ggms_induced_edges_workspace_bytes(mn, ne), dev)
    check(lib().ggms_induced_edges(C.byref(graph.c), ne, _ptr(nodes), mn, _ptr(num_nodes_dev), _ptr(local_of),
                                   _ptr(row), _ptr(col), _ptr(eid), max_edges, _ptr(counts), _ptr(ws), ws.numel() * 4,
                                   _stream()), "ggms_induced_edges")
    return row, col, eid, counts


MAX_NODE_TYPES = 32   # GGMS_MAX_NODE_TYPES
HETERO_MAX_CUTS = 17  # GGMS_HETERO_MAX_CUTS


def hetero_nodes(node_type, num_type, nodes, num_nodes_dev=None, cut_base=None, cut_words=(), max_nodes=None, out=None,
                 workspace=None):
    """ggms_hetero_nodes: the nodes of a batch grouped by node type.  node_type: a device uint8 tensor, one byte per node
    id, values below num_type; nodes: the batch's ids (int32), the first n = min(num_nodes_dev[0], max_nodes) count
    (num_nodes_dev: a device int64 tensor; without it n = max_nodes, default len(nodes)).  cut_base: a device int64
    tensor, cut_words: indices into it -- cut k is cut_base[cut_words[k]].  Returns a dict: ntype (uint8; 255 for an id
    that is no node), local (rank inside the type), slot (= base[ntype] + local), typed_nodes (typed_nodes[slot[i]] =
    nodes[i]), base (int32, num_type + 1 words: base[t] = entries of a type below t), cut_counts (int32,
    (len(cut_words), num_type): the types of nodes[0, min(cut, n))).  Entries behind n are left alone.  out: a dict of
    tensors to write into (fresh ones unless given); workspace: an int32 tensor of at least
    ggms_hetero_nodes_workspace_bytes (a fresh one unless given)."""
    _require_gpu(_i32(nodes))
    _require_gpu(node_type)
    assert node_type.dtype == torch.uint8 and node_type.is_contiguous()
    dev = nodes.device
    T, B = int(num_type), len(cut_words)
    mn = int(max_nodes) if max_nodes is not None else nodes.numel()
    assert mn <= nodes.numel()
    o = dict(out) if out is not None else {}
    o.setdefault("ntype", torch.empty(max(1, mn), dtype=torch.uint8, device=dev))
    for name in ("local", "slot", "typed_nodes"):
        o.setdefault(name, torch.empty(max(1, mn), dtype=torch.int32, device=dev))
    o.setdefault("base", torch.empty(max(1, T + 1), dtype=torch.int32, device=dev))
    o.setdefault("cut_counts", torch.empty((B, max(1, T)), dtype=torch.int32, device=dev))
    for name in ("ntype", "local", "slot", "typed_nodes"):
        _require_gpu(o[name])
        assert o[name].is_contiguous() and o[name].numel() >= mn, f"hetero_nodes: {name} is shorter than max_nodes"
    assert o["ntype"].dtype == torch.uint8 and o["base"].numel() >= T + 1 and o["cut_counts"].numel() >= B * T
    for name in ("local", "slot", "typed_nodes", "base", "cut_counts"):
        assert o[name].dtype == torch.int32 and o[name].is_contiguous()
    if num_nodes_dev is not None:
        assert num_nodes_dev.dtype == torch.int64 and num_nodes_dev.is_cuda
    if B:
        assert cut_base is not None and cut_base.dtype == torch.int64 and cut_base.is_cuda and cut_base.is_contiguous()
        assert all(0 <= int(w) < cut_base.numel() for w in cut_words)
    need = lib().ggms_hetero_nodes_workspace_bytes(mn, T)
    ws = workspace if workspace is not None else _workspace(need, dev)
    c_words = (C.c_uint32 * max(1, B))(*[int(w) for w in cut_words])
    check(lib().ggms_hetero_nodes(_ptr(node_type), node_type.numel(), T, _ptr(nodes), mn, _ptr(num_nodes_dev),
                                  _ptr(cut_base), c_words, B, _ptr(o["ntype"]), _ptr(o["local"]), _ptr(o["slot"]),
                                  _ptr(o["typed_nodes"]), _ptr(o["base"]), _ptr(o["cut_counts"]), _ptr(ws),
                                  ws.numel() * 4, _stream()), "ggms_hetero_nodes")
    return o


def hetero_edges(rows, cols, etypes, num_rel, counts, local, eids=None, max_edges=None, out=None, rel_offsets=None,
                 workspace=None):
    """ggms_hetero_edges: every layer's edges grouped by relation (stable) and renumbered through `local`
    (hetero_nodes): per layer i the first E = min(counts[COUNT_EDGES(i)], max_edges[i]) entries of rows[i] / cols[i] /
    etypes[i] (uint8) / eids[i] count; entry e of relation r goes to q = off[r] + its rank among the layer's entries of r,
    out_row[q] = local[rows[i][e]], out_col[q] = local[cols[i][e]], out_eid[q] = eids[i][e].  counts: a device int64
    tensor in the batch counts layout.  Returns (out_rows, out_cols, out_eids or None, rel_offsets): rel_offsets is int32
    of shape (L, num_rel + 1).  out: (out_rows, out_cols, out_eids) lists to write into; workspace as in hetero_nodes."""
    L, R = len(rows), int(num_rel)
    _require_gpu(counts)
    dev = counts.device
    assert counts.dtype == torch.int64 and counts.is_contiguous()
    _require_gpu(_i32(local))
    for t in list(rows) + list(cols) + (list(eids) if eids is not None else []):
        _require_gpu(_i32(t))
    for t in etypes:
        _require_gpu(t)
        assert t.dtype == torch.uint8  # (any byte offset: a slice of a larger tensor is fine)
    me = [int(x) for x in max_edges] if max_edges is not None else [min(r.numel(), c.numel()) for r, c in zip(rows, cols)]
    if out is None:
        fresh = lambda: [torch.empty(max(1, m), dtype=torch.int32, device=dev) for m in me]  # noqa: E731
        out = (fresh(), fresh(), fresh() if eids is not None else None)
    out_rows, out_cols, out_eids = out
    assert (out_eids is None) == (eids is None)
    for ts in (out_rows, out_cols, out_eids):
        for t, m in zip(ts or [], me):
            _require_gpu(_i32(t))
            assert t.numel() >= m, "hetero_edges: an output tensor is shorter than its layer's bound"
    if rel_offsets is None:
        rel_offsets = torch.empty((max(1, L), R + 1), dtype=torch.int32, device=dev)
    assert rel_offsets.dtype == torch.int32 and rel_offsets.is_contiguous() and rel_offsets.numel() >= L * (R + 1)
    c_me = (C.c_size_t * max(1, L))(*me)
    arr = lambda ts: (C.c_void_p * max(1, L))(*[t.data_ptr() for t in ts]) if ts is not None else None  # noqa: E731
    need = lib().ggms_hetero_edges_workspace_bytes(c_me, L, R)
    ws = workspace if workspace is not None else _workspace(need, dev)
    check(lib().ggms_hetero_edges(arr(rows), arr(cols), arr(eids), arr(etypes), c_me, L, R, _ptr(counts), _ptr(local),
                                  local.numel(), arr(out_rows), arr(out_cols), arr(out_eids), _ptr(rel_offsets), _ptr(ws),
                                  ws.numel() * 4, _stream()), "ggms_hetero_edges")
    return out_rows, out_cols, out_eids, rel_offsets


def typed_tables(tables, out_dtypes=None, first_nodes=None):
    """The ggms_typed_table_t array of a table set.  tables: one entry per node type, a contiguous 2-D device tensor
    (float32, float16 or bfloat16) or None for a type without features; out_dtypes: the delivered dtype per type (None,
    or a None entry: the table's own); first_nodes: the first node id of every type, for calls without a rank table."""
    T = len(tables)
    arr = (_lib.TypedTable * max(1, T))()
    for t, tab in enumerate(tables):
        if tab is None:
            continue
        _require_gpu(tab)
        assert tab.dim() == 2 and tab.is_contiguous(), f"typed_tables: table {t} is not a contiguous 2-D tensor"
        od = out_dtypes[t] if out_dtypes is not None and out_dtypes[t] is not None else tab.dtype
        arr[t] = _lib.TypedTable(tab.data_ptr(), tab.shape[0], tab.shape[1], _dtype_code(tab.dtype), _dtype_code(od),
                                 int(first_nodes[t]) if first_nodes is not None else 0)
    return arr


def gather_typed_out_bytes(c_tables, num_type, max_nodes):
    """ggms_gather_typed_out_bytes (0 for arguments out of range)."""
    return lib().ggms_gather_typed_out_bytes(c_tables, num_type, max_nodes)


def gather_typed(c_tables, num_type, typed_nodes, base, row_of_node=None, num_node=None, max_nodes=None, out=None,
                 offsets=None):
    """ggms_gather_typed: the feature rows of a heterogeneous batch, one table per node type (c_tables: typed_tables()),
    into one uint8 buffer of per-type blocks.  typed_nodes / base: as hetero_nodes returns them; row_of_node: a device
    int32 tensor, a node's row in its type's table (None: row = node - first_node of the type); num_node: ids at or above
    it give zero rows (default: len(row_of_node); without a rank table no bound: every id is taken for a node, and a
    type's table alone decides which rows exist).  Returns (out, offsets): block t is out[offsets[t]:] as
    (base[t + 1] - base[t], dim_t) rows of the type's delivered dtype; offsets is a device int64 tensor of num_type + 1
    words.  out / offsets: tensors to write into (fresh ones unless given)."""
    _require_gpu(_i32(typed_nodes))
    _require_gpu(_i32(base))
    dev = typed_nodes.device
    T = int(num_type)
    mn = int(max_nodes) if max_nodes is not None else typed_nodes.numel()
    assert mn <= typed_nodes.numel() and base.numel() >= T + 1
    if row_of_node is not None:
        _require_gpu(_i32(row_of_node))
        num_node = row_of_node.numel() if num_node is None else num_node
        assert num_node <= row_of_node.numel()
    elif num_node is None:
        num_node = 1 << 32  # no bound: ids are 32-bit
    if out is None:
        out = torch.empty(max(16, gather_typed_out_bytes(c_tables, T, mn)), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(T + 1, dtype=torch.int64, device=dev)
    _require_gpu(out)
    assert out.dtype == torch.uint8 and out.is_contiguous()
    assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and offsets.numel() >= T + 1
    check(lib().ggms_gather_typed(_ptr(out), out.numel(), c_tables, T, _ptr(typed_nodes), _ptr(base), mn,
                                  _ptr(row_of_node), int(num_node), _ptr(offsets), _stream()), "ggms_gather_typed")
    return out, offsets


def sample_weighted_khop_prefix(graph, prob_prefix_table, inp, fanout, states):
    """GPUSampleWeightedKHopPrefix (cuda_sampling_weighted_khop_prefix.cu:145-246)."""
    return _sample("ggms_sample_weighted_khop_prefix", WEIGHTED_KHOP_PREFIX, graph, inp, fanout, states,
                   prob_prefix_table)


def sample_weighted_khop_hash_dedup(graph, prob_table, alias_table, inp, fanout, states):
    """GPUSampleWeightedKHopHashDedup (cuda_sampling_weighted_khop_hash_dedup.cu:196-283)."""
    return _sample("ggms_sample_weighted_khop_hash_dedup", WEIGHTED_KHOP_HASH_DEDUP, graph, inp, fanout, states,
                   prob_table, alias_table)


def sample_khop1(graph, inp, fanout, states):
    """GPUSampleKHop1 (cuda_sampling_khop1.cu:130-236): uniform with replacement, adjacent duplicates dropped."""
    return _sample("ggms_sample_khop1", KHOP1, graph, inp, fanout, states)


def sample_khop2(graph, inp, fanout, states):
    """GPUSampleKHop2 (cuda_sampling_khop2.cu:196-262).  Permutes graph.indices in place, like the reference."""
    graph.detach_heads()  # the draws permute graph.indices: inline list heads would go stale
    return _sample("ggms_sample_khop2", KHOP2, graph, inp, fanout, states)


def sample_weighted_khop(graph, prob_table, alias_table, inp, fanout, states):
    """GPUSampleWeightedKHop (cuda_sampling_weighted_khop.cu:132-238)."""
    return _sample("ggms_sample_weighted_khop", WEIGHTED_KHOP, graph, inp, fanout, states, prob_table, alias_table)


def sample_random_walk(graph, inp, walk_length, restart_prob, num_walk, K, states):
    """GPUSampleRandomWalk + FrequencyHashmap::GetTopK (cuda_sampling_random_walk.cu:116-165)."""
    _require_gpu(inp)
    _i32(inp)
    n = inp.numel()
    dev = inp.device
    outs = [torch.empty(max(1, n * K), dtype=torch.int32, device=dev) for _ in range(3)]
    num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_sample_random_walk_workspace_bytes(n, walk_length, num_walk, K), dev)
    check(lib().ggms_sample_random_walk(C.byref(graph.c), _ptr(inp), n, walk_length, restart_prob, num_walk, K,
                                        _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(num_out), _ptr(states),
                                        states.shape[0], _ptr(ws), ws.numel() * 4, _stream()),
          "ggms_sample_random_walk")
    return outs[0], outs[1], outs[2], num_out


class OrderedHashTable:
    """OrderedHashTable (cuda_hashtable.h:103-153) over caller-owned device buffers."""

    def __init__(self, capacity, device="cuda", num_node=None):
        """num_node=None: hashed layout sized like the reference (TableSize); num_node=N: direct-mapped
        layout, one 8-byte word per node id (the engine's choice on MI355X)."""
        direct = num_node is not None
        nb = int(num_node) if direct else lib().ggms_hashtable_num_buckets(capacity)
        self.o2n = torch.empty((nb, 2 if direct else 4), dtype=torch.int32, device=device)
        _require_gpu(self.o2n)
        self.n2o = torch.empty(max(1, capacity), dtype=torch.int32, device=device)
        self.num_items_dev = torch.zeros(2, dtype=torch.int32, device=device)  # [item count, batch status word]
        self.c = _CHashTable()
        self.c.o2n = self.o2n.data_ptr()
        self.c.n2o = self.n2o.data_ptr()
        self.c.num_items_dev = self.num_items_dev.data_ptr()
        self.c.o2n_size = nb
        self.c.n2o_size = self.n2o.numel()
        self.c.direct = 1 if direct else 0
        check(lib().ggms_hashtable_init(C.byref(self.c), _stream()), "ggms_hashtable_init")

    def reset(self):
        check(lib().ggms_hashtable_reset(C.byref(self.c), _stream()), "ggms_hashtable_reset")

    def fill_with_duplicates(self, inp, num_input=None, unique_out=None):
        _i32(inp)
        n = inp.numel() if num_input is None else int(num_input)
        ws = _workspace(lib().ggms_hashtable_workspace_bytes(n), inp.device)
        check(lib().ggms_hashtable_fill_with_duplicates(C.byref(self.c), _ptr(inp), n, _ptr(unique_out), _ptr(ws),
                                                        ws.numel() * 4, _stream()),
              "ggms_hashtable_fill_with_duplicates")

    @property
    def num_items(self):
        return int(self.num_items_dev[0].item())

    def unique(self):
        return self.n2o[: self.num_items]

    def map_edges(self, src, dst, num_edges=None):
        n = (src if src is not None else dst).numel() if num_edges is None else int(num_edges)
        dev = (src if src is not None else dst).device
        ns = torch.empty(max(1, n), dtype=torch.int32, device=dev) if src is not None else None
        nd = torch.empty(max(1, n), dtype=torch.int32, device=dev) if dst is not None else None
        check(lib().ggms_map_edges(C.byref(self.c), _ptr(src), _ptr(ns), _ptr(dst), _ptr(nd), n, _stream()),
              "ggms_map_edges")
        return (ns[:n] if ns is not None else None), (nd[:n] if nd is not None else None)


def _dim_of(t):
    return t.shape[1] if t.dim() > 1 else 1


def extract(src, index, out=None):
    """GPUExtract (cuda_extraction.cu:74-117): out[i, :] = src[index[i], :]."""
    _require_gpu(index)
    _i32(index)
    assert src.is_contiguous()
    n = index.numel()
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=index.device)
    check(lib().ggms_extract(_ptr(out), _ptr(src), _ptr(index), n, _dim_of(src), DTYPE_CODE[src.dtype], _stream()),
          "ggms_extract")
    return out


def mock_extract(src, index, mock_bits, out=None):
    """GPUMockExtract (cuda_extraction.cu:119-160): out[i, :] = src[index[i] & (2**mock_bits - 1), :]."""
    _require_gpu(index)
    _i32(index)
    n = index.numel()
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=index.device)
    check(lib().ggms_mock_extract(_ptr(out), _ptr(src), _ptr(index), n, _dim_of(src), DTYPE_CODE[src.dtype], mock_bits,
                                  _stream()), "ggms_mock_extract")
    return out


def count_nodes(freq, nodes, num=None, num_dev=None):
    """The presample ranking's counter (dist/pre_sampler.cc:79-111): freq[nodes[i]] += 1 for i < num (freq: int32, one
    word per node).  With num_dev (device int64[1]) num is an upper bound."""
    _require_gpu(nodes)
    _i32(nodes)
    n = nodes.numel() if num is None else int(num)
    check(lib().ggms_count_nodes(_ptr(freq), _ptr(nodes), n, _ptr(num_dev), _stream()), "ggms_count_nodes")
    return freq


def get_miss_cache_index(table, nodes, num=None, num_dev=None, outs=None):
    """GetMissCacheIndex (cuda_cache_manager_device.cu:355-441).  Counts stay on the device.  With num_dev (device
    int64[1]) the batch size is read on the device and num is its upper bound: it sizes the launch, the four index
    arrays and the workspace (ggms_get_miss_cache_index_dev).  outs (optional): the caller's four int32 index arrays
    (miss src, miss dst, hit src, hit dst) of at least num entries each."""
    _require_gpu(nodes)
    n = nodes.numel() if num is None else int(num)
    dev = nodes.device
    if outs is None:
        outs = [torch.empty(max(1, n), dtype=torch.int32, device=dev) for _ in range(4)]
    assert len(outs) == 4 and all(_i32(o).numel() >= n for o in outs)
    num_miss = torch.zeros(1, dtype=torch.int64, device=dev)
    num_hit = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_cache_index_workspace_bytes(n), dev)
    tail = (_ptr(outs[0]), _ptr(outs[1]), _ptr(num_miss), _ptr(outs[2]), _ptr(outs[3]), _ptr(num_hit), _ptr(ws),
            ws.numel() * 4, _stream())
    if num_dev is None:
        check(lib().ggms_get_miss_cache_index(_ptr(table), _ptr(nodes), n, *tail), "ggms_get_miss_cache_index")
    else:
        check(lib().ggms_get_miss_cache_index_dev(_ptr(table), _ptr(nodes), n, _ptr(num_dev), *tail),
              "ggms_get_miss_cache_index_dev")
    return outs[0], outs[1], num_miss, outs[2], outs[3], num_hit


def khop_closure(graph, seeds, num_hop, visit, stamp, freq=None):
    """L-hop closure of `seeds` (DoGPUSampleAllNeighbour, cuda_loops.cc:526-598).  visit: num_node int32 words the
    caller zeroed once; stamp: nonzero and new to `visit` on every call; freq (optional): += 1 per closure node.
    Returns (closure, hop_offsets): closure[hop_offsets[h]:hop_offsets[h + 1]] = the nodes at distance exactly h
    (order within a hop unspecified); hop_offsets is an int64 device tensor of num_hop + 2 words."""
    _require_gpu(seeds)
    _i32(seeds)
    dev = seeds.device
    n = graph.c.num_node
    assert visit.numel() >= n and (freq is None or freq.numel() >= n), "visit / freq need num_node words"
    closure = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    hop_offsets = torch.empty(num_hop + 2, dtype=torch.int64, device=dev)
    ws = _workspace(lib().ggms_khop_closure_workspace_bytes(n), dev)
    check(lib().ggms_khop_closure(C.byref(graph.c), _ptr(seeds), seeds.numel(), num_hop, _ptr(visit), stamp, _ptr(freq),
                                  _ptr(closure), _ptr(hop_offsets), _ptr(ws), ws.numel() * 4, _stream()),
          "ggms_khop_closure")
    return closure[: int(hop_offsets[-1].item())], hop_offsets


def gather_scatter(out, src, src_index, dst_index, num=None, num_dev=None):
    """combine_cache_data / extract_miss_data / combine_miss_data (cuda_cache_manager_device.cu:209-275)."""
    _require_gpu(out)
    if num is None:
        num = (src_index if src_index is not None else dst_index).numel()
    check(lib().ggms_gather_scatter(_ptr(out), _ptr(src), _ptr(src_index), _ptr(dst_index), num, _ptr(num_dev),
                                    _dim_of(out), DTYPE_CODE[out.dtype], _stream()), "ggms_gather_scatter")
    return out


def gather_scatter_convert(out, src, src_index, dst_index, num=None, num_dev=None, src_row_mask=0xFFFFFFFF,
                           src_dtype=None):
    """ggms_gather_scatter_convert: out[dst(i), :] = src[src(i) & mask, :] delivered in out's dtype (src and out each
    float16, bfloat16 or float32, src also float8_e4m3fn or float8_e5m2; the same dtype on both sides is the plain
    gather).  src_dtype=Q8ROW: src is the uint8 (rows, row_bytes(Q8ROW, dim)) tensor of a row-scaled table, dim is out's."""
    _require_gpu(out)
    if num is None:
        num = (src_index if src_index is not None else dst_index).numel()
    src_dtype = src.dtype if src_dtype is None else src_dtype
    _check_q8row(src, src_dtype, _dim_of(out))
    check(lib().ggms_gather_scatter_convert(_ptr(out), _ptr(src), _ptr(src_index), _ptr(dst_index), num, _ptr(num_dev),
                                            _dim_of(out), _dtype_code(src_dtype), DTYPE_CODE[out.dtype], src_row_mask,
                                            _stream()), "ggms_gather_scatter_convert")
    return out


UPDATE_SGD, UPDATE_ADAGRAD = 0, 1  # GGMS_UPDATE_*: the rules of ggms_update_rows (include/ggms.h)


def update_rows(table, nodes, grad, rule, lr, eps=1e-10, state=None, num=None, num_dev=None):
    """ggms_update_rows: the float32 `table` (rows, dim) takes the gradient of the rows `nodes` names, in place --
    row i of the contiguous float32 `grad` belongs to table row nodes[i].  rule: UPDATE_SGD (w -= lr * g) or
    UPDATE_ADAGRAD (state += g * g; w -= lr * g / (sqrt(state) + eps), `state` shaped like the table), each operation
    one float32 operation.  nodes must be pairwise distinct; EMPTY_KEY entries are skipped.  With num_dev (device
    int64[1]) the count is read on the device and num is its upper bound."""
    _require_gpu(table)
    _i32(nodes)
    assert table.dtype == torch.float32 and table.stride(-1) == 1 and (table.dim() < 2 or table.stride(0) == _dim_of(table)), \
        "update_rows: the table is float32 with rows dim elements apart"
    assert grad.dtype == torch.float32 and grad.is_contiguous() and _dim_of(grad) == _dim_of(table), \
        f"update_rows: grad is a contiguous float32 (count, {_dim_of(table)}) tensor, not {grad.dtype} {tuple(grad.shape)}"
    if state is not None:
        assert state.dtype == torch.float32 and state.shape == table.shape and state.stride() == table.stride(), \
            "update_rows: state is shaped like the table"
    n = nodes.numel() if num is None else int(num)
    assert n <= nodes.numel() and n <= grad.shape[0], "update_rows: num beyond nodes / grad"
    check(lib().ggms_update_rows(_ptr(table), _ptr(state), _ptr(nodes), n, _ptr(num_dev), _ptr(grad), _dim_of(table),
                                 rule, lr, eps, _stream()), "ggms_update_rows")
    return table


def quantize_rows(src, out_dtype, out=None, first_row=0, check=True):
    """ggms_quantize_rows: the 2-D float32 / float16 device tensor `src` encoded into out_dtype -- torch.float16,
    torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2, or Q8ROW (returned as the uint8 (rows, row_bytes(Q8ROW, dim))
    tensor of a row-scaled table) -- bit for bit what datagen.quantize_features computes on the CPU.  A Q8ROW row that
    holds NaN or inf has no codes: with check=True the smallest such row (first_row + its index) is read back and raised
    as quantize_q8row raises it; with check=False its output row is zero bytes and nothing is said."""
    _require_gpu(src)
    assert src.dim() == 2 and src.dtype in (torch.float32, torch.float16), \
        f"quantize_rows reads a 2-D float32 or float16 tensor, not {src.dtype} {tuple(src.shape)}"
    rows, dim = src.shape
    if not (src.stride(1) == 1 and src.stride(0) == dim) and rows * dim:
        src = src.contiguous()
    code = _dtype_code(out_dtype)
    if out is None:
        out = torch.empty((rows, row_bytes(Q8ROW, dim)), dtype=torch.uint8, device=src.device) if code == Q8ROW else \
            torch.empty((rows, dim), dtype=out_dtype, device=src.device)
    assert out.is_contiguous() and out.device == src.device
    bad = None
    if code == Q8ROW and check:
        bad = torch.full((1,), -1, dtype=torch.int64, device=src.device)  # UINT64_MAX
    _lib.check(lib().ggms_quantize_rows(_ptr(out), code, _ptr(src), DTYPE_CODE[src.dtype], rows, dim, first_row, _ptr(bad),
                                        _stream()), "ggms_quantize_rows")
    if bad is not None:
        row = int(bad.item())
        if row != -1:
            raise ValueError(f"quantize_features: row {row} holds NaN or inf: a row-scaled table has no code for either")
    return out


class PartTable:
    """HOST array of shard base pointers (DeviceDistFeature / DeviceDistGraph, dist_graph.h:114-212): the operators
    hand the pointers to their kernels by value, at most GGMS_MAX_PARTS = 8 shards."""

    def __init__(self, ptrs, keep=None):
        if len(ptrs) > 9:  # GGMS_MAX_PARTS shards + the topology's host slot
            raise ValueError(f"PartTable: {len(ptrs)} pointers, the kernels carry at most GGMS_MAX_PARTS = 8 shards "
                             "(+ the host slot of a graph view)")
        self.n = len(ptrs)
        self.arr = (C.c_void_p * max(1, self.n))(*[int(p) for p in ptrs])
        self._keep = keep

    def ptr(self):
        return C.cast(self.arr, C.c_void_p)


def part_pointer_table(parts, device=None):
    """Pointer table of a list of shard tensors (kept alive by the table)."""
    return PartTable([p.data_ptr() for p in parts], keep=list(parts))


def gather_scatter_partition(out, parts_table, num_part, src_index, dst_index, num=None, num_dev=None):
    """combine_cache_data_for_partition (cuda_cache_manager_device.cu:277-299)."""
    _require_gpu(out)
    if num is None:
        num = src_index.numel()
    check(lib().ggms_gather_scatter_partition(_ptr(out), parts_table.ptr(), num_part, _ptr(src_index),
                                              _ptr(dst_index), num, _ptr(num_dev), _dim_of(out),
                                              DTYPE_CODE[out.dtype], _stream()), "ggms_gather_scatter_partition")
    return out


def extract_cached(out, nodes, table, parts_table, num_part, host_feat, num=None, num_dev=None, num_miss=None):
    """Fused GetMissCacheIndex + GPUExtractMissData + CombineCacheData (dist_loops.cc:1209-1285).
    table=None: full cache kept in node order (slot = node id), no table read per row."""
    _require_gpu(out)
    if num is None:
        num = nodes.numel()
    check(lib().ggms_extract_cached(_ptr(out), _ptr(nodes), num, _ptr(num_dev), _ptr(table), parts_table.ptr(),
                                    num_part, _ptr(host_feat), _dim_of(out), DTYPE_CODE[out.dtype], _ptr(num_miss),
                                    _stream()), "ggms_extract_cached")
    return out


def extract_cached_convert(out, src_dtype, nodes, table, parts_table, num_part, host_feat, num=None, num_dev=None,
                           num_miss=None):
    """extract_cached with every source (shards, host rows) in `src_dtype` and the rows delivered in out's dtype
    (src_dtype=Q8ROW: every source is uint8 rows of row_bytes(Q8ROW, dim) bytes)."""
    _require_gpu(out)
    if num is None:
        num = nodes.numel()
    _check_q8row(host_feat, src_dtype, _dim_of(out))
    check(lib().ggms_extract_cached_convert(_ptr(out), _ptr(nodes), num, _ptr(num_dev), _ptr(table), parts_table.ptr(),
                                            num_part, _ptr(host_feat), _dim_of(out), _dtype_code(src_dtype),
                                            DTYPE_CODE[out.dtype], _ptr(num_miss), _stream()),
          "ggms_extract_cached_convert")
    return out


def _feature_tiers(table, replica, parts_table, num_part, my_part, host_feat, host_row_mask=0):
    t = _lib.FeatureTiers()
    t.table = table.data_ptr() if table is not None else None
    t.replica = replica.data_ptr() if replica is not None else None
    t.num_replica = replica.shape[0] if replica is not None else 0
    t.parts = parts_table.ptr().value
    t.num_part, t.my_part = num_part, my_part
    t.host_feat = host_feat.data_ptr() if host_feat is not None else None
    t.host_row_mask = host_row_mask
    return t


def extract_tiered_convert(out, src_dtype, nodes, table, replica, parts_table, num_part, my_part, host_feat, num=None,
                           num_dev=None, tier_rows=None, host_row_mask=0):
    """extract_tiered with every tier in `src_dtype` and the rows delivered in out's dtype (src_dtype=Q8ROW: every
    tier is uint8 rows of row_bytes(Q8ROW, dim) bytes)."""
    _require_gpu(out)
    if num is None:
        num = nodes.numel()
    _check_q8row(host_feat, src_dtype, _dim_of(out))
    _check_q8row(replica, src_dtype, _dim_of(out))
    t = _feature_tiers(table, replica, parts_table, num_part, my_part, host_feat, host_row_mask)
    check(lib().ggms_extract_tiered_convert(_ptr(out), _ptr(nodes), num, _ptr(num_dev), C.byref(t), _dim_of(out),
                                            _dtype_code(src_dtype), DTYPE_CODE[out.dtype], _ptr(tier_rows), _stream()),
          "ggms_extract_tiered_convert")
    return out


def extract_tiered(out, nodes, table, replica, parts_table, num_part, my_part, host_feat, num=None, num_dev=None,
                   tier_rows=None):
    """Every tier of the GGMS store in one gather (include/ggms.h ggms_extract_tiered): replica of the hottest
    slots, local / peer shards (slot - |replica| modulo num_part), pinned host rows for uncached nodes.
    tier_rows: int64[4] device counters {host, remote shard, local shard, replica}, added to."""
    _require_gpu(out)
    if num is None:
        num = nodes.numel()
    t = _feature_tiers(table, replica, parts_table, num_part, my_part, host_feat)
    check(lib().ggms_extract_tiered(_ptr(out), _ptr(nodes), num, _ptr(num_dev), C.byref(t), _dim_of(out),
                                    DTYPE_CODE[out.dtype], _ptr(tier_rows), _stream()), "ggms_extract_tiered")
    return out


class LaunchTimer:
    """ggms_launch_timer_t (include/ggms.h): the next row gather issued by this thread carries the timer's two events ON
    its dispatch packet -- the kernel's own start / end timestamps, no marker packet on the stream.  `wait(stream)` makes
    another stream wait for that launch; `elapsed_us()` blocks until it has finished."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib().ggms_launch_timer_create(C.byref(self._h)), "ggms_launch_timer_create")

    def arm(self):
        check(lib().ggms_launch_timer_arm(self._h), "ggms_launch_timer_arm")
        return self

    def wait(self, stream=None):
        s = _stream() if stream is None else C.c_void_p(stream.cuda_stream)
        check(lib().ggms_launch_timer_wait(self._h, s), "ggms_launch_timer_wait")

    def elapsed_us(self):
        us = C.c_double(0)
        check(lib().ggms_launch_timer_elapsed_us(self._h, C.byref(us)), "ggms_launch_timer_elapsed_us")
        return us.value

    def span_us(self, last):
        """From the start of this timer's launch to the end of `last`'s (both waited for)."""
        us = C.c_double(0)
        check(lib().ggms_launch_timer_span_us(self._h, last._h, C.byref(us)), "ggms_launch_timer_span_us")
        return us.value

    def close(self):
        if self._h:
            lib().ggms_launch_timer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def batch_handoff(segments):
    """ggms_batch_handoff (include/ggms.h): every segment copied in ONE launch on the current stream, which belongs to
    the destination's device.  segments: (src, dst, count) with src / dst contiguous tensors of one element size and
    count an int (elements, on the host) or a one-element int64 device tensor read by the kernel at the launch; at
    most dst.numel() (and src.numel()) elements are copied."""
    n = len(segments)
    arr = (_lib.CopySeg * max(n, 1))()
    for k, (src, dst, count) in enumerate(segments):
        _require_gpu(dst)
        if dst.device.index != torch.cuda.current_device():
            raise _lib.GgmsError(f"batch_handoff: dst is on {dst.device}, the current stream on "
                                 f"cuda:{torch.cuda.current_device()}: launch it on the destination's device")
        assert src.is_contiguous() and dst.is_contiguous() and src.element_size() == dst.element_size()
        c = arr[k]
        c.src, c.dst = src.data_ptr(), dst.data_ptr()
        if isinstance(count, torch.Tensor):
            assert count.dtype == torch.int64 and count.is_cuda
            c.count_dev, c.count_host = count.data_ptr(), 0
        else:
            c.count_dev, c.count_host = None, int(count)
        c.max_count = min(src.numel(), dst.numel())
        c.elem_bytes = dst.element_size()
    check(lib().ggms_batch_handoff(arr, n, _stream()), "ggms_batch_handoff")


def queue_layout(max_edges, max_input, max_output, has_data=False):
    """ggms_queue_layout (include/ggms.h): offsets and size of one batch-queue slot for these bounds."""
    lay = _lib.QueueLayout()
    me = (C.c_size_t * len(max_edges))(*[int(x) for x in max_edges])
    check(lib().ggms_queue_layout(C.byref(lay), len(max_edges), me, int(max_input), int(max_output), int(bool(has_data))),
          "ggms_queue_layout")
    return lay


def _queue_batch(lay, rows, cols, datas, input_nodes, output_nodes, counts):
    b = _lib.QueueBatch()
    for i in range(lay.num_layer):
        b.row[i], b.col[i] = rows[i].data_ptr(), cols[i].data_ptr()
        b.data[i] = datas[i].data_ptr() if lay.has_data else None
    b.input_nodes, b.output_nodes, b.counts = input_nodes.data_ptr(), output_nodes.data_ptr(), counts.data_ptr()
    return b


def queue_pack(slot_ptr, lay, rows, cols, datas, input_nodes, output_nodes, counts, key, num_output):
    """ggms_queue_pack: one launch on the current stream writes the slot at device address `slot_ptr` (an int: mapped
    host memory or device memory).  Arrays are device tensors sized to the layout's bounds; counts holds the batch's
    3L + 8 counts words (int64, on the device), from which the kernel reads every length but the output nodes'."""
    b = _queue_batch(lay, rows, cols, datas, input_nodes, output_nodes, counts)
    check(lib().ggms_queue_pack(C.c_void_p(slot_ptr), C.byref(lay), C.byref(b), int(key), int(num_output), _stream()),
          "ggms_queue_pack")


def queue_unpack(slot_ptr, lay, rows, cols, datas, input_nodes, output_nodes, counts):
    """ggms_queue_unpack: one launch on the current stream copies the slot's arrays and counts words into the given
    device tensors, every length read from the slot's header by the kernel."""
    b = _queue_batch(lay, rows, cols, datas, input_nodes, output_nodes, counts)
    check(lib().ggms_queue_unpack(C.byref(b), C.c_void_p(slot_ptr), C.byref(lay), _stream()), "ggms_queue_unpack")


def owner_histogram(table, nodes, num_part, slots_out, counts, num=None, num_dev=None):
    """slots_out[i] = table[nodes[i]]; counts[p] += rows of the batch owned by shard p (p = num_part: host tier)."""
    _require_gpu(nodes)
    n = nodes.numel() if num is None else num
    check(lib().ggms_owner_histogram(_ptr(table), _ptr(nodes), n, _ptr(num_dev), num_part, _ptr(slots_out),
                                     _ptr(counts), _stream()), "ggms_owner_histogram")


def owner_bucket(slots, nodes, num_part, cursor, bucket_row, bucket_pos, num=None, num_dev=None):
    """Group the batch by owning shard: bucket p starts at cursor[p] (exclusive prefix of the histogram)."""
    _require_gpu(nodes)
    n = nodes.numel() if num is None else num
    check(lib().ggms_owner_bucket(_ptr(slots), _ptr(nodes), n, _ptr(num_dev), num_part, _ptr(cursor),
                                  _ptr(bucket_row), _ptr(bucket_pos), _stream()), "ggms_owner_bucket")


class _RawDevice:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


_TYPESTR = {torch.float32: "<f4", torch.float64: "<f8", torch.float16: "<f2", torch.uint8: "|u1",
            torch.int32: "<i4", torch.int8: "|i1", torch.int64: "<i8",
            # the OCP 8-bit floats have no typestr: bytes, re-viewed as the dtype
            torch.float8_e4m3fn: "|u1", torch.float8_e5m2: "|u1"}


class RegisteredHost:
    """A host array registered for device access (hipHostRegister, mapped): what DistGraph keeps in its last slot --
    the whole CSR in host memory, read by the sampling kernels over PCIe (dist_graph.cu:367-381) -- and what the
    `gpu_extract` miss tier is (dist_engine.cc:217-241).  `.tensor` aliases the host pages as a device tensor."""

    def __init__(self, array, device="cuda"):
        self.array = np.ascontiguousarray(array)  # kept alive: the registration pins THESE pages
        hip = C.CDLL("libamdhip64.so")
        self._hip = hip
        nbytes = self.array.nbytes
        self._host = C.c_void_p(self.array.ctypes.data)
        with torch.cuda.device(torch.device(device)):
            rc = hip.hipHostRegister(self._host, C.c_size_t(nbytes), C.c_uint(2))  # hipHostRegisterMapped
            if rc != 0:
                raise _lib.GgmsError(f"hipHostRegister({nbytes} bytes) -> {rc}")
            dp = C.c_void_p()
            rc = hip.hipHostGetDevicePointer(C.byref(dp), self._host, C.c_uint(0))
            if rc != 0:
                hip.hipHostUnregister(self._host)
                raise _lib.GgmsError(f"hipHostGetDevicePointer -> {rc}")
        kind = {4: "<i4", 8: "<i8", 1: "|u1", 2: "<i2"}[self.array.dtype.itemsize]
        self.ptr = dp.value
        self.tensor = torch.as_tensor(_RawDevice(self.ptr, self.array.shape, kind), device=torch.device(device))

    def close(self):
        if self._host is not None:
            self.tensor = None
            self._hip.hipHostUnregister(self._host)
            self._host = None


class SharedShard:
    """A GGMS shard that other processes can map: an allocation of its own (hipMalloc), published with
    hipIpcGetMemHandle and opened by peers with hipIpcOpenMemHandle (cuda/dist_graph.cu:228-272)."""

    def __init__(self, shape, dtype, device):
        self.shape, self.dtype, self.device = tuple(int(x) for x in shape), dtype, torch.device(device)
        nbytes = max(1, int(np.prod(self.shape))) * torch.empty(0, dtype=dtype).element_size()
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().ggms_device_alloc(C.byref(p), nbytes), "ggms_device_alloc")
        self.ptr = p.value
        self.tensor = torch.as_tensor(_RawDevice(self.ptr, self.shape, _TYPESTR[dtype]), device=self.device).view(dtype)
        self._imported = []

    def export_handle(self):
        buf = C.create_string_buffer(64)
        check(lib().ggms_ipc_export(C.c_void_p(self.ptr), buf), "ggms_ipc_export")
        return bytes(buf.raw)

    def import_peer(self, handle):
        """Map a peer's shard; returns its device address in this process."""
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().ggms_ipc_import(C.c_char_p(handle), C.byref(p)), "ggms_ipc_import")
        self._imported.append(p.value)
        return p.value

    def release_peers(self):
        """Unmap every peer shard opened through this holder (hipIpcCloseMemHandle)."""
        for p in self._imported:
            lib().ggms_ipc_release(C.c_void_p(p))
        self._imported = []

    def close(self):
        self.release_peers()
        if self.ptr:
            self.tensor = None
            lib().ggms_device_free(C.c_void_p(self.ptr))
            self.ptr = None


class _BatchBuffers:
    """What BatchSampler and PrefetchBatchSampler set up and slice alike; whatever differs between them is an argument."""

    def _init_capacity(self, graph, fanouts, sample_type, max_seeds, prob_table, alias_table):
        self.graph, self.fanouts, self.sample_type = graph, [int(f) for f in fanouts], sample_type
        if sample_type == KHOP2:
            graph.detach_heads()  # the draws permute graph.indices: inline list heads would go stale
        L = self.L = len(self.fanouts)
        self._f = (C.c_size_t * L)(*self.fanouts)
        self.max_seeds = max_seeds
        mi, me, mu = (C.c_size_t * L)(), (C.c_size_t * L)(), C.c_size_t(0)
        check(lib().ggms_sample_batch_capacity(max_seeds, self._f, L, mi, me, C.byref(mu)), "capacity")
        self.max_input, self.max_edges, self.max_unique = list(mi), list(me), mu.value
        self._keep = (prob_table, alias_table)
        self._extra = _lib.SampleExtra()
        self._extra.prob_table = prob_table.data_ptr() if prob_table is not None else None
        self._extra.alias_table = alias_table.data_ptr() if alias_table is not None else None

    def _init_states(self, stateless, seed, device, num_random_walk=0):
        """the RNG pool (None for the sample types in `stateless`)"""
        nstates = lib().ggms_random_states_count(self.sample_type, self._f, self.L, self.max_seeds, num_random_walk)
        nstates = max(nstates, (max(self.max_input) + 127) // 128 * 8, (max(self.max_input) + 1023) // 1024 * 256)
        if self.sample_type == RANDOM_WALK:
            nstates = max(nstates, lib().ggms_random_walk_num_states(max(self.max_input), num_random_walk))
        self.states = random_states(nstates, seed, device) if self.sample_type not in stateless else None

    def _layer_buffers(self, min_len, device):
        """one id buffer per layer at its edge bound (min_len at least), and the host array of their device pointers"""
        ts = [torch.empty(max(min_len, e), dtype=torch.int32, device=device) for e in self.max_edges]
        return ts, (C.c_void_p * self.L)(*[t.data_ptr() for t in ts])

    def _sliced(self, what, detail=None):
        """Sync; raise on a non-zero batch status; -> (the counts words as a host list, the per-layer slices)."""
        c = self.counts.cpu().tolist()
        status = c[COUNT_STATUS(self.L)]
        if status:  # a kernel of the batch hit a bound it must not hit: the outputs are invalid
            check_device_status(what)
            raise _lib.GgmsError(f"{what}: device status {status:#x}" + (detail(c) if detail else ""))
        return c, [dict(row=self.row[i][:c[COUNT_EDGES(i)]], col=self.col[i][:c[COUNT_EDGES(i)]],
                        num_src=c[COUNT_SRC(i)], num_dst=c[COUNT_DST(i)]) for i in range(self.L)]


class BatchSampler(_BatchBuffers):
    """DoGPUSample (dist_loops.cc:62-368) as one enqueue: buffers sized once, reused every batch.

    num_slots      output slots (the engine's batch slots): a batch's COO / counts / input-node copy stay valid
                   while later batches are being sampled.
    num_pipelines  batches that may be in flight at once, each with its own dedup table and workspace.  Call
                   sample() for consecutive batches from different streams; the shared RNG pool (and khop2's CSR)
                   is still consumed in call order (ggms_sample_extra_t.rng_wait / rng_done)."""

    def __init__(self, graph, fanouts, batch_size, sample_type=KHOP3, seed=0, device="cuda", direct_table=True,
                 prob_table=None, alias_table=None, random_walk_length=0, random_walk_restart_prob=0.0,
                 num_random_walk=0, num_slots=1, num_pipelines=1):
        # first batch of an epoch may be 1.25x (dist_shuffler_aligned.cc:137-140): size for it
        self._init_capacity(graph, fanouts, sample_type, int(batch_size * 1.25) + 1, prob_table, alias_table)
        L = self.L
        self.num_pipelines = num_pipelines
        self.hts = [OrderedHashTable(self.max_unique, device, num_node=graph.c.num_node if direct_table else None)
                    for _ in range(num_pipelines)]
        self.ht = self.hts[0]
        self._init_states(_STATELESS, seed, device, num_random_walk)
        self.num_slots = num_slots
        def per_slot():  # -> every slot's buffers, every slot's pointer array
            made = [self._layer_buffers(1, device) for _ in range(num_slots)]
            return [t for t, _ in made], [p for _, p in made]
        (self.rows, self._rows), (self.cols, self._cols) = per_slot(), per_slot()
        self.counts_slots = [torch.zeros(COUNTS_SAMPLE_WORDS(L), dtype=torch.int64, device=device)
                             for _ in range(num_slots)]
        self.input_nodes = [torch.empty(self.max_unique, dtype=torch.int32, device=device) for _ in range(num_slots)]
        self.row, self.col, self.counts = self.rows[0], self.cols[0], self.counts_slots[0]
        self.data = None
        self.datas = None
        if sample_type == RANDOM_WALK:
            self.datas, self._datas = per_slot()
            self.data = self.datas[0]
        # one extras struct per (pipeline, slot) use: filled in sample()
        self._extra.random_walk_length = random_walk_length
        self._extra.random_walk_restart_prob = random_walk_restart_prob
        self._extra.num_random_walk = num_random_walk
        if self.datas is not None:
            self._extra.data = C.cast(self._datas[0], C.c_void_p)
        wsb = lib().ggms_sample_batch_workspace_bytes(sample_type, self.max_seeds, self._f, L, C.byref(self._extra))
        self.wss = [_workspace(wsb, device) for _ in range(num_pipelines)]
        self.ws = self.wss[0]
        # batch-order events on the RNG pool; only needed when batches overlap
        self._events = []
        if num_pipelines > 1 and sample_type not in _STATELESS:
            for _ in range(num_pipelines):
                e = C.c_void_p()
                check(lib().ggms_event_create(C.byref(e)), "ggms_event_create")
                self._events.append(e)
        self._batch_no = 0
        self.active_pipelines = num_pipelines

    def use_pipelines(self, k):
        """Run the following batches on the first k of the allocated pipelines (1 <= k <= num_pipelines).  The caller
        has drained the device (nothing of an earlier batch is in flight): the batch order on the RNG pool starts anew."""
        assert 1 <= k <= self.num_pipelines
        self.active_pipelines = k
        self._batch_no = 0

    def __del__(self):
        try:
            for e in self._events:
                lib().ggms_event_destroy(e)
        except Exception:
            pass

    def sample(self, seeds, slot=0, copy_input_nodes=False, heavy_wait=None, distinct=False, labor_salt=0):
        """Enqueue one batch into output slot `slot`; read counts / row / col / ht.n2o after a sync.
        copy_input_nodes: also copy the unique list (ht.n2o, reused by a later batch) into the slot.
        distinct: the caller promises pairwise distinct seeds (ggms_sample_extra_t.seeds_distinct) -- a slice of a
        shuffled train set is; the seeds' insert / ordered scan / look-up launches are then skipped.
        labor_salt: khop_labor's batch salt (ggms_sample_extra_t.labor_salt); the other samplers ignore it.
        Batch b runs on pipeline b % num_pipelines (its table is `self.ht` until the next call)."""
        _i32(seeds)
        n = seeds.numel()
        assert n <= self.max_seeds
        b, K = self._batch_no, self.active_pipelines
        self._batch_no += 1
        pipe = b % K
        self.ht = self.hts[pipe]
        counts = self.counts_slots[slot]
        self.row, self.col, self.counts = self.rows[slot], self.cols[slot], counts
        ex = self._extra
        if self.datas is not None:
            ex.data = C.cast(self._datas[slot], C.c_void_p)
            self.data = self.datas[slot]
        if self._events and K > 1:
            ex.rng_wait = self._events[(b - 1) % K] if b > 0 else None
            ex.rng_done = self._events[pipe]
        else:
            ex.rng_wait = ex.rng_done = None
        # heavy_wait (torch.cuda.Event): the last layer's sampler launch waits for it (ggms_sample_extra_t.heavy_wait)
        ex.heavy_wait = C.c_void_p(heavy_wait.cuda_event) if heavy_wait is not None else None
        ex.seeds_distinct = 1 if distinct else 0
        ex.labor_salt = labor_salt & 0xFFFFFFFF
        ws = self.wss[pipe]
        self._seed_ids_of = None if distinct else (n, ws)
        # copy_input_nodes: the slot keeps the batch's unique list.  The table's n2o buffer is the caller's
        # (ggms_hashtable_t is plain data), so the batch simply builds the list IN the slot's buffer -- no copy
        self._n2o = self.input_nodes[slot] if copy_input_nodes else self.ht.n2o
        self.ht.c.n2o = self._n2o.data_ptr()
        self.ht.c.n2o_size = self._n2o.numel()
        check(lib().ggms_sample_batch(self.sample_type, C.byref(self.graph.c), _ptr(seeds), n, self._f, self.L,
                                      C.byref(self.ht.c), _ptr(self.states),
                                      self.states.shape[0] if self.states is not None else 0, self._rows[slot],
                                      self._cols[slot], _ptr(counts), C.byref(ex), _ptr(ws), ws.numel() * 4,
                                      _stream()),
              "ggms_sample_batch")

    def seed_ids(self):
        """Local ids of the raw seeds of the last batch (ggms_sample_batch_seed_ids): a device view into that batch's
        workspace, valid until its pipeline samples again.  input_nodes[seed_ids[p]] == seeds[p]; the ids a
        link-prediction batch's pairs are made of.  Not for a batch sampled with distinct=True (its ids are positions)."""
        if getattr(self, "_seed_ids_of", None) is None:
            raise _lib.GgmsError("seed_ids(): the last batch took the distinct-seeds path (or nothing was sampled)")
        n, ws = self._seed_ids_of
        p = C.c_void_p()
        check(lib().ggms_sample_batch_seed_ids(self.sample_type, n, self._f, self.L, C.byref(self._extra), _ptr(ws),
                                               C.byref(p)), "ggms_sample_batch_seed_ids")
        off = (p.value - ws.data_ptr()) // 4
        return ws[off: off + n]

    def drop_pair_edges(self, pair_src, pair_dst, which):
        """ggms_drop_pair_edges on the last sampled batch: the edges between the pairs (local ids, e.g. slices of
        seed_ids()) leave its layers; result() then shows the filtered layers.  -> dropped edges per layer (device)."""
        return drop_pair_edges(pair_src, pair_dst, which, self.row, self.col, self.counts, self.max_edges)

    def result(self):
        """Sync and slice the outputs (host round trip: for tests and hand-off, not for the hot loop)."""
        c, layers = self._sliced("ggms_sample_batch")
        for i, lay in enumerate(layers):
            lay["data"] = self.data[i][:c[COUNT_EDGES(i)]] if self.data is not None else None
        return dict(layers=layers, input_nodes=self._n2o[: c[COUNT_INPUT(self.L)]])


def prefetch_capacity(num_seeds, fanouts, indptr_host, max_edges_budget):
    """ggms_sample_batch_prefetch_capacity: (max_prefetch_edges, max_input_nodes) of an arch4 batch of num_seeds seeds.
    indptr_host: the host CSR offsets (uint32 / int32 numpy array of num_node + 1 entries)."""
    L = len(fanouts)
    f = (C.c_size_t * L)(*[int(x) for x in fanouts])
    ip = np.ascontiguousarray(indptr_host).view(np.uint32)
    me, mi = C.c_size_t(0), C.c_size_t(0)
    check(lib().ggms_sample_batch_prefetch_capacity(int(num_seeds), f, L, ip.ctypes.data_as(C.c_void_p), ip.size - 1,
                                                    int(max_edges_budget), C.byref(me), C.byref(mi)),
          "ggms_sample_batch_prefetch_capacity")
    return me.value, mi.value


class PrefetchBatchSampler(_BatchBuffers):
    """arch4's batch (DoGPUSampleDyCache, cuda_loops.cc:294-524) through ggms_sample_batch_prefetch: the layers of
    BatchSampler, the expansion after the second-to-last layer, the last layer sampled from the set before it.
    One slot, one pipeline; the RNG pool is BatchSampler's for the same arguments."""

    def __init__(self, graph, indptr_host, fanouts, batch_size, sample_type=KHOP0, seed=0, device="cuda",
                 prob_table=None, alias_table=None, max_edges_budget=1 << 26, max_seeds=None):
        self._init_capacity(graph, fanouts, sample_type, int(batch_size * 1.25) + 1 if max_seeds is None else int(max_seeds),
                            prob_table, alias_table)
        L = self.L
        self.max_prefetch_edges, self.max_unique = prefetch_capacity(self.max_seeds, self.fanouts, indptr_host,
                                                                     max_edges_budget)
        self.ht = OrderedHashTable(self.max_unique, device, num_node=graph.c.num_node)
        self._init_states((KHOP0,), seed, device)
        (self.row, self._rows), (self.col, self._cols) = self._layer_buffers(4, device), self._layer_buffers(4, device)
        self.counts = torch.zeros(COUNTS_WORDS(L), dtype=torch.int64, device=device)
        wsb = lib().ggms_sample_batch_prefetch_workspace_bytes(sample_type, self.max_seeds, self._f, L,
                                                               C.byref(self._extra), self.max_prefetch_edges)
        self.ws = _workspace(wsb, device)

    def sample(self, seeds, distinct=False, input_final=None):
        """Enqueue one batch; input_final (torch.cuda.Event, optional) is recorded once the input nodes are final."""
        _i32(seeds)
        n = seeds.numel()
        assert n <= self.max_seeds
        self._extra.seeds_distinct = 1 if distinct else 0
        ev = C.c_void_p(input_final.cuda_event) if input_final is not None else None
        check(lib().ggms_sample_batch_prefetch(self.sample_type, C.byref(self.graph.c), _ptr(seeds), n, self._f, self.L,
                                               C.byref(self.ht.c), _ptr(self.states),
                                               self.states.shape[0] if self.states is not None else 0, self._rows,
                                               self._cols, _ptr(self.counts), C.byref(self._extra),
                                               self.max_prefetch_edges, None, ev, _ptr(self.ws), self.ws.numel() * 4,
                                               _stream()),
              "ggms_sample_batch_prefetch")

    def result(self):
        """Sync and slice the outputs; raises on a non-zero batch status (GGMS_STATUS_PREFETCH_FULL: expansion over
        capacity, `needed` edges)."""
        needed = COUNT_EXPANSION(self.L)
        c, layers = self._sliced("ggms_sample_batch_prefetch", lambda c: f" (expansion needed {c[needed]} edges, "
                                                                         f"capacity {self.max_prefetch_edges})")
        return dict(layers=layers, input_nodes=self.ht.n2o[: c[COUNT_INPUT(self.L)]], expansion_edges=c[needed])


class TemporalBatchSampler(_BatchBuffers):
    """ggms_sample_batch_temporal: BatchSampler's layers with khop_temporal as the sampler.  One slot, one pipeline, one
    cut table (8 bytes per node, zeroed here) whose stamp goes up by one per batch."""

    def __init__(self, graph, edge_time, fanouts, batch_size, pick=PICK_UNIFORM, device="cuda", direct_table=True,
                 max_seeds=None):
        self._init_capacity(graph, fanouts, KHOP_TEMPORAL, int(batch_size * 1.25) + 1 if max_seeds is None else int(max_seeds),
                            None, None)
        _require_gpu(_i32(edge_time))
        self.edge_time, self.pick = edge_time, pick
        self.ht = OrderedHashTable(self.max_unique, device, num_node=graph.c.num_node if direct_table else None)
        self.states = None
        (self.row, self._rows), (self.col, self._cols) = self._layer_buffers(1, device), self._layer_buffers(1, device)
        self.eid, self._eids = self._layer_buffers(1, device)
        self.node_cut = torch.empty(max(1, self.max_unique), dtype=torch.int32, device=device)
        self.counts = torch.zeros(COUNTS_SAMPLE_WORDS(self.L), dtype=torch.int64, device=device)
        self.cut_table = torch.zeros(max(1, graph.c.num_node), dtype=torch.int64, device=device)
        self.stamp = 0
        wsb = lib().ggms_sample_batch_temporal_workspace_bytes(self.max_seeds, self._f, self.L, C.byref(self._extra))
        self.ws = _workspace(wsb, device)
        self._n = 0

    def sample(self, seeds, seed_time, salt=0, stamp=None):
        """Enqueue one batch: seeds[j] is sampled strictly before min(seed_time over the occurrences of that node).
        stamp: the batch's stamp on the cut table (default: the last one + 1; after 0xffffffff the table is zeroed)."""
        _i32(seeds), _i32(seed_time)
        n = self._n = seeds.numel()
        assert n <= self.max_seeds and seed_time.numel() == n
        if stamp is None:
            if self.stamp == 0xFFFFFFFF:
                self.cut_table.zero_()
                self.stamp = 0
            stamp = self.stamp + 1
        self.stamp = stamp
        t = _lib.Temporal(self.edge_time.data_ptr(), self.cut_table.data_ptr(), stamp, self.pick)
        self._extra.labor_salt = salt & 0xFFFFFFFF
        check(lib().ggms_sample_batch_temporal(C.byref(self.graph.c), _ptr(seeds), _ptr(seed_time), n, self._f, self.L,
                                               C.byref(self.ht.c), self._rows, self._cols, self._eids,
                                               _ptr(self.node_cut), _ptr(self.counts), C.byref(t), C.byref(self._extra),
                                               _ptr(self.ws), self.ws.numel() * 4, _stream()),
              "ggms_sample_batch_temporal")

    def seed_ids(self):
        """Local ids of the raw seeds of the last batch (ggms_sample_batch_seed_ids)."""
        p = C.c_void_p()
        check(lib().ggms_sample_batch_seed_ids(KHOP_TEMPORAL, self._n, self._f, self.L, C.byref(self._extra),
                                               _ptr(self.ws), C.byref(p)), "ggms_sample_batch_seed_ids")
        off = (p.value - self.ws.data_ptr()) // 4
        return self.ws[off: off + self._n]

    def result(self):
        """Sync and slice the outputs: BatchSampler.result()'s, each layer with its `eid`, and `node_cut`."""
        c, layers = self._sliced("ggms_sample_batch_temporal")
        for i, lay in enumerate(layers):
            lay["eid"] = self.eid[i][:c[COUNT_EDGES(i)]]
        n_in = c[COUNT_INPUT(self.L)]
        return dict(layers=layers, input_nodes=self.ht.n2o[:n_in], node_cut=self.node_cut[:n_in])


class TypedBatchSampler(_BatchBuffers):
    """ggms_sample_batch_typed: BatchSampler's layers with khop_typed as the sampler.  One slot, one pipeline.
    type_fanouts: num_layer rows of num_type fanouts, indexed by layer id like `fanouts`; the batch's fanouts are the
    rows' sums."""

    def __init__(self, graph, edge_type, type_fanouts, batch_size, device="cuda", direct_table=True, max_seeds=None):
        rows = [[int(k) for k in row] for row in type_fanouts]
        self.num_type = len(rows[0])
        assert all(len(row) == self.num_type for row in rows), "type_fanouts: every layer has one fanout per edge type"
        self._init_capacity(graph, [sum(row) for row in rows], KHOP_TYPED,
                            int(batch_size * 1.25) + 1 if max_seeds is None else int(max_seeds), None, None)
        _require_gpu(_u8(edge_type))
        self.edge_type, self.type_fanouts = edge_type, rows
        self._tf = (C.c_uint32 * (self.L * self.num_type))(*[k for row in rows for k in row])
        self._typed = _lib.Typed(edge_type.data_ptr(), self.num_type, self._tf)
        self.ht = OrderedHashTable(self.max_unique, device, num_node=graph.c.num_node if direct_table else None)
        self.states = None
        (self.row, self._rows), (self.col, self._cols) = self._layer_buffers(1, device), self._layer_buffers(1, device)
        self.eid, self._eids = self._layer_buffers(1, device)
        self.etype = [torch.empty(max(1, e), dtype=torch.uint8, device=device) for e in self.max_edges]
        self._etypes = (C.c_void_p * self.L)(*[t.data_ptr() for t in self.etype])
        self.counts = torch.zeros(COUNTS_SAMPLE_WORDS(self.L), dtype=torch.int64, device=device)
        wsb = lib().ggms_sample_batch_typed_workspace_bytes(self.max_seeds, self._f, self.L, self.num_type,
                                                            C.byref(self._extra))
        self.ws = _workspace(wsb, device)
        self._n = 0

    def sample(self, seeds, salt=0):
        """Enqueue one batch; salt: the batch salt (layer i samples under fmix32(salt + 0x9e3779b9 * (i + 1)))."""
        _i32(seeds)
        n = self._n = seeds.numel()
        assert n <= self.max_seeds
        self._extra.labor_salt = salt & 0xFFFFFFFF
        check(lib().ggms_sample_batch_typed(C.byref(self.graph.c), _ptr(seeds), n, self._f, self.L, C.byref(self.ht.c),
                                            self._rows, self._cols, self._eids, self._etypes, _ptr(self.counts),
                                            C.byref(self._typed), C.byref(self._extra), _ptr(self.ws),
                                            self.ws.numel() * 4, _stream()), "ggms_sample_batch_typed")

    def seed_ids(self):
        """Local ids of the raw seeds of the last batch (ggms_sample_batch_seed_ids)."""
        p = C.c_void_p()
        check(lib().ggms_sample_batch_seed_ids(KHOP_TYPED, self._n, self._f, self.L, C.byref(self._extra),
                                               _ptr(self.ws), C.byref(p)), "ggms_sample_batch_seed_ids")
        off = (p.value - self.ws.data_ptr()) // 4
        return self.ws[off: off + self._n]

    def result(self):
        """Sync and slice the outputs: BatchSampler.result()'s, each layer with its `eid` and `etype`."""
        c, layers = self._sliced("ggms_sample_batch_typed")
        for i, lay in enumerate(layers):
            lay["eid"] = self.eid[i][:c[COUNT_EDGES(i)]]
            lay["etype"] = self.etype[i][:c[COUNT_EDGES(i)]]
        return dict(layers=layers, input_nodes=self.ht.n2o[:c[COUNT_INPUT(self.L)]])


def dynamic_cache_reset(stamps):
    """dynamic_cache: zero the stamp table (int64, one word per node)."""
    check(lib().ggms_dynamic_cache_reset(_ptr(stamps), stamps.numel(), _stream()), "ggms_dynamic_cache_reset")


def extract_dynamic(out, nodes, stamps, seq, prev_feat, host_feat, num=None, num_dev=None, num_miss=None):
    """dynamic_cache gather of batch `seq`: rows batch seq - 1 published come from prev_feat, the rest from host_feat."""
    _require_gpu(out)
    if num is None:
        num = nodes.numel()
    check(lib().ggms_extract_dynamic(_ptr(out), _ptr(nodes), num, _ptr(num_dev), _ptr(stamps), int(seq), _ptr(prev_feat),
                                     _ptr(host_feat), _dim_of(out), DTYPE_CODE[out.dtype], _ptr(num_miss), _stream()),
          "ggms_extract_dynamic")
    return out


def dynamic_cache_publish(stamps, nodes, seq, num=None, num_dev=None):
    """stamps[nodes[i]] = (seq << 32) | i: batch seq's rows are in its own feature buffer."""
    if num is None:
        num = nodes.numel()
    check(lib().ggms_dynamic_cache_publish(_ptr(stamps), _ptr(nodes), num, _ptr(num_dev), int(seq), _stream()),
          "ggms_dynamic_cache_publish")
