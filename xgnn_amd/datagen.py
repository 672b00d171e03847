"""Seeded synthetic datasets shaped like the reference's.

There is no network, so ogbn-products / papers100M cannot be downloaded; these
generators produce power-law in-neighbour CSRs with the same node count, mean
degree, feature width and train-set size, plus exactly representable features
so gathers can be checked bit for bit.  numpy only (host side), but for the FP8 tables, which use torch's CPU casts.
"""
import numpy as np

PRESETS = {
    # name: num_node, mean_deg, alpha, dmax, feat_dim, num_class, num_train
    "products": dict(num_node=2_449_029, mean_deg=50.5, alpha=0.75, dmax=17_000, feat_dim=100, num_class=47,
                     num_train=196_615),
    "papers100M": dict(num_node=111_059_956, mean_deg=14.55, alpha=0.7, dmax=300_000, feat_dim=128, num_class=172,
                       num_train=1_207_179),
    # com-friendster as the reference generates it (datagen/friendster.py:68-69: 65.6 M nodes, 1.8 G directed edges;
    # synthetic 256-dim f32 features per BASELINE configs[4], 1 % of the nodes as the train set)
    "friendster": dict(num_node=65_608_366, mean_deg=27.53, alpha=0.7, dmax=6_000, feat_dim=256, num_class=100,
                       num_train=656_083),
    "tiny": dict(num_node=20_000, mean_deg=30.0, alpha=0.75, dmax=2_000, feat_dim=100, num_class=47,
                 num_train=4_000),
}


def powerlaw_degrees(num_node, mean_deg, alpha, dmax, rng):
    """d_v = min(dmax, floor(c * u^-alpha)), c tuned so that the mean is mean_deg."""
    u = rng.random_sample(num_node)
    base = u ** (-alpha)
    calib = base if num_node <= (1 << 22) else base[:: num_node // (1 << 22)]  # calibrate c on a subsample
    lo, hi = 1e-3, 1e6
    for _ in range(60):  # bisection on c
        c = 0.5 * (lo + hi)
        m = np.minimum(dmax, np.floor(c * calib)).mean()
        if m < mean_deg:
            lo = c
        else:
            hi = c
    return np.minimum(dmax, np.floor(hi * base)).astype(np.int64)


def _host_threads():
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


def make_graph(preset="products", seed=42, chunk=1 << 24, neighbour_skew=0.0, threads=None):
    """Returns dict(indptr uint32[N+1], indices uint32[E], train_set uint32[T], meta).

    neighbour_skew = 0 (the default everywhere): neighbour ids uniform over the nodes.
    neighbour_skew = p in (0, 1]: each neighbour is, with probability p, the OWNER OF A UNIFORMLY RANDOM EDGE SLOT
    (probability proportional to the node's degree -- the hubs of the power law turn up in many lists, as in a real
    symmetrised graph) and uniform otherwise.  Chunks are seeded one by one, so the result does not depend on the
    number of host threads that fill them."""
    p = dict(PRESETS[preset]) if isinstance(preset, str) else dict(preset)
    rng = np.random.RandomState(seed)
    n = p["num_node"]
    deg = powerlaw_degrees(n, p["mean_deg"], p["alpha"], p["dmax"], rng)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    num_edge = int(indptr[-1])
    assert num_edge < 2 ** 32, "IdType is uint32 (constant.h:28): num_edge must stay below 2^32"
    indices = np.empty(num_edge, dtype=np.uint32)
    owner = None
    if neighbour_skew > 0:  # owner[e] = the node whose list holds edge slot e
        owner = np.repeat(np.arange(n, dtype=np.uint32), deg)

    def fill(s):  # chunked: bounded temporaries; numpy releases the GIL in randint / take
        e = min(num_edge, s + chunk)
        ids = np.random.RandomState(1234 + s // chunk).randint(0, n, size=e - s, dtype=np.int64)
        if owner is not None:
            r2 = np.random.RandomState(991234 + s // chunk)
            slot = r2.randint(0, num_edge, size=e - s, dtype=np.int64)
            hub = r2.random_sample(e - s) < neighbour_skew
            ids = np.where(hub, owner.take(slot), ids)
        indices[s:e] = ids

    starts = range(0, num_edge, chunk)
    nt = threads or _host_threads()
    if nt > 1 and len(starts) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(nt) as ex:
            list(ex.map(fill, starts))
    else:
        for s in starts:
            fill(s)
    del owner
    train = np.random.RandomState(seed + 1).permutation(n)[: p["num_train"]].astype(np.uint32)
    p["num_edge"] = num_edge
    p["neighbour_skew"] = float(neighbour_skew)
    return dict(indptr=indptr.astype(np.uint32), indices=indices, train_set=train, meta=p)


def degree_rank(indptr):
    """cache_by_degree.bin equivalent: node ids by descending in-degree (stable)."""
    deg = (indptr[1:].astype(np.int64) - indptr[:-1].astype(np.int64))
    return np.argsort(-deg, kind="stable").astype(np.uint32)


def edge_weights(graph, policy="default", seed=0):
    """Per-edge weights in the spirit of the reference's weight tool (create_alias_table.cc:36-60,75-92), seeded:
    'default' = integers 1..10, 'inverse_src_degree' = 1 / out-degree of the neighbour, 'src_suffix' = 100 for
    neighbours with out-degree < 10 else 1."""
    ip, ix = graph["indptr"], graph["indices"]
    if policy == "default":
        return np.random.RandomState(seed).randint(1, 11, size=ix.size).astype(np.float32)
    out_deg = np.bincount(ix, minlength=ip.size - 1).astype(np.int64)
    if policy == "inverse_src_degree":
        return (1.0 / out_deg[ix]).astype(np.float32)
    if policy == "src_suffix":
        return np.where(out_deg[ix] < 10, 100.0, 1.0).astype(np.float32)
    raise ValueError(policy)


def build_alias_tables(indptr, indices, weights, num_threads=8):
    """prob_table / alias_table of the alias-method samplers from per-edge weights (create_alias_table.cc:105-170);
    the alias slot holds the GLOBAL node id of the donor neighbour.  Host-only entry point of the library."""
    import ctypes as C
    from ._lib import check, lib
    ip = np.ascontiguousarray(indptr, np.uint32)
    ix = np.ascontiguousarray(indices, np.uint32)
    w = np.ascontiguousarray(weights, np.float32)
    assert w.size == ix.size
    prob, alias = np.empty(ix.size, np.float32), np.empty(ix.size, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(lib().ggms_build_alias_table_host(vp(ip), vp(ix), ip.size - 1, vp(w), vp(prob), vp(alias), num_threads),
          "ggms_build_alias_table_host")
    return prob, alias


def build_prob_prefix_table(indptr, weights, num_threads=8):
    """prob_prefix_table of the inverse-CDF sampler: running float sum per neighbour list
    (create_prob_prefix_table.cc:94-123)."""
    import ctypes as C
    from ._lib import check, lib
    ip = np.ascontiguousarray(indptr, np.uint32)
    w = np.ascontiguousarray(weights, np.float32)
    out = np.empty(w.size, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(lib().ggms_build_prob_prefix_table_host(vp(ip), ip.size - 1, vp(w), vp(out), num_threads),
          "ggms_build_prob_prefix_table_host")
    return out


def write_dataset(path, graph, feat=None, label=None, valid_frac=0.02, test_frac=0.05, feat_dtype="F32", weights=None,
                  minimal=False, train_edges=None, edge_feat=None, edge_feat_dtype="F32", edge_time=None, edge_type=None,
                  num_edge_type=None, node_type=None, num_node_type=None, node_feat=None):
    """Write a dataset directory in the reference's on-disk format (datagen/README.md:37-51,
    samgraph/common/constant.cc:23-51, engine.cc:109-443): meta.txt (tab separated) + raw little-endian
    arrays: indptr/indices/train_set/test_set/valid_set/cache_by_* uint32, feat row-major, label int64;
    feat_dtype "F8E4M3" / "F8E5M2": feat is a torch.float8_e4m3fn / float8_e5m2 tensor, or its bytes as a uint8 array;
    feat_dtype "Q8ROW": feat is the packed (n, q8row_stride(feat_dim)) uint8 rows of pack_q8row;
    weights (one float per edge) adds prob_table.bin / alias_table.bin / prob_prefix_table.bin.
    train_edges (uint32 positions in indices, each below the edge count) adds train_edge_set.bin, the set a
    link_prediction run shuffles (config key `task`); without it such a run takes every edge.
    edge_feat (one row per edge, in the order of indices; a 1-d array is dim 1) adds edge_feat.bin and the meta keys
    EDGE_FEAT_DIM / EDGE_FEAT_DATA_TYPE, the table of config key `edge_feat`; edge_feat_dtype names an element type
    (FP8: as for feat), not Q8ROW.
    edge_time (one uint32 per edge, in the order of indices, non-decreasing inside every node's list -- see
    sort_lists_by_time) adds edge_time.bin, the times `sample_type khop_temporal` samples before.
    edge_type (one uint8 per edge, in the order of indices, non-decreasing inside every node's list -- see
    sort_lists_by_type -- and below num_edge_type, 1 .. 32) adds edge_type.bin and the meta key NUM_EDGE_TYPE, the
    relations `sample_type khop_typed` has a fanout for.
    node_type (one uint8 per node id, below num_node_type, 1 .. 32) adds node_type.bin and the meta key NUM_NODE_TYPE,
    the types a heterogeneous batch groups its nodes by (relation_types derives consistent relations from them).
    node_feat (needs node_type; one entry per node type: a 2-d float32 / float16 numpy array, a 2-d float32 / float16 /
    bfloat16 torch tensor, or None for a type without features) adds node_feat_<t>.bin for every type that has a table
    and the meta keys NODE_FEAT_DIM_<t> (0 without a table) / NODE_FEAT_DATA_TYPE_<t>, the tables of config key
    `typed_feat`.  Entry t has one row per node of type t; row k belongs to the k-th such node in ascending node id.
    minimal: what a sampling + extract run needs and nothing that costs minutes at papers100M size -- one-node
    valid / test sets instead of random slices of the complement, no cache_by_random.bin."""
    import os
    os.makedirs(path, exist_ok=True)
    ip, ix, train, meta = graph["indptr"], graph["indices"], graph["train_set"], graph["meta"]
    n = ip.size - 1
    if minimal:
        valid = test = np.zeros(1, np.uint32)
    else:
        rng = np.random.RandomState(7)
        rest = np.setdiff1d(np.arange(n, dtype=np.uint32), train, assume_unique=False)
        rng.shuffle(rest)
        nv, nt = int(n * valid_frac), int(n * test_frac)
        valid, test = rest[:nv].astype(np.uint32), rest[nv:nv + nt].astype(np.uint32)
    ip.astype(np.uint32).tofile(os.path.join(path, "indptr.bin"))
    ix.astype(np.uint32).tofile(os.path.join(path, "indices.bin"))
    train.astype(np.uint32).tofile(os.path.join(path, "train_set.bin"))
    valid.tofile(os.path.join(path, "valid_set.bin"))
    test.tofile(os.path.join(path, "test_set.bin"))
    if train_edges is not None:
        train_edges = np.ascontiguousarray(train_edges, dtype=np.uint32)
        assert train_edges.size == 0 or int(train_edges.max()) < ix.size, "train_edges: positions in indices, below the edge count"
        train_edges.tofile(os.path.join(path, "train_edge_set.bin"))
    if feat is not None:
        if feat_dtype in FP8_FORMATS:
            feat = _fp8_bytes(feat, feat_dtype)
        if feat_dtype == "Q8ROW":
            feat = np.asarray(feat)
            assert feat.dtype == np.uint8 and feat.shape == (n, q8row_stride(meta["feat_dim"])), \
                f"a Q8ROW table is the packed uint8 rows ({n}, {q8row_stride(meta['feat_dim'])}), not {feat.dtype} {feat.shape}"
        np.ascontiguousarray(feat).tofile(os.path.join(path, "feat.bin"))
    if edge_feat is not None:
        assert edge_feat_dtype != "Q8ROW", "edge_feat_dtype: an element type; a row-scaled edge table is not built"
        if edge_feat_dtype in FP8_FORMATS:
            edge_feat = _fp8_bytes(edge_feat, edge_feat_dtype)
        edge_feat = np.ascontiguousarray(edge_feat)
        edge_feat = edge_feat.reshape(edge_feat.shape[0], -1)
        assert edge_feat.shape[0] == ix.size, f"edge_feat: one row per edge ({ix.size}), not {edge_feat.shape[0]}"
        edge_feat.tofile(os.path.join(path, "edge_feat.bin"))
    if edge_time is not None:
        edge_time = np.ascontiguousarray(edge_time, dtype=np.uint32)
        assert edge_time.shape == (ix.size,), f"edge_time: one time per edge ({ix.size}), not {edge_time.shape}"
        bad = first_unsorted_list(ip, edge_time)
        assert bad is None, (f"edge_time: the times of node {bad}'s list are not non-decreasing "
                             "(datagen.sort_lists_by_time re-sorts a graph)")
        edge_time.tofile(os.path.join(path, "edge_time.bin"))
    if edge_type is not None:
        assert num_edge_type is not None and 1 <= int(num_edge_type) <= 32, \
            f"num_edge_type: 1 .. 32 (GGMS_MAX_EDGE_TYPES), not {num_edge_type}"
        assert np.asarray(edge_type).size == 0 or (0 <= int(np.min(edge_type)) and int(np.max(edge_type)) < 256), \
            "edge_type: uint8 values"
        edge_type = np.ascontiguousarray(edge_type, dtype=np.uint8)
        assert edge_type.shape == (ix.size,), f"edge_type: one type per edge ({ix.size}), not {edge_type.shape}"
        bad = first_unsorted_list(ip, edge_type)
        assert bad is None, (f"edge_type: the types of node {bad}'s list are not non-decreasing "
                             "(datagen.sort_lists_by_type re-sorts a graph)")
        over = np.flatnonzero(edge_type >= int(num_edge_type))
        assert over.size == 0, (f"edge_type: node {int(np.searchsorted(ip, over[0], side='right') - 1) if over.size else 0}"
                                f"'s list holds a type >= num_edge_type = {num_edge_type}")
        edge_type.tofile(os.path.join(path, "edge_type.bin"))
    else:
        assert num_edge_type is None, "num_edge_type without edge_type"
    if node_type is not None:
        node_type = _checked_node_types(node_type, num_node_type, n)
        node_type.tofile(os.path.join(path, "node_type.bin"))
    else:
        assert num_node_type is None, "num_node_type without node_type"
    typed = _checked_node_feat(node_feat, node_type, num_node_type) if node_feat is not None else None
    for t, (table, _) in enumerate(typed or []):
        if table is not None:
            table.tofile(os.path.join(path, f"node_feat_{t}.bin"))
    if label is not None:
        np.ascontiguousarray(label, dtype=np.int64).tofile(os.path.join(path, "label.bin"))
    if weights is not None:  # tables of the weighted samplers (engine.cc:372-384 loads them by these names)
        prob, alias = build_alias_tables(ip, ix, weights)
        prob.tofile(os.path.join(path, "prob_table.bin"))
        alias.tofile(os.path.join(path, "alias_table.bin"))
        build_prob_prefix_table(ip, weights).tofile(os.path.join(path, "prob_prefix_table.bin"))
    degree_rank(ip).tofile(os.path.join(path, "cache_by_degree.bin"))
    if not minimal:
        np.random.RandomState(11).permutation(n).astype(np.uint32).tofile(os.path.join(path, "cache_by_random.bin"))
    with open(os.path.join(path, "meta.txt"), "w") as f:
        for k, v in [("NUM_NODE", n), ("NUM_EDGE", ix.size), ("FEAT_DIM", meta["feat_dim"]),
                     ("NUM_CLASS", meta["num_class"]), ("NUM_TRAIN_SET", train.size), ("NUM_TEST_SET", test.size),
                     ("NUM_VALID_SET", valid.size)]:
            f.write(f"{k}\t{v}\n")
        if feat_dtype != "F32":
            f.write(f"FEAT_DATA_TYPE\t{feat_dtype}\n")
        if edge_feat is not None:
            f.write(f"EDGE_FEAT_DIM\t{edge_feat.shape[1]}\n")
            f.write(f"EDGE_FEAT_DATA_TYPE\t{edge_feat_dtype}\n")
        if edge_type is not None:
            f.write(f"NUM_EDGE_TYPE\t{int(num_edge_type)}\n")
        if node_type is not None:
            f.write(f"NUM_NODE_TYPE\t{int(num_node_type)}\n")
        for t, (table, dtype_name) in enumerate(typed or []):
            f.write(f"NODE_FEAT_DIM_{t}\t{0 if table is None else table.shape[1]}\n")
            f.write(f"NODE_FEAT_DATA_TYPE_{t}\t{dtype_name}\n")
    return path


MAX_NODE_TYPES = 32  # GGMS_MAX_NODE_TYPES


def _checked_node_types(node_type, num_node_type, num_node):
    """node_type as the uint8 array the dataset stores, or an AssertionError that names what is wrong with it."""
    assert num_node_type is not None and 1 <= int(num_node_type) <= MAX_NODE_TYPES, \
        f"num_node_type: 1 .. {MAX_NODE_TYPES} (GGMS_MAX_NODE_TYPES), not {num_node_type}"
    a = np.asarray(node_type)
    assert a.shape == (num_node,), f"node_type: one type per node ({num_node}), not {a.shape}"
    over = np.flatnonzero((a < 0) | (a >= int(num_node_type)))
    assert over.size == 0, (f"node_type: node {int(over[0]) if over.size else 0} has type "
                            f"{int(a[over[0]]) if over.size else 0}, not below num_node_type = {num_node_type}")
    return np.ascontiguousarray(a, dtype=np.uint8)


def _checked_node_feat(node_feat, node_type, num_node_type):
    """node_feat as [(the (rows, dim) array a file stores -- bfloat16 as its uint16 bits -- or None, dtype name)], one
    per node type, or an AssertionError that names the type and what is wrong with its entry."""
    assert node_type is not None, "node_feat: needs node_type / num_node_type (one table per node type)"
    T = int(num_node_type)
    assert len(node_feat) == T, f"node_feat: one entry per node type ({T}), not {len(node_feat)}"
    counts = np.bincount(node_type, minlength=T)
    out = []
    for t, a in enumerate(node_feat):
        if a is None:
            out.append((None, "F32"))
            continue
        if hasattr(a, "detach"):  # a torch tensor
            import torch
            names = {torch.float32: "F32", torch.float16: "F16", torch.bfloat16: "BF16"}
            assert a.dtype in names, f"node_feat[{t}]: dtype {a.dtype} (F32, F16 or BF16)"
            name = names[a.dtype]
            a = a.detach().cpu().contiguous()
            a = a.view(torch.int16).numpy().view(np.uint16) if name == "BF16" else a.numpy()
        else:
            a = np.asarray(a)
            names = {np.dtype(np.float32): "F32", np.dtype(np.float16): "F16"}
            assert a.dtype in names, f"node_feat[{t}]: dtype {a.dtype} (F32, F16 or BF16)"
            name = names[a.dtype]
        assert a.ndim == 2, f"node_feat[{t}]: a 2-d (rows, dim) array, not rank {a.ndim}"
        assert a.shape[0] == counts[t], f"node_feat[{t}]: one row per node of type {t} ({int(counts[t])}), not {a.shape[0]}"
        assert a.shape[1] >= 1, f"node_feat[{t}]: rows of dim 0 (None is a type without features)"
        out.append((np.ascontiguousarray(a), name))
    return out


def relation_types(indptr, indices, node_type, num_node_type):
    """Relations that are consistent with the node types by construction: for a list entry p of owner v (the edge's
    destination; indices[p] is its source) etype[p] = type(v) * T + type(indices[p]), T = num_node_type, so relation r
    joins source type r % T to destination type r // T and there are T * T of them (T * T <= 32: the sampler's bound on
    NUM_EDGE_TYPE).  The result is in the order of `indices`; sort_lists_by_type makes the CSR khop_typed wants of it."""
    T = int(num_node_type) if num_node_type is not None else 0
    ip = np.asarray(indptr, dtype=np.int64)
    nt = _checked_node_types(node_type, num_node_type, ip.size - 1)
    assert T * T <= 32, f"relation_types: {T} node types give {T * T} relations, above 32 (GGMS_MAX_EDGE_TYPES)"
    owner = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return (nt[owner].astype(np.uint32) * T + nt[np.asarray(indices, dtype=np.int64)]).astype(np.uint8)


def first_unsorted_list(indptr, edge_time):
    """The first node whose list's values (times, types) are not non-decreasing -- the precondition of khop_temporal and
    khop_typed -- or None."""
    ip = np.asarray(indptr, dtype=np.int64)
    t = np.asarray(edge_time, dtype=np.int64)
    if t.size < 2:
        return None
    drop = np.flatnonzero(t[1:] < t[:-1]) + 1  # positions whose time is below their predecessor's
    starts = np.zeros(t.size + 1, bool)
    starts[ip[:-1]] = True  # a list's first position has no predecessor in its list
    drop = drop[~starts[drop]]
    return None if drop.size == 0 else int(np.searchsorted(ip, drop[0], side="right") - 1)


def sort_lists_by_time(indptr, indices, edge_time, *edge_arrays):
    """A time-sorted CSR for khop_temporal: every node's list stably re-sorted by time (equal times keep their order).
    Returns (indices, edge_time, *edge_arrays, perm), all permuted alike -- new[p] = old[perm[p]]; every other per-edge
    array (edge_feat rows, weights) must be permuted with `perm` too, and positions kept elsewhere (train_edges) are
    re-mapped by the caller: new position = inverse[old position], inverse[perm] = arange.
    Times are uint32.  Float or 64-bit times are rank-transformed first (np.unique(t, return_inverse=True)[1]): only
    their order matters to the sampler."""
    return _sort_lists_by(indptr, indices, np.ascontiguousarray(edge_time, dtype=np.uint32), "edge_time", edge_arrays)


def sort_lists_by_type(indptr, indices, edge_type, *edge_arrays):
    """A type-sorted CSR for khop_typed: every node's list stably re-sorted by edge type (a relation's edges keep their
    order), so the edges of one type of a node are one contiguous segment.  Returns (indices, edge_type, *edge_arrays,
    perm), sort_lists_by_time's convention: new[p] = old[perm[p]]."""
    return _sort_lists_by(indptr, indices, np.ascontiguousarray(edge_type, dtype=np.uint8), "edge_type", edge_arrays)


def _sort_lists_by(indptr, indices, key, what, edge_arrays):
    """Every list stably re-sorted by a per-edge key: (indices, key, *edge_arrays, perm), all permuted alike."""
    ip = np.asarray(indptr, dtype=np.int64)
    assert key.shape == (int(ip[-1]),), f"{what}: one value per edge"
    owner = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    perm = np.lexsort((np.arange(key.size), key, owner))  # by list, then key, then old position
    return (np.asarray(indices)[perm], key[perm], *[np.asarray(a)[perm] for a in edge_arrays], perm)


# FEAT_DATA_TYPE names of the OCP 8-bit float tables (include/ggms.h: GGMS_F8E4M3 = 16, GGMS_F8E5M2 = 17)
FP8_FORMATS = ("F8E4M3", "F8E5M2")
E4M3_MAX = 448.0  # the largest finite E4M3 value; the format has no infinity


def _fp8_torch_dtype(fmt):
    import torch
    return {"F8E4M3": torch.float8_e4m3fn, "F8E5M2": torch.float8_e5m2}[fmt]


def _fp8_bytes(feat, fmt):
    """The bytes of an FP8 table: a torch tensor of the format's dtype, or a uint8 array that already holds them."""
    import torch
    if isinstance(feat, torch.Tensor):
        assert feat.dtype == _fp8_torch_dtype(fmt), (feat.dtype, fmt)
        return feat.contiguous().view(torch.uint8).numpy()
    feat = np.asarray(feat)
    assert feat.dtype == np.uint8, f"an {fmt} table is passed as its torch dtype or as uint8 bytes, not {feat.dtype}"
    return feat


# ---- Q8ROW: row-scaled 8-bit tables (include/ggms.h: GGMS_Q8ROW = 18) ------------------------------------------------
# A row of `dim` elements is `dim` uint8 codes, zero bytes up to the next multiple of 8, then the row's little-endian
# float32 scale and float32 bias; element value = float32(float32(code * scale) + bias), two roundings.
def q8row_stride(dim):
    """Bytes from one Q8ROW row of `dim` elements to the next (ggms_row_bytes)."""
    return (dim + 7) // 8 * 8 + 8


def pack_q8row(codes, scale, bias):
    """(n, dim) uint8 codes + (n,) float32 scale and bias -> the (n, q8row_stride(dim)) uint8 rows of a Q8ROW table."""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint8 and codes.ndim == 2, (codes.dtype, codes.shape)
    n, dim = codes.shape
    pad = q8row_stride(dim) - 8
    rows = np.zeros((n, pad + 8), np.uint8)
    rows[:, :dim] = codes
    rows[:, pad:pad + 4] = np.ascontiguousarray(scale, dtype="<f4").reshape(n, 1).view(np.uint8)
    rows[:, pad + 4:] = np.ascontiguousarray(bias, dtype="<f4").reshape(n, 1).view(np.uint8)
    return rows


def unpack_q8row(rows, dim):
    """The inverse of pack_q8row: (codes, scale, bias) of packed rows (copies; the pad bytes are not looked at)."""
    rows = np.asarray(rows)
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.shape[1] == q8row_stride(dim), (rows.dtype, rows.shape, dim)
    pad = q8row_stride(dim) - 8
    scale = np.ascontiguousarray(rows[:, pad:pad + 4]).view("<f4").ravel().astype(np.float32)
    bias = np.ascontiguousarray(rows[:, pad + 4:]).view("<f4").ravel().astype(np.float32)
    return np.ascontiguousarray(rows[:, :dim]), scale, bias


def quantize_q8row(values, first_row=0):
    """(n, dim) finite F32 / F16 values -> (codes, scale, bias), per row and computed in float64: bias = min,
    scale = float32((max - min) / 255), code = clip(rint((x - bias) / scale), 0, 255); a constant row (and one whose
    range is so small that the scale rounds to 0) gets scale 0 and codes 0, and decodes to its minimum.  A row holding
    NaN or +-inf is an error that names the row (first_row + its index)."""
    v = np.asarray(values).astype(np.float64)
    bad = ~np.isfinite(v).all(axis=1)
    if bad.any():
        raise ValueError(f"quantize_features: row {first_row + int(np.flatnonzero(bad)[0])} holds NaN or inf: a "
                         "row-scaled table has no code for either")
    lo, hi = v.min(axis=1), v.max(axis=1)
    scale = ((hi - lo) / 255.0).astype(np.float32)
    s64 = scale.astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint((v - lo[:, None]) / s64)
    codes = np.where(s64 > 0, np.clip(q, 0, 255), 0).astype(np.uint8)
    return codes, scale, lo.astype(np.float32)  # (the minimum of F32 / F16 values is an f32 number)


def quantize_features(path_in, path_out, fmt, chunk_rows=1 << 20, device=None):
    """Rewrite the F32 / F16 dataset at path_in as the same dataset with an 8-bit feature table at path_out: fmt
    "Q8ROW" quantises every row to 8-bit codes with the row's own scale and bias (quantize_q8row); for an FP8 feature
    table (fmt "F8E4M3" or "F8E5M2"): every other file is linked (or copied where a link is not possible), feat.bin is cast on the
    CPU with torch, round to nearest even, one chunk of rows at a time, and meta.txt names the new FEAT_DATA_TYPE.
    device=None: on the CPU, numpy / torch in float64, as described here.  device="cuda:0" (a torch device string): every
    chunk is uploaded, encoded by the GPU (ops.quantize_rows, ggms_quantize_rows) and written out -- the same files byte
    for byte; with a device fmt may also be "F16" (from an F32 table) or "BF16".

    E4M3 has no infinity and torch's cast turns everything beyond its range into NaN, so for E4M3 the values are
    clamped to +-448 (the largest finite value) FIRST: an out-of-range input saturates; NaN stays NaN.  E5M2 is cast
    as it is: overflow becomes +-inf, as in every IEEE-like format.  Unscaled: values are stored as they are."""
    import os
    import shutil
    import torch
    assert fmt in FP8_FORMATS or fmt == "Q8ROW" or (device is not None and fmt in ("F16", "BF16")), fmt
    with open(os.path.join(path_in, "meta.txt")) as f:
        meta = [line.split() for line in f if line.strip()]
    kv = dict(meta)
    src_name = kv.get("FEAT_DATA_TYPE", "F32")
    assert src_name in ("F32", "F16"), f"quantize_features reads F32 and F16 tables, not {src_name}"
    assert src_name != fmt, f"the table is {fmt} already"
    src_dt = np.float32 if src_name == "F32" else np.float16
    n, dim = int(kv["NUM_NODE"]), int(kv["FEAT_DIM"])
    os.makedirs(path_out, exist_ok=True)
    for name in os.listdir(path_in):
        if name in ("feat.bin", "meta.txt"):
            continue
        src, dst = os.path.join(path_in, name), os.path.join(path_out, name)
        if os.path.exists(dst):
            os.remove(dst)
        try:
            os.link(src, dst)
        except OSError:
            shutil.copyfile(src, dst)
    table = np.memmap(os.path.join(path_in, "feat.bin"), dtype=src_dt, mode="r", shape=(n, dim))
    with open(os.path.join(path_out, "feat.bin"), "wb") as out:
        for r in range(0, n, chunk_rows):
            if device is not None:
                from . import ops
                out_dtype = ops.Q8ROW if fmt == "Q8ROW" else \
                    {"F16": torch.float16, "BF16": torch.bfloat16}.get(fmt) or _fp8_torch_dtype(fmt)
                rows = ops.quantize_rows(torch.from_numpy(np.array(table[r:r + chunk_rows])).to(device), out_dtype, first_row=r)
                out.write(rows.view(torch.uint8).cpu().numpy().tobytes())
                continue
            if fmt == "Q8ROW":
                out.write(pack_q8row(*quantize_q8row(table[r:r + chunk_rows], first_row=r)).tobytes())
                continue
            v = torch.from_numpy(np.array(table[r:r + chunk_rows])).float()
            if fmt == "F8E4M3":
                v = v.clamp(-E4M3_MAX, E4M3_MAX)
            out.write(v.to(_fp8_torch_dtype(fmt)).view(torch.uint8).numpy().tobytes())
    with open(os.path.join(path_out, "meta.txt"), "w") as f:
        for k, v in meta:
            if k != "FEAT_DATA_TYPE":
                f.write(f"{k}\t{v}\n")
        f.write(f"FEAT_DATA_TYPE\t{fmt}\n")
    return path_out
