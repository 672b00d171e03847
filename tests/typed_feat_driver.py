"""tests/hetero_driver.py's run for a dataset with one feature table per node type.  Without typed_feat = on it IS that run.
With the key there is no single feature matrix: the record holds, per type, the block get_graph_feat_of_type hands out --
its raw bits, dtype and shape -- after checking that every block is a view of ONE buffer at the offset the definition gives
(off[t + 1] = round_up(off[t] + cnt_t x dim_t x element size, 16)), plus what the engine says about the types' tables.

    python tests/typed_feat_driver.py <dataset_dir> <out_prefix> [probe=<accessor>] [extra k=v ...]

probe=<accessor>: called on the first batch whatever the configuration says (a type of 0 where it takes one); the run must
die there, by name.
"""
import sys

PROBE = [a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("probe=")]
sys.argv = [a for a in sys.argv if not a.startswith("probe=")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hetero_driver  # noqa: E402
import link_driver  # noqa: E402
import typed_driver  # noqa: E402

ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
TYPED_FEAT = ARGS.get("typed_feat") == "on"
PROBE_ARGS = dict(get_graph_feat=("key",), get_graph_feat_of_type=("key", 0), feat_dim_of_type=(0,), feat_dtype_of_type=(0,))
INT_VIEW = {2: torch.int16, 4: torch.int32}


def record_batch(sam, key, num_layers, link):
    for name in PROBE:
        getattr(sam, name)(*[key if a == "key" else a for a in PROBE_ARGS[name]])
    if not TYPED_FEAT:
        return hetero_driver.record_batch(sam, key, num_layers, link)
    # link_driver.py records get_graph_feat, which dies by name under the key (probed by the tests): not called here
    real = sam.get_graph_feat
    sam.get_graph_feat = lambda k: torch.empty((0, 0))
    try:
        rec = typed_driver.record_batch(sam, key, num_layers, link)
    finally:
        sam.get_graph_feat = real
    del rec["feat"]
    T = sam.num_node_type()
    R = len(typed_driver.ARGS["type_fanout"].split("/")[0].split(","))
    ntype, local, slot = sam.get_graph_node_type(key), sam.get_graph_node_local(key), sam.get_graph_node_slot(key)
    rec.update(ntype=ntype.cpu().numpy(), local=local.cpu().numpy(), slot=slot.cpu().numpy(), num_node_type=T,
               rel_src=[sam.relation_src_type(r) for r in range(R)], rel_dst=[sam.relation_dst_type(r) for r in range(R)])
    off, base = 0, None
    for t in range(T):
        nodes, rows = sam.get_graph_typed_nodes(key, t), sam.get_graph_feat_of_type(key, t)
        dim, dt = sam.feat_dim_of_type(t), sam.feat_dtype_of_type(t)
        assert tuple(rows.shape) == (nodes.numel(), dim) and (dim == 0 or rows.dtype == dt), (rows.shape, rows.dtype, dim, dt)
        assert rows.device == nodes.device
        if rows.numel():  # a view of the batch's buffer at the type's offset word, not a copy
            base = rows.data_ptr() - off if base is None else base
            assert rows.data_ptr() == base + off and rows.data_ptr() % 16 == 0, (t, rows.data_ptr(), base, off)
            assert rows.is_contiguous()
        es = rows.element_size()
        off = (off + rows.numel() * es + 15) // 16 * 16
        bits = rows.contiguous().view(INT_VIEW[es]).cpu().numpy() if rows.numel() else np.zeros(tuple(rows.shape), np.int32)
        rec[f"typed{t}"], rec[f"feat{t}"] = nodes.cpu().numpy(), bits
        rec[f"feat_dtype{t}"], rec[f"feat_dim{t}"] = (str(rows.dtype) if dim else "none"), dim
        rec[f"src_of{t}"] = [sam.get_graph_num_src_of_type(key, i, t) for i in range(num_layers)]
        rec[f"dst_of{t}"] = [sam.get_graph_num_dst_of_type(key, i, t) for i in range(num_layers)]
    for i in range(num_layers):
        for r in range(R):
            row, col, eid = sam.get_graph_rel_row(key, i, r), sam.get_graph_rel_col(key, i, r), sam.get_graph_rel_edge_ids(key, i, r)
            assert row.numel() == col.numel() == eid.numel() == sam.get_graph_rel_num_edges(key, i, r)
            rec[f"rel_row{i}_{r}"], rec[f"rel_col{i}_{r}"], rec[f"rel_eid{i}_{r}"] = (x.cpu().numpy() for x in (row, col, eid))
    rec["feature_bytes"] = sam.get_log_step_value_by_key(key, 9)  # kLogL1FeatureBytes
    return rec


if __name__ == "__main__":
    link_driver.base_config = typed_driver.base_config
    link_driver.record_batch = record_batch
    link_driver.main()
