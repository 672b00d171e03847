"""tests/typed_driver.py's run (link_driver.py's batches with edge ids and edge types), with what hetero_batch = on adds to a
batch: the node types, ranks and slots, the grouped node list and its feature slices per type, the per-type source /
destination counts, and every layer's per-relation blocks.

    python tests/hetero_driver.py <dataset_dir> <out_prefix> [probe=<accessor>] [extra k=v ...]

probe=<accessor>: the named accessor of samgraph.torch is called on the first batch (with a layer / type / relation of 0 where
it takes one) whatever the configuration says -- a run without the key must die there, by name; the argument does not
reach the configuration.
"""
import sys

PROBE = [a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("probe=")]
sys.argv = [a for a in sys.argv if not a.startswith("probe=")]

import link_driver  # noqa: E402
import typed_driver  # noqa: E402

ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
HETERO = ARGS.get("hetero_batch") == "on"
NO_KEY = ("num_node_type", "relation_src_type", "relation_dst_type")  # accessors of the run, not of a batch
NUM_ARGS = dict(get_graph_node_type=0, get_graph_node_local=0, get_graph_node_slot=0, get_graph_typed_nodes=1,
                get_graph_feat_of_type=1, get_graph_num_src_of_type=2, get_graph_num_dst_of_type=2, get_graph_rel_row=2,
                get_graph_rel_col=2, get_graph_rel_edge_ids=2, get_graph_rel_num_edges=2, num_node_type=0,
                relation_src_type=1, relation_dst_type=1)


def record_batch(sam, key, num_layers, link):
    rec = typed_driver.record_batch(sam, key, num_layers, link)
    for name in PROBE:
        args = (() if name in NO_KEY else (key,)) + (0,) * NUM_ARGS[name]
        getattr(sam, name)(*args)
    if not HETERO:
        return rec
    T = sam.num_node_type()
    R = len(typed_driver.ARGS["type_fanout"].split("/")[0].split(","))
    feat = sam.get_graph_feat(key)
    ntype, local, slot = sam.get_graph_node_type(key), sam.get_graph_node_local(key), sam.get_graph_node_slot(key)
    assert str(ntype.dtype) == "torch.uint8" and local.dtype == slot.dtype == sam.get_graph_row(key, 0).dtype
    assert ntype.numel() == local.numel() == slot.numel() == sam.get_graph_input_nodes(key).numel() == feat.shape[0]
    rec.update(ntype=ntype.cpu().numpy(), local=local.cpu().numpy(), slot=slot.cpu().numpy(), num_node_type=T,
               rel_src=[sam.relation_src_type(r) for r in range(R)], rel_dst=[sam.relation_dst_type(r) for r in range(R)])
    at = 0
    for t in range(T):
        nodes, rows = sam.get_graph_typed_nodes(key, t), sam.get_graph_feat_of_type(key, t)
        assert rows.shape == (nodes.numel(), feat.shape[1]) and rows.dtype == feat.dtype
        if nodes.numel():  # a view of the batch's feature buffer, not a copy: the type's rows are one slice of it
            assert rows.data_ptr() == feat.data_ptr() + at * feat.shape[1] * feat.element_size()
        at += nodes.numel()
        rec[f"typed{t}"], rec[f"feat{t}"] = nodes.cpu().numpy(), rows.cpu().numpy()
        rec[f"src_of{t}"] = [sam.get_graph_num_src_of_type(key, i, t) for i in range(num_layers)]
        rec[f"dst_of{t}"] = [sam.get_graph_num_dst_of_type(key, i, t) for i in range(num_layers)]
    assert at == feat.shape[0]
    for i in range(num_layers):
        for r in range(R):
            row, col, eid = sam.get_graph_rel_row(key, i, r), sam.get_graph_rel_col(key, i, r), sam.get_graph_rel_edge_ids(key, i, r)
            assert row.numel() == col.numel() == eid.numel() == sam.get_graph_rel_num_edges(key, i, r)
            rec[f"rel_row{i}_{r}"], rec[f"rel_col{i}_{r}"], rec[f"rel_eid{i}_{r}"] = (x.cpu().numpy() for x in (row, col, eid))
    return rec


if __name__ == "__main__":
    link_driver.base_config = typed_driver.base_config
    link_driver.record_batch = record_batch
    link_driver.main()
