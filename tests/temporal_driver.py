"""tests/edge_driver.py's run (link_driver.py's batches with edge ids and edge rows), with what a khop_temporal batch adds:
every layer's edge times, the input nodes' cut-offs and the positives' times.

    python tests/temporal_driver.py <dataset_dir> <out_prefix> [extra k=v ...]

With another sample_type the three accessors are not called: the record is edge_driver.py's.
"""
import sys

import edge_driver
import link_driver

ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
TEMPORAL = ARGS.get("sample_type") == "khop_temporal"
if TEMPORAL:
    edge_driver.IDS = True  # implied: the sampler emits the positions


def record_batch(sam, key, num_layers, link):
    rec = edge_driver.record_batch(sam, key, num_layers, link)
    if TEMPORAL:
        for i in range(num_layers):
            t = sam.get_graph_edge_time(key, i)
            assert t.numel() == sam.get_graph_num_edge(key, i) and t.device == sam.get_graph_row(key, i).device
            rec[f"etime{i}"] = t.cpu().numpy()
        cut = sam.get_graph_node_cut(key)
        assert cut.numel() == sam.get_graph_input_nodes(key).numel()
        rec["node_cut"] = cut.cpu().numpy()
        rec["link_time"] = sam.get_graph_link_time(key).cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.record_batch = record_batch
    link_driver.main()
