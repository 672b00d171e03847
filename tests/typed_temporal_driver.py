"""tests/hetero_driver.py's run (typed_driver.py's batches, with the typed view under hetero_batch = on) for sample_type
khop_typed_temporal, with what temporal_driver.py adds: edge times, node cuts, link times.

    python tests/typed_temporal_driver.py <dataset_dir> <out_prefix> sample_type=khop_typed_temporal [extra k=v ...]
"""
import edge_driver
import link_driver
import typed_driver

typed_driver.TYPED = edge_driver.IDS = True  # the drivers below gate on khop_typed's name; this sampler shares its keys
import hetero_driver  # noqa: E402


def record_batch(sam, key, num_layers, link):
    rec = hetero_driver.record_batch(sam, key, num_layers, link)
    for i in range(num_layers):
        rec[f"etime{i}"] = sam.get_graph_edge_time(key, i).cpu().numpy()
    rec["node_cut"] = sam.get_graph_node_cut(key).cpu().numpy()
    rec["link_time"] = sam.get_graph_link_time(key).cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.base_config = typed_driver.base_config
    link_driver.record_batch = record_batch
    link_driver.main()
