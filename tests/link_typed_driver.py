"""tests/hetero_driver.py's run, with what negative_mode = typed_uniform | typed_exclude adds to a batch: the relation of
every positive edge.

    python tests/link_typed_driver.py <dataset_dir> <out_prefix> [extra k=v ...]
"""
import hetero_driver
import link_driver
import typed_driver


def record_batch(sam, key, num_layers, link):
    rec = hetero_driver.record_batch(sam, key, num_layers, link)
    if hetero_driver.ARGS.get("negative_mode", "").startswith("typed_"):
        rel = sam.get_graph_link_rel(key)
        assert str(rel.dtype) == "torch.uint8" and rel.numel() == sam.get_graph_link_edge_ids(key).numel()
        rec["link_rel"] = rel.cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.base_config = typed_driver.base_config
    link_driver.record_batch = record_batch
    link_driver.main()
