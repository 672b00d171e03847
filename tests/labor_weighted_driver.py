"""tests/edge_driver.py's run with what a khop_labor_weighted batch adds: every layer's edge weights.

    python tests/labor_weighted_driver.py <dataset_dir> <out_prefix> [extra k=v ...]
"""
import edge_driver
import link_driver

edge_driver.IDS = True  # implied: the sampler emits the positions


def record_batch(sam, key, num_layers, link):
    rec = edge_driver.record_batch(sam, key, num_layers, link)
    for i in range(num_layers):
        w = sam.get_graph_edge_weight(key, i)
        assert w.numel() == sam.get_graph_num_edge(key, i) and w.device == sam.get_graph_row(key, i).device
        assert str(w.dtype) == "torch.float32"
        rec[f"eweight{i}"] = w.cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.record_batch = record_batch
    link_driver.main()
