"""tests/edge_driver.py's run (link_driver.py's batches with edge ids and edge rows), with what a khop_typed batch adds:
every layer's edge types.

    python tests/typed_driver.py <dataset_dir> <out_prefix> [extra k=v ...]

type_fanout=3,1,1/2,2,0 (rows by layer id) reaches sam.config as a list of lists, and `fanout` / `num_fanout` are left to
the front-end, which fills in the rows' sums; the fanout argument only says how many layers there are.  With another
sample_type the accessor is not called: the record is edge_driver.py's.
"""
import sys

import edge_driver
import link_driver

ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
TYPED = ARGS.get("sample_type") == "khop_typed"
if TYPED:
    edge_driver.IDS = True  # implied: the sampler emits the positions

_base_config = link_driver.base_config


def base_config(sam, dataset, arch, extra):
    cfg = _base_config(sam, dataset, arch, extra)
    if TYPED:
        cfg["type_fanout"] = [[int(k) for k in row.split(",")] for row in cfg["type_fanout"].split("/")]
        del cfg["fanout"], cfg["num_fanout"]
    return cfg


def record_batch(sam, key, num_layers, link):
    rec = edge_driver.record_batch(sam, key, num_layers, link)
    if TYPED:
        for i in range(num_layers):
            t = sam.get_graph_edge_type(key, i)
            assert t.numel() == sam.get_graph_num_edge(key, i) and t.device == sam.get_graph_row(key, i).device
            assert str(t.dtype) == "torch.uint8"
            rec[f"etype{i}"] = t.cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.base_config = base_config
    link_driver.record_batch = record_batch
    link_driver.main()
