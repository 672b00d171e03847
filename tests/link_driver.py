"""tests/engine_driver.py's loop for an arch1 run that may be a link_prediction run: every batch goes to .npz with the
sampled arrays, its feature rows and -- with task = link_prediction -- the pair ids.

    python tests/link_driver.py <dataset_dir> <out_prefix> [extra k=v ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config  # noqa: E402


def record_batch(sam, key, num_layers, link):
    rec = {"feat": sam.get_graph_feat(key).cpu().numpy(), "label": sam.get_graph_label(key).cpu().numpy(),
           "input_nodes": sam.get_graph_input_nodes(key).cpu().numpy(),
           "output_nodes": sam.get_graph_output_nodes(key).cpu().numpy()}
    for i, (row, col, ns, nd) in enumerate(sam.get_graph_coo(key, num_layers)):
        rec[f"row{i}"], rec[f"col{i}"] = row.cpu().numpy(), col.cpu().numpy()
        rec[f"num_src{i}"], rec[f"num_dst{i}"] = ns, nd
    if link:
        ids = sam.get_graph_seed_ids(key)
        pos_src, pos_dst, neg_src, neg_dst = sam.get_graph_link_pairs(key)
        k = sam.num_negative()
        b = ids.numel() // (2 + k)
        # views of the one id tensor, neg_src the positives' sources expanded
        assert pos_src.data_ptr() == ids.data_ptr() and pos_dst.data_ptr() == ids.data_ptr() + 4 * b
        assert neg_dst.data_ptr() == ids.data_ptr() + 8 * b and neg_src.data_ptr() == ids.data_ptr()
        assert tuple(neg_src.shape) == tuple(neg_dst.shape) == (b, k) and neg_src.stride() == (1, 0)
        rec.update(seed_ids=ids.cpu().numpy(), pos_src=pos_src.cpu().numpy(), pos_dst=pos_dst.cpu().numpy(),
                   neg_src=neg_src.cpu().numpy(), neg_dst=neg_dst.cpu().numpy(), num_negative=k)
    return rec


def main():
    dataset, out_prefix = sys.argv[1:3]
    extra = dict(a.split("=", 1) for a in sys.argv[3:])
    import torch
    import samgraph.torch as sam
    cfg = base_config(sam, dataset, "arch1", extra)
    cfg.update(sampler_ctx="cuda:0", trainer_ctx="cuda:0")
    link = cfg.get("task") == "link_prediction"
    sam.config(cfg)
    sam.init()
    batches = {"steps_per_epoch": sam.steps_per_epoch(), "num_negative": sam.num_negative()}
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        sam.sample_once()
        key = sam.get_next_batch()
        for k, v in record_batch(sam, key, cfg["num_layer"], link).items():
            batches[f"{key}:{k}"] = v
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w0.npz", **batches)
    sam.shutdown()


if __name__ == "__main__":
    main()
