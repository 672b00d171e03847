"""An arch1 training loop over a learnable feature table (config key feat_learnable), in the manner of
tests/link_driver.py: sample_once; get_next_batch; a "gradient"; update_graph_feat.  Every batch goes to .npz with its
sampled arrays and the rows it was delivered, and the live table (and the Adagrad state) as they stand at the end.

    python tests/learn_driver.py <dataset_dir> <out_prefix> <mode> [extra k=v ...]

mode: run (the loop; without feat_learnable among the keys nothing is updated), bad_shape (the first update gets a
gradient with one row too many), bad_shape_abi (the same through the C entry point), extract_start (calls it).
The gradient is a function of the delivered rows and the input node ids that numpy reproduces bit for bit: one f32
multiply, then one f32 add, each a torch operator of its own."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config  # noqa: E402


def gradient(rows, nodes):
    """torch (device) or numpy: fl(fl(rows * 0.5) + (nodes % 7)), float32 throughout."""
    if isinstance(rows, np.ndarray):
        bump = (nodes.astype(np.int64) % 7).astype(np.float32)[:, None]
        return ((rows * np.float32(0.5)).astype(np.float32) + bump).astype(np.float32)
    import torch
    bump = (nodes.to(torch.int64) % 7).to(torch.float32)[:, None]
    return torch.add(torch.mul(rows, 0.5), bump).contiguous()


def main():
    dataset, out_prefix, mode = sys.argv[1:4]
    extra = dict(a.split("=", 1) for a in sys.argv[4:])
    import torch
    import samgraph.torch as sam
    cfg = base_config(sam, dataset, "arch1", extra)
    cfg.update(sampler_ctx="cuda:0", trainer_ctx="cuda:0")
    learn = "feat_learnable" in cfg
    sam.config(cfg)
    sam.init()
    if mode == "extract_start":
        sam.extract_start(0)
        return
    batches = {"steps_per_epoch": sam.steps_per_epoch()}
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        sam.sample_once()
        key = sam.get_next_batch()
        rows, nodes = sam.get_graph_feat(key), sam.get_graph_input_nodes(key)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (nodes.numel(), sam.feat_dim())
        batches[f"{key}:feat"], batches[f"{key}:input_nodes"] = rows.cpu().numpy(), nodes.cpu().numpy()
        batches[f"{key}:output_nodes"] = sam.get_graph_output_nodes(key).cpu().numpy()
        for i, (row, col, _, _) in enumerate(sam.get_graph_coo(key, cfg["num_layer"])):
            batches[f"{key}:row{i}"], batches[f"{key}:col{i}"] = row.cpu().numpy(), col.cpu().numpy()
        if learn:
            grad = gradient(rows, nodes)
            if mode == "bad_shape":
                grad = torch.cat([grad, grad[:1]]).contiguous()
            if mode == "bad_shape_abi":
                from xgnn_amd.common import _basics
                _basics.C_LIB_CTYPES.samgraph_update_graph_feat(key, grad.data_ptr(), grad.shape[0] - 1, grad.shape[1],
                                                                torch.cuda.current_stream().cuda_stream)
            sam.update_graph_feat(key, grad)
        del rows, nodes  # the views hold the batch's slot
    torch.cuda.synchronize()
    if learn:
        live = sam.get_store_feat()
        assert live.is_cuda and live.dtype == torch.float32
        batches["store_feat"] = live.cpu().numpy()
        if cfg["feat_learnable"] == "adagrad":
            batches["store_state"] = sam.get_store_state().cpu().numpy()
        mapped = sam.get_dataset_feat()  # still the file
        assert not mapped.is_cuda
        batches["dataset_feat"] = mapped.numpy().copy()
    np.savez(f"{out_prefix}.w0.npz", **batches)
    sam.shutdown()


if __name__ == "__main__":
    main()
