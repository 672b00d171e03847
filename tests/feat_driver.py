"""tests/engine_driver.py's loop for runs on a feature table of any format (config keys `feat_out_dtype`,
`feat_store_dtype`): every batch goes to .npz with its feature rows as raw 8- / 16- / 32-bit integers (numpy has neither
FP8 nor bfloat16) next to the name of their torch dtype.

    python tests/feat_driver.py <dataset_dir> <out_prefix> <arch1|arch3|arch4|arch5|arch6> <num_worker> [table] [extra k=v ...]

arch1, arch3 and arch4 are one process with two contexts (arch3: cuda:0 samples, cuda:1 trains; arch4: the reverse;
SAMGRAPH_FORCE_DEVICE=0 on a one-GPU box) that steps with sample_once() + get_next_batch(), so an arch1 run with the same
keys is the comparison; arch6 forks num_worker workers; arch5 is tests/arch5_driver.py (1 sampler, 1 trainer, step mode)
with this batch record.  `table` also records what the engine says about its feature table after init: the stored
bytes, their torch dtype and shape, and feat_row_bytes().
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arch5_driver  # noqa: E402
from engine_driver import base_config  # noqa: E402

CTX = {"arch1": ("cuda:0", "cuda:0"), "arch3": ("cuda:0", "cuda:1"), "arch4": ("cuda:1", "cuda:0")}


def record_batch(sam, key, num_layers):
    import torch
    feat = sam.get_graph_feat(key)
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[feat.element_size()]
    rec = {"feat_bits": feat.view(bits).cpu().numpy(), "feat_dtype": str(feat.dtype),
           "label": sam.get_graph_label(key).cpu().numpy(), "input_nodes": sam.get_graph_input_nodes(key).cpu().numpy(),
           "output_nodes": sam.get_graph_output_nodes(key).cpu().numpy()}
    for i, (row, col, ns, nd) in enumerate(sam.get_graph_coo(key, num_layers)):
        rec[f"row{i}"], rec[f"col{i}"] = row.cpu().numpy(), col.cpu().numpy()
        rec[f"num_src{i}"], rec[f"num_dst{i}"] = ns, nd
    rec["miss_bytes"] = sam.get_log_step_value_by_key(key, sam.kLogL1MissBytes)
    rec["feature_bytes"] = sam.get_log_step_value_by_key(key, sam.kLogL1FeatureBytes)
    return rec


def run_worker(sam, worker_id, num_layers, out_prefix, table):
    import torch
    batches = {}
    if table:
        feat = sam.get_dataset_feat()
        batches = {"table_bytes": feat.contiguous().view(torch.uint8).numpy().copy(), "table_dtype": str(feat.dtype),
                   "table_shape": np.array(feat.shape), "feat_row_bytes": sam.feat_row_bytes()}
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        sam.sample_once()
        key = sam.get_next_batch()
        for k, v in record_batch(sam, key, num_layers).items():
            batches[f"{key}:{k}"] = v
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w{worker_id}.npz", **batches)
    sam.shutdown()


def main():
    dataset, out_prefix, arch, num_worker = sys.argv[1:4] + [int(sys.argv[4])]
    table = sys.argv[5:6] == ["table"]
    rest = sys.argv[6 if table else 5:]
    if arch == "arch5":
        sys.argv[1:] = [dataset, out_prefix, "1", "1", "step"] + rest
        return arch5_driver.main(lambda sam, key, num_layers: (record_batch(sam, key, num_layers), set()))
    extra = dict(a.split("=", 1) for a in rest)
    import samgraph.torch as sam
    if arch in CTX:
        cfg = base_config(sam, dataset, arch, {"sampler_ctx": CTX[arch][0], "trainer_ctx": CTX[arch][1], **extra})
        sam.config(cfg)
        sam.init()
        run_worker(sam, 0, cfg["num_layer"], out_prefix, table)
        return
    assert arch == "arch6", arch
    cfg = base_config(sam, dataset, arch, extra)
    cfg["num_worker"] = num_worker
    sam.config(cfg)
    sam.data_init()  # host only: the GPU is first touched in the children
    pids = []
    for w in range(num_worker):
        pid = os.fork()
        if pid == 0:
            try:
                sam.sample_init(w, f"cuda:{w}")
                sam.train_init(w, f"cuda:{w}")
                run_worker(sam, w, cfg["num_layer"], out_prefix, table)
                os._exit(0)
            except BaseException as e:  # noqa: BLE001
                print("worker failed:", repr(e), file=sys.stderr)
                os._exit(1)
        pids.append(pid)
    bad = 0
    for _ in pids:
        bad += sam.wait_one_child()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
