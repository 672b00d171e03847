"""tests/engine_driver.py's loop for runs with the config key `feat_out_dtype`: every batch goes to .npz with its feature
rows as raw 16- / 32-bit integers (numpy has no bfloat16) next to the name of their torch dtype.

    python tests/feat_convert_driver.py <dataset_dir> <out_prefix> <arch1|arch3|arch6> [num_worker] [extra k=v ...]

arch3 places its two contexts as tests/arch3_driver.py does (cuda:0 samples, cuda:1 trains; SAMGRAPH_FORCE_DEVICE=0 on a
one-GPU box) and steps with sample_once() + get_next_batch(), so an arch1 run with the same keys is the comparison.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config  # noqa: E402


def record_batch(sam, key, num_layers):
    import torch
    feat = sam.get_graph_feat(key)
    rec = {"feat_bits": feat.view({2: torch.int16, 4: torch.int32}[feat.element_size()]).cpu().numpy(),
           "feat_dtype": str(feat.dtype), "label": sam.get_graph_label(key).cpu().numpy(),
           "input_nodes": sam.get_graph_input_nodes(key).cpu().numpy(),
           "output_nodes": sam.get_graph_output_nodes(key).cpu().numpy()}
    for i, (row, col, ns, nd) in enumerate(sam.get_graph_coo(key, num_layers)):
        rec[f"row{i}"], rec[f"col{i}"] = row.cpu().numpy(), col.cpu().numpy()
        rec[f"num_src{i}"], rec[f"num_dst{i}"] = ns, nd
    rec["miss_bytes"] = sam.get_log_step_value_by_key(key, sam.kLogL1MissBytes)
    rec["feature_bytes"] = sam.get_log_step_value_by_key(key, sam.kLogL1FeatureBytes)
    return rec


def run_worker(sam, worker_id, num_layers, out_prefix):
    import torch
    batches = {}
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        sam.sample_once()
        key = sam.get_next_batch()
        for k, v in record_batch(sam, key, num_layers).items():
            batches[f"{key}:{k}"] = v
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w{worker_id}.npz", **batches)
    sam.shutdown()


def main():
    dataset, out_prefix, arch = sys.argv[1:4]
    num_worker = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    extra = dict(a.split("=", 1) for a in sys.argv[5:])
    import samgraph.torch as sam
    if arch in ("arch1", "arch3"):
        ctx = {"sampler_ctx": "cuda:0", "trainer_ctx": "cuda:0" if arch == "arch1" else "cuda:1"}
        cfg = base_config(sam, dataset, arch, {**ctx, **extra})
        sam.config(cfg)
        sam.init()
        run_worker(sam, 0, cfg["num_layer"], out_prefix)
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
                run_worker(sam, w, cfg["num_layer"], out_prefix)
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
