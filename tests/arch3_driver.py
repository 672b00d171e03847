"""Runs the samgraph_* engine as arch3 (sampler GPU + trainer GPU) like a reference example script would, and dumps
every batch to .npz in the format of tests/engine_driver.py.

    python tests/arch3_driver.py <dataset_dir> <out_prefix> <step|start> [extra k=v ...]

step:  sample_once() + get_next_batch() per step (engine_driver.run_worker: the same file, byte for byte, as an arch1
       run of tests/engine_driver.py with the same keys).
start: one start() -- the engine's own background loop, as train_gcn.py:178-182 runs it with `pipeline` on -- then
       get_next_batch() per step.  Also writes <out_prefix>.info.json: the device of every returned tensor and the
       hand-off's profiler items per batch.

sampler_ctx / trainer_ctx default to cuda:0 / cuda:1; on a one-GPU box run it with SAMGRAPH_FORCE_DEVICE=0.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config, record_batch, run_worker  # noqa: E402


def run_started(sam, num_layers, out_prefix):
    import torch
    batches, info = {}, {"devices": [], "steps": []}
    sam.start()
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        key = sam.get_next_batch()
        rec, devices = record_batch(sam, key, num_layers)
        for k, v in rec.items():
            batches[f"{key}:{k}"] = v
        info["devices"].append(sorted(devices))
        info["steps"].append({"key": int(key), "graph_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1GraphBytes),
                              "id_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1IdBytes),
                              "graph_copy_s": sam.get_log_step_value_by_key(key, sam.kLogL2GraphCopyTime),
                              "copy_s": sam.get_log_step_value_by_key(key, sam.kLogL1CopyTime),
                              "feature_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1FeatureBytes),
                              "num_input": int(rec["input_nodes"].size), "num_seeds": int(rec["output_nodes"].size)})
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w0.npz", **batches)
    with open(f"{out_prefix}.info.json", "w") as f:
        json.dump(info, f)
    sam.shutdown()


def main():
    dataset, out_prefix, mode = sys.argv[1:4]
    assert mode in ("step", "start"), mode
    extra = dict(a.split("=", 1) for a in sys.argv[4:])
    import samgraph.torch as sam
    # the keys and defaults of tests/engine_driver.py: an arch1 run there with the same extra keys is the comparison
    cfg = base_config(sam, dataset, "arch3", {"sampler_ctx": "cuda:0", "trainer_ctx": "cuda:1", **extra})
    sam.config(cfg)
    sam.init()
    if mode == "step":
        run_worker(sam, 0, cfg["num_layer"], out_prefix, False)
    else:
        run_started(sam, cfg["num_layer"], out_prefix)


if __name__ == "__main__":
    main()
