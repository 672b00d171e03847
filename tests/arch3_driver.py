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


def run_started(sam, num_layers, out_prefix):
    import torch
    batches, info = {}, {"devices": [], "steps": []}
    sam.start()
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        key = sam.get_next_batch()
        feat, label = sam.get_graph_feat(key), sam.get_graph_label(key)
        inp, out = sam.get_graph_input_nodes(key), sam.get_graph_output_nodes(key)
        rec = {"feat": feat.cpu().numpy(), "label": label.cpu().numpy(), "input_nodes": inp.cpu().numpy(),
               "output_nodes": out.cpu().numpy()}
        devices = {str(t.device) for t in (feat, label, inp, out)}
        for i, (row, col, ns, nd) in enumerate(sam.get_graph_coo(key, num_layers)):
            data = sam.get_graph_data(key, i)
            rec[f"row{i}"], rec[f"col{i}"] = row.cpu().numpy(), col.cpu().numpy()
            rec[f"data{i}"] = data.cpu().numpy()
            rec[f"num_src{i}"], rec[f"num_dst{i}"] = ns, nd
            assert sam.get_graph_num_edge(key, i) == row.numel()
            devices |= {str(row.device), str(col.device)}
        rec["miss_bytes"] = sam.get_log_step_value_by_key(key, sam.kLogL1MissBytes)
        rec["num_sample"] = sam.get_log_step_value_by_key(key, sam.kLogL1NumSample)
        for k, v in rec.items():
            batches[f"{key}:{k}"] = v
        info["devices"].append(sorted(devices))
        info["steps"].append({"key": int(key), "graph_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1GraphBytes),
                              "id_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1IdBytes),
                              "graph_copy_s": sam.get_log_step_value_by_key(key, sam.kLogL2GraphCopyTime),
                              "copy_s": sam.get_log_step_value_by_key(key, sam.kLogL1CopyTime),
                              "feature_bytes": sam.get_log_step_value_by_key(key, sam.kLogL1FeatureBytes),
                              "num_input": int(inp.numel()), "num_seeds": int(out.numel())})
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
    from engine_driver import run_worker
    fanout = [int(x) for x in extra.pop("fanout", "5 4").split()]
    # the keys and defaults of tests/engine_driver.py: an arch1 run there with the same extra keys is the comparison
    cfg = {"dataset_path": dataset, "_arch": sam.builtin_archs["arch3"]["arch"],
           "_sample_type": sam.sample_types[extra.pop("sample_type", "khop3")],
           "batch_size": int(extra.pop("batch_size", 64)), "num_epoch": int(extra.pop("num_epoch", 2)),
           "_cache_policy": sam.cache_policies[extra.pop("cache_policy", "degree")],
           "cache_percentage": float(extra.pop("cache_percentage", 0.0)), "max_sampling_jobs": 10,
           "max_copying_jobs": 2, "omp_thread_num": int(extra.pop("omp_thread_num", 4)), "num_layer": len(fanout),
           "num_hidden": 256, "lr": 0.003, "dropout": 0.5, "num_fanout": len(fanout), "fanout": fanout,
           "seed": int(extra.pop("seed", 1234)), "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:1"}
    if cfg["_sample_type"] == sam.kRandomWalk:  # operation.cc:164-175: no fanout keys, num_neighbor per layer
        cfg.pop("num_fanout"), cfg.pop("fanout")
        cfg.update(random_walk_length=3, random_walk_restart_prob=0.5, num_random_walk=4, num_neighbor=5)
    cfg.update(extra)
    sam.config(cfg)
    sam.init()
    if mode == "step":
        run_worker(sam, 0, len(fanout), out_prefix, False)
    else:
        run_started(sam, len(fanout), out_prefix)


if __name__ == "__main__":
    main()
