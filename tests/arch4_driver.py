"""Runs the samgraph_* engine as arch4 (sampler GPU + trainer GPU, early prefetch, optional dynamic_cache) like a
reference example script would, and dumps every batch to .npz in the format of tests/engine_driver.py.

    python tests/arch4_driver.py <dataset_dir> <out_prefix> <step|start> [extra k=v ...]

Modes as tests/arch3_driver.py.  Also writes <out_prefix>.info.json: the arch4 profiler items of every batch.
sampler_ctx / trainer_ctx default to cuda:1 / cuda:0; on a one-GPU box run it with SAMGRAPH_FORCE_DEVICE=0.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config, record_batch  # noqa: E402


def main():
    dataset, out_prefix, mode = sys.argv[1:4]
    assert mode in ("step", "start"), mode
    extra = dict(a.split("=", 1) for a in sys.argv[4:])
    extra.setdefault("sample_type", "khop0")
    import torch
    import samgraph.torch as sam
    cfg = base_config(sam, dataset, "arch4", {"sampler_ctx": "cuda:1", "trainer_ctx": "cuda:0", **extra})
    sam.config(cfg)
    sam.init()
    L = cfg["num_layer"]
    batches, info = {}, {"steps": [], "devices": []}
    if mode == "start":
        sam.start()
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        if mode == "step":
            sam.sample_once()
        key = sam.get_next_batch()
        rec, devices = record_batch(sam, key, L)
        for k, v in rec.items():
            batches[f"{key}:{k}"] = v
        info["devices"].append(sorted(devices))
        item = lambda name: sam.get_log_step_value_by_key(key, getattr(sam, name))  # noqa: E731
        info["steps"].append({"key": int(key), "miss_bytes": item("kLogL1MissBytes"),
                              "feature_bytes": item("kLogL1FeatureBytes"), "copy_s": item("kLogL1CopyTime"),
                              "neighbour_s": item("kLogL1GetNeighbourTime"), "advanced_s": item("kLogL1PrefetchAdvanced"),
                              "cache_copy_s": item("kLogL2CacheCopyTime")})
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w0.npz", **batches)
    with open(f"{out_prefix}.info.json", "w") as f:
        json.dump(info, f)
    sam.shutdown()


if __name__ == "__main__":
    main()
