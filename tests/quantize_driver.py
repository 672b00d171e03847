"""The engine driver of the `feat_store_dtype` tests: tests/feat_convert_driver.py's loop with tests/fp8_driver.py's
batch record (feature rows as raw bits next to the name of their torch dtype), for the single-process deployments
arch1, arch3 and arch4 (step mode), plus what the engine says about its feature table after init: the stored bytes,
their torch dtype and shape, and feat_row_bytes().

    python tests/quantize_driver.py <dataset_dir> <out_prefix> <arch1|arch3|arch4> [extra k=v ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config  # noqa: E402
from fp8_driver import record_batch  # noqa: E402

CTX = {"arch1": ("cuda:0", "cuda:0"), "arch3": ("cuda:0", "cuda:1"), "arch4": ("cuda:1", "cuda:0")}


def main():
    dataset, out_prefix, arch = sys.argv[1:4]
    extra = dict(a.split("=", 1) for a in sys.argv[4:])
    import torch
    import samgraph.torch as sam
    cfg = base_config(sam, dataset, arch, {"sampler_ctx": CTX[arch][0], "trainer_ctx": CTX[arch][1], **extra})
    sam.config(cfg)
    sam.init()
    feat = sam.get_dataset_feat()
    batches = {"table_bytes": feat.contiguous().view(torch.uint8).numpy().copy(), "table_dtype": str(feat.dtype),
               "table_shape": np.array(feat.shape), "feat_row_bytes": sam.feat_row_bytes()}
    for _ in range(sam.num_epoch() * sam.num_local_step()):
        sam.sample_once()
        key = sam.get_next_batch()
        for k, v in record_batch(sam, key, cfg["num_layer"]).items():
            batches[f"{key}:{k}"] = v
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.w0.npz", **batches)
    sam.shutdown()


if __name__ == "__main__":
    main()
