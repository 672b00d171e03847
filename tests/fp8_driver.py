"""The engine drivers for runs on an FP8 feature table: tests/feat_convert_driver.py (arch1 / arch3 / arch6) and
tests/arch5_driver.py with a batch record whose feature rows are raw 8- / 16- / 32-bit integers (numpy has neither FP8
nor bfloat16) next to the name of their torch dtype.

    python tests/fp8_driver.py engine <dataset_dir> <out_prefix> <arch1|arch3|arch6> [num_worker] [extra k=v ...]
    python tests/fp8_driver.py arch5 <dataset_dir> <out_prefix> <S> <T> <step|start> [extra k=v ...]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arch5_driver  # noqa: E402
import feat_convert_driver  # noqa: E402


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


if __name__ == "__main__":
    kind = sys.argv.pop(1)
    if kind == "arch5":
        arch5_driver.record_batch = lambda sam, key, num_layers: (record_batch(sam, key, num_layers), set())
        arch5_driver.main()
    else:
        assert kind == "engine", kind
        feat_convert_driver.record_batch = record_batch
        feat_convert_driver.main()
