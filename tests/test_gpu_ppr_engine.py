"""sample_type ppr_topk through the engine (arch1, 2 layers, induced_subgraph = on behind it: ShaDow with a PPR
extractor): every batch of an epoch is the numpy statement (tests/ppr_ref.py) replayed from the batch's own output
nodes -- input nodes, row, col and the scores."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ppr_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features, powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "engine_driver.py")
NODES, BATCH, ALPHA, EPS, C, ROUNDS, K = 3000, 64, 0.25, 1e-3, 128, 16, 4


def test_every_batch_equals_the_reference(tmp_path):
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(NODES, mean_deg=12, seed=9)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 10, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    path = str(tmp_path / "ds")
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13)
    args = ["seed=21", f"batch_size={BATCH}", "num_epoch=1", "sample_type=ppr_topk", f"ppr_alpha={ALPHA}", f"ppr_eps={EPS}",
            f"ppr_max_nodes={C}", f"ppr_max_rounds={ROUNDS}", f"num_neighbor={K}", "induced_subgraph=on"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    prefix = str(tmp_path / "w")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, path, prefix, "arch1", "1"] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(f"{prefix}.w0.npz")
    keys = batch_keys(got)
    assert keys == list(range(len(keys))) and len(keys) >= 4
    for key in keys:
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = ref.sample_batch(ip, ix, out, 2, ALPHA, EPS, C, ROUNDS, K)
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "data"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"].view(np.uint32), wl[name], err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
        assert want["layers"][0]["row"].size > want["layers"][1]["row"].size > 0
