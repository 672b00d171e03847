"""sample_type random_walk_metapath through the engine (arch1, 2 layers): every batch of an epoch is the numpy statement
(tests/walk_metapath_ref.py) replayed from the batch's own output nodes under the salt of the batch's key -- input
nodes, row, col and the visit counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_typed_ref as typed
import walk_metapath_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features, powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "engine_driver.py")
NODES, BATCH, SEED, PATH, T, P, W, K = 3000, 64, 21, [0, 1], 2, 0.25, 3, 4


def test_every_batch_equals_the_reference(tmp_path):
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(NODES, mean_deg=12, seed=9)
    et = typed.sorted_types(ip, np.random.RandomState(9), 3)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 10, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    path = str(tmp_path / "ds")
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          edge_type=et, num_edge_type=3)
    args = [f"seed={SEED}", f"batch_size={BATCH}", "num_epoch=1", "sample_type=random_walk_metapath",
            "metapath=" + " ".join(map(str, PATH)), f"random_walk_length={T}", f"random_walk_restart_prob={P}",
            f"num_random_walk={W}", f"num_neighbor={K}"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    prefix = str(tmp_path / "w")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, path, prefix, "arch1", "1"] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(f"{prefix}.w0.npz")
    keys = batch_keys(got)
    steps = len(keys)
    assert keys == list(range(steps)) and steps >= 4
    for key in keys:
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = ref.sample_batch(ip, ix, et, PATH, out, 2, T, P, W, K, labor.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "data"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"].view(np.uint32), wl[name], err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
        assert want["layers"][0]["row"].size > want["layers"][1]["row"].size > 0
