"""sample_type khop_budget through the engine (arch1, both tasks, edge_ids = on): every batch is
ops.BudgetBatchSampler's, replayed from the batch's own output nodes under the salt of the batch's key, and no layer adds
more nodes than its budget.  Node 0 is a hub of 1100 entries (the workgroup route)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as labor
from engine_harness import batch_keys
from graphgen import exact_features, powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "engine_driver.py")
NODES, HUB_DEG, BATCH, SEED, FANOUT, LAYER_NODES = 1500, 1100, 64, 21, [5, 4], [150, 40]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@pytest.mark.parametrize("weight,task", [("uniform", "node_classification"), ("ladies", "node_classification"),
                                         ("ladies", "link_prediction")])
def test_every_batch_equals_the_batch_sampler(tmp_path, weight, task):
    from xgnn_amd import datagen, ops
    rng = np.random.RandomState(9)
    ip, ix = powerlaw_csr(NODES, mean_deg=12, seed=9)
    ix = np.concatenate([rng.randint(0, NODES, HUB_DEG), ix[ip[1]:]]).astype(np.uint32)  # node 0 becomes the hub
    ip = np.concatenate([[0], ip[1:].astype(np.int64) - int(ip[1]) + HUB_DEG]).astype(np.uint32)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    path = str(tmp_path / "ds")
    os.makedirs(path)
    edges = np.concatenate([np.arange(40), HUB_DEG + rng.permutation(ix.size - HUB_DEG)[:5 * BATCH - 40]]).astype(np.uint32)
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges)
    args = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
            "sample_type=khop_budget", "layer_nodes=" + " ".join(map(str, LAYER_NODES)), f"budget_weight={weight}",
            "edge_ids=on", f"task={task}"] + ["num_negative=2"] * (task == "link_prediction")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    prefix = str(tmp_path / "b")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, path, prefix, "arch1", "1"] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(f"{prefix}.w0.npz")
    steps = len(batch_keys(got))
    assert batch_keys(got) == list(range(steps)) and steps >= 4
    graph = ops.DeviceGraph(dev(ip), dev(ix))
    bs = ops.BudgetBatchSampler(graph, FANOUT, LAYER_NODES, 4 * BATCH, mode=ops.BUDGET_LADIES if weight == "ladies" else
                                ops.BUDGET_UNIFORM)
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"]
        bs.sample(dev(out), salt=labor.batch_salt(SEED, 0, key))
        want = bs.result()
        np.testing.assert_array_equal(got[f"{key}:input_nodes"], want["input_nodes"].cpu().numpy(), err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"], wl[name].cpu().numpy(), err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
            assert got[f"{key}:num_src{i}"] - got[f"{key}:num_dst{i}"] <= LAYER_NODES[i]
    graph.detach_heads()
