"""sample_type khop_labor_weighted through the engine (arch1, both tasks): every batch is the numpy statement
(tests/khop_labor_weighted_ref.py) replayed from the batch's own output nodes under the salt of the batch's key, and the
delivered weights are the file's at the delivered edge ids.  Node 0 is a hub of 1100 entries (the workgroup route)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_labor_weighted_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features, powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "labor_weighted_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, FANOUT = 1500, 1100, 64, 2, 21, [5, 4]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    rng = np.random.RandomState(9)
    ip, ix = powerlaw_csr(NODES, mean_deg=12, seed=9)
    ix = np.concatenate([rng.randint(0, NODES, HUB_DEG), ix[ip[1]:]]).astype(np.uint32)  # node 0 becomes the hub
    ip = np.concatenate([[0], ip[1:].astype(np.int64) - int(ip[1]) + HUB_DEG]).astype(np.uint32)
    ew = np.exp2(rng.uniform(-8, 8, ix.size)).astype(np.float32)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    edges = np.concatenate([np.arange(40), HUB_DEG + rng.permutation(ix.size - HUB_DEG)[:5 * BATCH - 40]]).astype(np.uint32)
    path = str(tmp_path_factory.mktemp("labor_weighted_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_weight=ew)
    return dict(path=path, ip=ip, ix=ix, ew=ew)


#        task                   pipelines table
CASES = [("node_classification", 1, "direct"), ("link_prediction", 2, "hashed")]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_equals_the_reference(dataset, tmp_path, case):
    task, pipes, table = case
    d = dataset
    args = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
            "sample_type=khop_labor_weighted", f"pipelines={pipes}", "lookahead=2", f"task={task}", f"hash_table={table}"]
    if task == "link_prediction":
        args.append(f"num_negative={K}")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    prefix = str(tmp_path / "w")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(f"{prefix}.w0.npz")
    steps = int(got["steps_per_epoch"])
    assert batch_keys(got) == list(range(steps)) and steps >= 4
    hub_sampled = False
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = ref.sample_batch(d["ip"], d["ix"], d["ew"], out, FANOUT, labor.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "eid"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"].view(np.uint32), wl[name], err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
            eid = got[f"{key}:eid{i}"].view(np.uint32).astype(np.int64)
            np.testing.assert_array_equal(got[f"{key}:eweight{i}"].view(np.uint32), d["ew"][eid].view(np.uint32))
            hub_sampled |= bool((eid < HUB_DEG).any())
    assert hub_sampled  # the hub's list went through the workgroup route
