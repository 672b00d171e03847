"""sample_type khop_temporal through the engine (arch1, task = link_prediction): every batch is the numpy statement
(tests/khop_temporal_ref.py) replayed from the batch's own output nodes and the times of its positive edges, under the
salt of the batch's key; the edge rows and edge times are table[eid] and edge_time[eid] on a graph whose parallel edges
carry different rows; and a khop_labor run on the same data set is untouched by the times lying beside it.

The graph is a multigraph: every list holds a few ids several times, at different times, and one hub list of 1100
entries is longer than the wave routes' 1024."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_temporal_ref as ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features, feature_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "temporal_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, FANOUT = 1500, 1100, 64, 2, 21, [5, 4]


def multigraph():
    """Lists of 4 .. 40 entries drawn from 12 candidates each (parallel edges in every list), node 0 a hub; times sorted
    inside every list with ties."""
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    lists = []
    for v in range(NODES):
        cand = rng.randint(0, NODES, 300 if v == 0 else 12)
        lists.append(cand[rng.randint(0, cand.size, deg[v])])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = np.concatenate(lists).astype(np.uint32)
    et = ref.sorted_times(ip, rng, 1, 200)
    # the hub: 1060 early entries, then the 40 the data set's hub positives are taken from -- a batch with one of them
    # samples the hub from a prefix of more than 1024 entries
    et[:HUB_DEG] = np.concatenate([np.sort(rng.randint(1, 6, HUB_DEG - 40)), np.sort(rng.randint(50, 200, 40))])
    return ip, ix, et


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    ip, ix, et = multigraph()
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    rng = np.random.RandomState(3)
    # (no other positive from the hub's list: an early one would cut the hub's prefix short in its batch)
    edges = np.concatenate([HUB_DEG + rng.permutation(ix.size - HUB_DEG)[:5 * BATCH - 40],
                            np.arange(HUB_DEG - 40, HUB_DEG)]).astype(np.uint32)
    table = feature_rows(np.arange(ix.size), 3, np.float32)  # a function of the POSITION: parallel edges differ
    path = str(tmp_path_factory.mktemp("temporal_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_feat=table, edge_time=et)
    return dict(path=path, ip=ip, ix=ix, et=et, table=table, edges=edges)


def drive(d, prefix, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


def args_of(sampler, pipes=1, table="direct", **keys):
    a = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
         f"sample_type={sampler}", f"pipelines={pipes}", "lookahead=2", "task=link_prediction", f"num_negative={K}",
         f"hash_table={table}"]
    return a + [f"{k}={v}" for k, v in keys.items()]


#        pick       pipelines table     edge_feat
CASES = [("uniform", 1, "direct", True), ("recent", 2, "hashed", False), ("uniform", 2, "direct", False),
         ("recent", 1, "direct", True), ("uniform", 1, "hashed", False)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_equals_the_reference(dataset, tmp_path, case):
    pick_name, pipes, table_kind, with_rows = case
    d = dataset
    ip, ix, et, table = d["ip"], d["ix"], d["et"], d["table"]
    pick = ref.RECENT if pick_name == "recent" else ref.UNIFORM
    keys = dict(temporal_pick=pick_name)
    if with_rows:
        keys["edge_feat"] = "on"
    got = drive(d, str(tmp_path / "t"), args_of("khop_temporal", pipes, table_kind, **keys))
    steps = int(got["steps_per_epoch"])
    assert batch_keys(got) == list(range(steps)) and steps >= 4
    taken, parallel, hub_prefix = [], 0, 0
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"].view(np.uint32)
        pos = got[f"{key}:link_edge_ids"].view(np.uint32)
        B = pos.size
        assert out.size == (2 + K) * B
        np.testing.assert_array_equal(got[f"{key}:link_time"].view(np.uint32), et[pos])
        seed_time = np.concatenate([et[pos], et[pos], np.repeat(et[pos], K)])
        want = ref.sample_batch(ip, ix, et, out, seed_time, FANOUT, labor.batch_salt(SEED, key // steps, key % steps), pick)
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        np.testing.assert_array_equal(got[f"{key}:node_cut"].view(np.uint32), want["node_cut"], err_msg=f"{key}")
        np.testing.assert_array_equal(got[f"{key}:seed_ids"].view(np.uint32), want["seed_local"], err_msg=f"{key}")
        nodes = want["input_nodes"].astype(np.int64)
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "eid"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"].view(np.uint32), wl[name], err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
            eid = wl["eid"].astype(np.int64)
            np.testing.assert_array_equal(got[f"{key}:etime{i}"].view(np.uint32), et[eid], err_msg=f"{key}: etime{i}")
            if with_rows:
                rows = got[f"{key}:efeat{i}"]
                np.testing.assert_array_equal(rows.view(np.uint8), table[eid].view(np.uint8), err_msg=f"{key}: efeat{i}")
            # positions of parallel edges that are NOT the first copy's: what a post-pass by (col, row) cannot name
            s, t = nodes[wl["col"]], nodes[wl["row"]]
            first = np.array([ip[a] + int(np.flatnonzero(ix[ip[a]:ip[a + 1]] == b)[0]) for a, b in zip(s, t)], np.int64)
            parallel += int((first != eid).sum())
            hub_prefix = max(hub_prefix, max([ref.eligible(et[ip[0]:ip[1]], c) for a, c in
                                              zip(nodes[: wl["cut_at_start"].size], wl["cut_at_start"]) if a == 0] or [0]))
        taken += pos.tolist()
        # nothing from the positive's own time on: a first-layer edge lies before the time of its seed
        first_layer = want["layers"][len(FANOUT) - 1]
        root = np.full(nodes.size, ref.INF, np.int64)
        np.minimum.at(root, want["seed_local"], seed_time.astype(np.int64))
        assert (et[got[f"{key}:eid{len(FANOUT) - 1}"].view(np.uint32)] < root[first_layer["col"]]).all()
    assert sorted(taken) == sorted(d["edges"].tolist())  # the epoch hands out the shuffled train-edge set, once
    assert parallel > 0 and hub_prefix > 1024  # later copies were sampled; the hub went through the workgroup route


def test_khop_labor_on_the_same_data_set_is_untouched(dataset, tmp_path):
    """The control: a khop_labor run on the data set that carries edge_time.bin is khop_labor_ref's, batch for batch (what
    it was before the times existed), and hands out no temporal arrays."""
    d = dataset
    got = drive(d, str(tmp_path / "labor"), args_of("khop_labor", edge_ids="on"))
    steps = int(got["steps_per_epoch"])
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = labor.sample_batch(d["ip"], d["ix"], out, FANOUT, labor.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"])
        for i, wl in enumerate(want["layers"]):
            np.testing.assert_array_equal(got[f"{key}:row{i}"].view(np.uint32), wl["row"])
            np.testing.assert_array_equal(got[f"{key}:col{i}"].view(np.uint32), wl["col"])
    assert not any("etime" in k or "node_cut" in k or "link_time" in k for k in got.files)
