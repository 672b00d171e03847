"""sample_type khop_typed_temporal through the engine (arch1, task = link_prediction): every batch is the numpy statement
(tests/khop_typed_temporal_ref.py) replayed from the batch's own output nodes and the times of its positive edges, under
the salt of the batch's key -- layers, edge ids, types, times, node cuts, link times.  With hetero_batch = on and typed
negatives every layer's relation blocks are exactly the layer's edges split by type (tests/hetero_ref.py).

The graph: 2000 nodes of 2 types, 3 relations from datagen.relation_types (type-1 nodes only have type-0 neighbours, so
relation 3 does not occur), lists sorted by (type, time); node 0 is a hub of 2500 early entries."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_ref
import khop_labor_ref as labor
import khop_typed_temporal_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "typed_temporal_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, T, R = 2000, 2500, 64, 2, 21, 2, 3
TYPE_FANOUT = [[3, 1, 1], [2, 2, 1]]  # by layer id
L = len(TYPE_FANOUT)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    nt = rng.choice(T, NODES, p=[0.6, 0.4]).astype(np.uint8)
    nt[0] = 0
    zero = np.flatnonzero(nt == 0)
    u = rng.randint(0, NODES, int(ip[-1]))
    ix = np.where(np.repeat(nt, deg) == 1, zero[u % zero.size], u).astype(np.uint32)
    tm = rng.randint(1, 200, ix.size)
    tm[:HUB_DEG] = rng.randint(1, 6, HUB_DEG)
    ix, et, tm, _ = datagen.sort_lists_by_type_time(ip, ix, datagen.relation_types(ip, ix, nt, T), tm)
    assert et.max() == R - 1
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    edges = (HUB_DEG + np.random.RandomState(3).permutation(ix.size - HUB_DEG)[:5 * BATCH]).astype(np.uint32)
    path = str(tmp_path_factory.mktemp("typed_temporal_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_type=et, num_edge_type=R, edge_time=tm, node_type=nt, num_node_type=T)
    return dict(path=path, ip=ip, ix=ix, et=et, tm=tm, nt=nt, edges=edges)


#        pick       pipelines table    hetero_batch + typed negatives
CASES = [("uniform", 1, "direct", False), ("recent", 2, "hashed", False), ("uniform", 2, "direct", True)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_equals_the_reference(dataset, tmp_path, case):
    pick_name, pipes, table_kind, hetero = case
    d = dataset
    ip, ix, et, tm, nt = d["ip"], d["ix"], d["et"], d["tm"], d["nt"]
    args = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(str(sum(row)) for row in TYPE_FANOUT),
            "num_epoch=1", "sample_type=khop_typed_temporal", f"pipelines={pipes}", "lookahead=2", "task=link_prediction", f"num_negative={K}", f"hash_table={table_kind}",
            f"temporal_pick={pick_name}", "type_fanout=" + "/".join(",".join(map(str, row)) for row in TYPE_FANOUT)]
    if hetero:
        args += ["hetero_batch=on", "negative_mode=typed_uniform"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], str(tmp_path / "t")] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(str(tmp_path / "t") + ".w0.npz")
    steps = int(got["steps_per_epoch"])
    assert batch_keys(got) == list(range(steps)) and steps >= 4
    pick = ref.RECENT if pick_name == "recent" else ref.UNIFORM
    taken = []
    for key in batch_keys(got):
        g = lambda name, dt=np.uint32: got[f"{key}:{name}"].view(dt)  # noqa: E731
        out, pos = g("output_nodes"), g("link_edge_ids")
        assert out.size == (2 + K) * pos.size
        np.testing.assert_array_equal(g("link_time"), tm[pos])
        seed_time = np.concatenate([tm[pos], tm[pos], np.repeat(tm[pos], K)])
        want = ref.sample_batch(ip, ix, et, tm, out, seed_time, TYPE_FANOUT, labor.batch_salt(SEED, key // steps, key % steps), pick)
        for name in ("input_nodes", "node_cut"):
            np.testing.assert_array_equal(g(name), want[name], err_msg=f"{key}: {name}")
        np.testing.assert_array_equal(g("seed_ids"), want["seed_local"], err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "eid"):
                np.testing.assert_array_equal(g(f"{name}{i}"), wl[name], err_msg=f"{key}: {name}{i}")
            np.testing.assert_array_equal(g(f"etype{i}", np.uint8), wl["etype"], err_msg=f"{key}: etype{i}")
            np.testing.assert_array_equal(g(f"etime{i}"), tm[wl["eid"].astype(np.int64)], err_msg=f"{key}: etime{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
        taken += pos.tolist()
        if hetero:  # the relation blocks: the layer's edges split by type, in the types' local ids
            nodes = want["input_nodes"]
            cuts = [wl["num_src"] for wl in want["layers"]] + [want["layers"][L - 1]["num_dst"]]
            local = hetero_ref.hetero_nodes(nt, T, nodes, cuts)["local"]
            layers = ([wl[n] for wl in want["layers"]] for n in ("row", "col", "eid", "etype"))
            w_row, w_col, w_eid, w_off = hetero_ref.hetero_edges(*layers, R, local)
            for i in range(L):
                assert w_off[i, R] == want["layers"][i]["row"].size
                for r in range(R):
                    a, b = int(w_off[i, r]), int(w_off[i, r + 1])
                    for name, w in (("rel_row", w_row), ("rel_col", w_col), ("rel_eid", w_eid)):
                        np.testing.assert_array_equal(g(f"{name}{i}_{r}"), w[i][a:b], err_msg=f"{key} {name} {i} {r}")
                    assert (et[g(f"rel_eid{i}_{r}").astype(np.int64)] == r).all()
    assert sorted(taken) == sorted(d["edges"].tolist())  # the epoch hands out the shuffled train-edge set, once
