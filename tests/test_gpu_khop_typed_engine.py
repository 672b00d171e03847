"""sample_type khop_typed through the engine (arch1, both tasks): every batch is the numpy statement
(tests/khop_typed_ref.py) replayed from the batch's own output nodes under the salt of the batch's key; every (col node,
type) pair has min(k_r, e_r) edges; the delivered types are the file's at the delivered ids; the edge rows are table[eid]
on a graph whose parallel edges of different relations carry different rows; and a khop_labor run on the same data set
is untouched by the types lying beside it.

The graph is a multigraph: every list holds a few ids several times, under different relations, and the hub's first
relation has 1060 entries, more than the wave routes' 1024."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_typed_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features, feature_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "typed_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, R = 1500, 1100, 64, 2, 21, 3
TYPE_FANOUT = [[3, 1, 1], [2, 2, 0]]  # by layer id; the layers' fanouts are 5 and 4
FANOUT = [sum(row) for row in TYPE_FANOUT]


def multigraph():
    """Lists of 4 .. 40 entries drawn from 12 candidates each (parallel edges in every list), node 0 a hub; types sorted
    inside every list, the third relation rare."""
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    lists = []
    for v in range(NODES):
        cand = rng.randint(0, NODES, 300 if v == 0 else 12)
        lists.append(cand[rng.randint(0, cand.size, deg[v])])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = np.concatenate(lists).astype(np.uint32)
    et = ref.sorted_types(ip, rng, R, [0.6, 0.3, 0.1])
    et[:HUB_DEG] = np.repeat(np.arange(R), [HUB_DEG - 40, 30, 10])  # the hub: a segment for the workgroup route
    return ip, ix, et


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    ip, ix, et = multigraph()
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    rng = np.random.RandomState(3)
    edges = np.concatenate([HUB_DEG + rng.permutation(ix.size - HUB_DEG)[:5 * BATCH - 40],
                            np.arange(HUB_DEG - 40, HUB_DEG)]).astype(np.uint32)
    table = feature_rows(np.arange(ix.size), 3, np.float32)  # a function of the POSITION: parallel edges differ
    path = str(tmp_path_factory.mktemp("typed_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_feat=table, edge_type=et, num_edge_type=R)
    return dict(path=path, ip=ip, ix=ix, et=et, table=table, edges=edges)


def drive(d, prefix, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


def args_of(sampler, task, pipes=1, table="direct", **keys):
    a = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
         f"sample_type={sampler}", f"pipelines={pipes}", "lookahead=2", f"task={task}", f"hash_table={table}"]
    if task == "link_prediction":
        a.append(f"num_negative={K}")
    if sampler == "khop_typed":
        a.append("type_fanout=" + "/".join(",".join(map(str, row)) for row in TYPE_FANOUT))
    return a + [f"{k}={v}" for k, v in keys.items()]


#        task                   pipelines table     edge_feat
CASES = [("node_classification", 1, "direct", True), ("node_classification", 2, "hashed", False),
         ("link_prediction", 1, "hashed", False), ("link_prediction", 2, "direct", True)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_equals_the_reference(dataset, tmp_path, case):
    task, pipes, table_kind, with_rows = case
    d = dataset
    ip, ix, et, table = d["ip"], d["ix"], d["et"], d["table"]
    keys = dict(edge_feat="on") if with_rows else {}
    got = drive(d, str(tmp_path / "t"), args_of("khop_typed", task, pipes, table_kind, **keys))
    steps = int(got["steps_per_epoch"])
    assert batch_keys(got) == list(range(steps)) and steps >= 4
    seg = np.stack([np.searchsorted(et[ip[v]:ip[v + 1]], np.arange(R + 1)) for v in range(NODES)])  # b_r of every node
    e_r = np.diff(seg, axis=1)
    parallel, hub_sampled = 0, False
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = ref.sample_batch(ip, ix, et, out, TYPE_FANOUT, labor.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        if task == "link_prediction":
            assert out.size == (2 + K) * got[f"{key}:link_edge_ids"].size
            np.testing.assert_array_equal(got[f"{key}:seed_ids"].view(np.uint32), want["seed_local"], err_msg=f"{key}")
        nodes = want["input_nodes"].astype(np.int64)
        for i, wl in enumerate(want["layers"]):
            for name in ("row", "col", "eid"):
                np.testing.assert_array_equal(got[f"{key}:{name}{i}"].view(np.uint32), wl[name], err_msg=f"{key}: {name}{i}")
            assert (got[f"{key}:num_src{i}"], got[f"{key}:num_dst{i}"]) == (wl["num_src"], wl["num_dst"])
            # from the delivered arrays alone: the types are the file's at the delivered ids, and every (col node, type)
            # pair has min(k_r, e_r) edges
            eid = got[f"{key}:eid{i}"].view(np.uint32).astype(np.int64)
            typ = got[f"{key}:etype{i}"]
            col = got[f"{key}:col{i}"].view(np.uint32).astype(np.int64)
            row = got[f"{key}:row{i}"].view(np.uint32).astype(np.int64)
            assert typ.dtype == np.uint8
            np.testing.assert_array_equal(typ, et[eid], err_msg=f"{key}: etype{i}")
            count = np.zeros((nodes.size, R), np.int64)
            np.add.at(count, (col, typ.astype(np.int64)), 1)
            # how often a node is sampled in the layer: the first layer's raw seeds may repeat, later frontiers do not
            times = (np.bincount(want["seed_local"], minlength=nodes.size) if i == len(FANOUT) - 1
                     else (np.arange(nodes.size) < wl["num_dst"]).astype(np.int64))
            np.testing.assert_array_equal(count, times[:, None] * np.minimum(e_r[nodes], np.array(TYPE_FANOUT[i])))
            if with_rows:
                rows = got[f"{key}:efeat{i}"]
                np.testing.assert_array_equal(rows.view(np.uint8), table[eid].view(np.uint8), err_msg=f"{key}: efeat{i}")
                # two parallel edges of different relations: the same (col, row), other types, other positions -- and
                # their rows differ as the table does
                order = np.lexsort((typ, row, col))
                c, r_, t, e = col[order], row[order], typ[order], eid[order]
                twin = np.flatnonzero((c[1:] == c[:-1]) & (r_[1:] == r_[:-1]) & (t[1:] != t[:-1]))
                parallel += twin.size
                sorted_rows = rows[order]
                for q in twin[:20]:
                    assert e[q] != e[q + 1] and (table[e[q]] != table[e[q + 1]]).any()
                    assert (sorted_rows[q] != sorted_rows[q + 1]).any()
            hub_sampled |= bool((nodes[col] == 0).any())
    assert hub_sampled  # the hub's first relation went through the workgroup route
    if with_rows:
        assert parallel > 0


def test_khop_labor_on_the_same_data_set_is_untouched(dataset, tmp_path):
    """The control: a khop_labor run on the data set that carries edge_type.bin is khop_labor_ref's, batch for batch (what
    it was before the types existed), and hands out no types."""
    d = dataset
    got = drive(d, str(tmp_path / "labor"), args_of("khop_labor", "node_classification", edge_ids="on"))
    steps = int(got["steps_per_epoch"])
    for key in batch_keys(got):
        out = got[f"{key}:output_nodes"].view(np.uint32)
        want = labor.sample_batch(d["ip"], d["ix"], out, FANOUT, labor.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(got[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"])
        for i, wl in enumerate(want["layers"]):
            np.testing.assert_array_equal(got[f"{key}:row{i}"].view(np.uint32), wl["row"])
            np.testing.assert_array_equal(got[f"{key}:col{i}"].view(np.uint32), wl["col"])
    assert not any("etype" in k for k in got.files)
