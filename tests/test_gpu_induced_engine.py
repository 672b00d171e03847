"""induced_subgraph through the engine (arch1): for every batch of an epoch the delivered induced arrays are the numpy
statement's (tests/induced_ref.py) on the batch's own input nodes, num_induced is exact, the edge rows are table[eid] bit
for bit; the twin run without the key delivers the same batch and its accessors die by name; a capacity of 1 dies with
the key and the count it needed.

The graph is a multigraph: lists of 4 .. 40 entries drawn from 12 candidates each (parallel edges in every list), some
self-loops, node 0 a hub of 1100 entries; edge types are sorted inside every list (khop_typed reads them, nobody else).
A batch reaches most of the graph, so its induced subgraph holds far more edges than its sampled layers: the runs give
induced_max_edges = NUM_EDGE (the default, the layers' capacity, is what test_induced_config.py pins)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import induced_ref as ref
import khop_typed_ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features, feature_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "induced_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, R = 1500, 1100, 64, 2, 21, 3
TYPE_FANOUT = [[3, 1, 1], [2, 2, 0]]  # khop_typed, by layer id; the layers' fanouts are 5 and 4
FANOUT = [sum(row) for row in TYPE_FANOUT]
GETTERS = ["get_graph_num_induced", "get_graph_induced_row", "get_graph_induced_col", "get_graph_induced_edge_ids",
           "get_graph_induced_edge_feat"]


def multigraph():
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    lists = []
    for v in range(NODES):
        cand = rng.randint(0, NODES, 300 if v == 0 else 12)
        lst = cand[rng.randint(0, cand.size, deg[v])]
        if v % 50 == 1:
            lst[0] = v  # a self-loop
        lists.append(lst)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = np.concatenate(lists).astype(np.uint32)
    return ip, ix, khop_typed_ref.sorted_types(ip, rng, R, [0.6, 0.3, 0.1])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    ip, ix, et = multigraph()
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    edges = np.random.RandomState(3).permutation(ix.size)[:5 * BATCH].astype(np.uint32)
    table = feature_rows(np.arange(ix.size), 3, np.float32)  # a function of the POSITION: parallel edges differ
    path = str(tmp_path_factory.mktemp("induced_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_feat=table, edge_type=et, num_edge_type=R)
    return dict(path=path, ip=ip, ix=ix, table=table)


def drive(d, prefix, args, ok=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    if not ok:
        return r
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


def names_of(task):
    names = ["input_nodes", "output_nodes", "feat", "label"]
    for i in range(len(FANOUT)):
        names += [f"row{i}", f"col{i}", f"num_src{i}", f"num_dst{i}"]
    if task == "link_prediction":
        names += ["seed_ids", "pos_src", "pos_dst", "neg_src", "neg_dst", "link_edge_ids"]
    return names


#        sampler       task                   pipelines table     edge_feat
CASES = [("khop3",      "node_classification", 1, "direct", True),
         ("khop3",      "link_prediction",     2, "hashed", False),
         ("khop_labor", "node_classification", 2, "hashed", True),
         ("khop_labor", "link_prediction",     1, "direct", False),
         ("khop_typed", "node_classification", 2, "direct", False),
         ("khop_typed", "link_prediction",     1, "hashed", True)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_carries_its_induced_subgraph(dataset, tmp_path, case):
    sampler, task, pipes, table_kind, with_rows = case
    d = dataset
    ip, ix, table = d["ip"], d["ix"], d["table"]
    base = args_of(sampler, task, pipes, table_kind, **(dict(edge_feat="on") if with_rows else {}))
    got = drive(d, str(tmp_path / "keys"), base + ["induced_subgraph=on", f"induced_max_edges={ix.size}"])
    twin = drive(d, str(tmp_path / "twin"), base)
    same_batches(got, twin, names_of(task))  # the same layers, input nodes, features and labels, bit for bit
    assert not any(":ind_" in k or ":num_induced" in k for k in twin.files)
    loops = parallel = 0
    for key in batch_keys(got):
        nodes = got[f"{key}:input_nodes"].view(np.uint32)
        row, col, eid, M, _ = ref.induced_edges(ip, ix, nodes)
        print(f"batch {key}: {nodes.size} input nodes induce {M} edges; delivered {int(got[f'{key}:num_induced'])}")
        assert int(got[f"{key}:num_induced"]) == M
        for name, want in (("ind_row", row), ("ind_col", col), ("ind_eid", eid)):
            np.testing.assert_array_equal(got[f"{key}:{name}"].view(np.uint32), want, err_msg=f"batch {key} {name}")
        sampled = sum(got[f"{key}:row{i}"].size for i in range(len(FANOUT)))
        assert M > 2048  # more than one edge tile of hits
        assert np.unique(nodes).size == nodes.size and sampled > 0
        loops += int((row == col).sum())
        parallel += M - np.unique(np.stack([row, col], 1), axis=0).shape[0]
        if with_rows:
            rows = got[f"{key}:ind_efeat"]
            assert rows.dtype == table.dtype and rows.shape == (M, table.shape[1])
            np.testing.assert_array_equal(rows.view(np.uint8), table[eid].view(np.uint8), err_msg=f"batch {key} rows")
    assert loops > 0 and parallel > 0


@pytest.mark.parametrize("getter", GETTERS)
def test_without_the_key_the_accessors_die_by_name(dataset, tmp_path, getter):
    r = drive(dataset, str(tmp_path / "probe"), args_of("khop3", "node_classification") + [f"probe={getter}"], ok=False)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "probe") + ".w0.npz")
    assert f"samgraph_{getter} needs the config key induced_subgraph = on" in r.stderr, r.stderr[-2000:]


def test_edge_rows_need_edge_feat(dataset, tmp_path):
    r = drive(dataset, str(tmp_path / "probe"), args_of("khop3", "node_classification", induced_subgraph="on",
                                                       induced_max_edges=dataset["ix"].size) +
              ["probe=get_graph_induced_edge_feat"], ok=False)
    assert r.returncode != 0 and "needs the config key edge_feat = on" in r.stderr, r.stderr[-2000:]


def test_a_capacity_of_one_dies_with_the_key_and_the_needed_count(dataset, tmp_path):
    d = dataset
    base = args_of("khop_labor", "node_classification")  # stateless: the first batch is the same in both runs
    r = drive(d, str(tmp_path / "full"), base + ["induced_subgraph=on", "induced_max_edges=1"], ok=False)
    assert r.returncode != 0
    m = re.search(r"induced_subgraph: batch (\d+): its (\d+) input nodes induce (\d+) edges, capacity 1 "
                  r"\(config key induced_max_edges: at least (\d+)\)", r.stderr)
    assert m, r.stderr[-2000:]
    key, num_input, need, again = (int(x) for x in m.groups())
    assert need == again > 1
    ok = drive(d, str(tmp_path / "ok"), base + ["induced_subgraph=on", f"induced_max_edges={d['ix'].size}"])
    assert int(ok[f"{key}:num_induced"]) == need and ok[f"{key}:input_nodes"].size == num_input
