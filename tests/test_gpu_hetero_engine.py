"""hetero_batch through the engine (arch1, khop_typed, both tasks, 1 and 2 pipelines, both tables): every batch's typed
outputs are the numpy statement (tests/hetero_ref.py) replayed from that batch's OWN homogeneous outputs; every edge of
block r joins the relation table's source and destination types; row s of the features is the table row of
typed_nodes[s]; the per-type counts are the prefix counts; the twin run without the key delivers the same homogeneous
outputs bit for bit, and its hetero accessors die by name.

The graph: 1500 nodes of T = 3 types, lists of 4 .. 40 entries, node 0 a hub of 1100; the R = 9 relations come from
datagen.relation_types (relation r joins source type r % 3 to destination type r // 3), the lists are sorted by type."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_ref as ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "hetero_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, T = 1500, 1100, 64, 2, 21, 3
R = T * T
TYPE_FANOUT = [[2, 1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1, 0]]  # by layer id
FANOUT = [sum(row) for row in TYPE_FANOUT]
L = len(FANOUT)
DIM = 20
GETTERS = ["get_graph_node_slot", "get_graph_rel_row", "relation_src_type"]  # a node tensor, a block, the run's table; all
#                                                                             fourteen: tests/test_hetero_config.py


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = rng.randint(0, NODES, int(ip[-1])).astype(np.uint32)
    nt = rng.choice(T, NODES, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, nt, T))
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=DIM, num_class=13))
    edges = np.random.RandomState(3).permutation(ix.size)[:5 * BATCH].astype(np.uint32)
    path = str(tmp_path_factory.mktemp("hetero_ds"))
    datagen.write_dataset(path, g, feat=exact_features(NODES, DIM, np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_type=et, num_edge_type=R, node_type=nt, num_node_type=T)
    return dict(path=path, ip=ip, ix=ix, et=et, nt=nt, table=exact_features(NODES, DIM, np.float32))


def drive(d, prefix, args, ok=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


def args_of(task, pipes=1, table="direct", **keys):
    a = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
         "sample_type=khop_typed", f"pipelines={pipes}", "lookahead=2", f"task={task}", f"hash_table={table}",
         "type_fanout=" + "/".join(",".join(map(str, row)) for row in TYPE_FANOUT)]
    if task == "link_prediction":
        a.append(f"num_negative={K}")
    return a + [f"{k}={v}" for k, v in keys.items()]


def names_of(task):
    names = ["input_nodes", "output_nodes", "label"]
    for i in range(L):
        names += [f"row{i}", f"col{i}", f"num_src{i}", f"num_dst{i}", f"eid{i}", f"etype{i}"]
    if task == "link_prediction":
        names += ["seed_ids", "pos_src", "pos_dst", "neg_src", "neg_dst", "link_edge_ids"]
    return names


#        task                   pipelines table
CASES = [("node_classification", 1, "direct"), ("node_classification", 2, "hashed"),
         ("link_prediction", 1, "hashed"), ("link_prediction", 2, "direct")]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_batch_carries_its_typed_view(dataset, tmp_path, case):
    task, pipes, table_kind = case
    d = dataset
    nt, table = d["nt"], d["table"]
    base = args_of(task, pipes, table_kind)
    got = drive(d, str(tmp_path / "keys"), base + ["hetero_batch=on"])
    twin = drive(d, str(tmp_path / "twin"), base)
    same_batches(got, twin, names_of(task))  # the homogeneous outputs, bit for bit
    assert not any(":ntype" in k or ":rel_row" in k for k in twin.files)
    blocks = 0
    for key in batch_keys(got):
        g = lambda name: got[f"{key}:{name}"]  # noqa: E731
        nodes = g("input_nodes").view(np.uint32)
        cuts = [int(g(f"num_src{i}")) for i in range(L)] + [int(g(f"num_dst{L - 1}"))]
        assert cuts[0] == nodes.size and all(int(g(f"num_dst{i}")) == cuts[i + 1] for i in range(L))
        want = ref.hetero_nodes(nt, T, nodes, cuts)
        assert int(g("num_node_type")) == T
        for name in ("ntype", "local", "slot"):
            np.testing.assert_array_equal(g(name).view(want[name].dtype), want[name], err_msg=f"batch {key} {name}")
        typed_all = np.concatenate([g(f"typed{t}").view(np.uint32) for t in range(T)])
        np.testing.assert_array_equal(typed_all, want["typed_nodes"], err_msg=f"batch {key} typed_nodes")
        for t in range(T):
            assert g(f"typed{t}").size == want["base"][t + 1] - want["base"][t]
            assert (nt[g(f"typed{t}").view(np.uint32)] == t).all()
            # the per-type counts of a layer are the counts of its prefix of the input nodes
            np.testing.assert_array_equal(g(f"src_of{t}"), [(nt[nodes[:cuts[i]]] == t).sum() for i in range(L)])
            np.testing.assert_array_equal(g(f"dst_of{t}"), [(nt[nodes[:cuts[i + 1]]] == t).sum() for i in range(L)])
            np.testing.assert_array_equal(g(f"feat{t}").view(np.uint8), table[g(f"typed{t}").view(np.uint32)].view(np.uint8))
        # row s of the features belongs to typed_nodes[s]; the twin's rows are the same rows in input order
        np.testing.assert_array_equal(g("feat").view(np.uint8), table[typed_all].view(np.uint8), err_msg=f"batch {key} feat")
        np.testing.assert_array_equal(g("feat")[want["slot"]], twin[f"{key}:feat"], err_msg=f"batch {key} feat by slot")
        rows, cols, eids, ets = ([g(f"{n}{i}").view(np.uint32 if n != "etype" else np.uint8) for i in range(L)]
                                 for n in ("row", "col", "eid", "etype"))
        w_row, w_col, w_eid, w_off = ref.hetero_edges(rows, cols, eids, ets, R, want["local"])
        rel_src, rel_dst = g("rel_src"), g("rel_dst")
        for i in range(L):
            assert w_off[i, R] == rows[i].size  # every sampled edge is in exactly one block
            for r in range(R):
                a, b = int(w_off[i, r]), int(w_off[i, r + 1])
                np.testing.assert_array_equal(g(f"rel_row{i}_{r}").view(np.uint32), w_row[i][a:b], err_msg=f"{key} row {i} {r}")
                np.testing.assert_array_equal(g(f"rel_col{i}_{r}").view(np.uint32), w_col[i][a:b], err_msg=f"{key} col {i} {r}")
                np.testing.assert_array_equal(g(f"rel_eid{i}_{r}").view(np.uint32), w_eid[i][a:b], err_msg=f"{key} eid {i} {r}")
                if b > a:  # the block's ends, through their types' lists, have the relation table's types -- and are the edge
                    blocks += 1
                    assert (rel_src[r], rel_dst[r]) == (r % T, r // T)
                    src = g(f"typed{rel_src[r]}").view(np.uint32)[g(f"rel_row{i}_{r}").view(np.uint32)]
                    dst = g(f"typed{rel_dst[r]}").view(np.uint32)[g(f"rel_col{i}_{r}").view(np.uint32)]
                    assert (nt[src] == rel_src[r]).all() and (nt[dst] == rel_dst[r]).all()
                    eid = g(f"rel_eid{i}_{r}").view(np.uint32).astype(np.int64)
                    np.testing.assert_array_equal(d["ix"][eid], src)
                    assert (d["et"][eid] == r).all()
                    assert (d["ip"][dst] <= eid).all() and (eid < d["ip"][dst.astype(np.int64) + 1]).all()
                    # a layer's ends lie inside its per-type source / destination counts
                    assert g(f"rel_row{i}_{r}").view(np.uint32).max() < g(f"src_of{rel_src[r]}")[i]
                    assert g(f"rel_col{i}_{r}").view(np.uint32).max() < g(f"dst_of{rel_dst[r]}")[i]
    assert blocks > 4 * R  # most relations show up in most layers


@pytest.mark.parametrize("getter", GETTERS)
def test_without_the_key_the_accessors_die_by_name(dataset, tmp_path, getter):
    r = drive(dataset, str(tmp_path / "probe"), args_of("node_classification") + [f"probe={getter}"], ok=False)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "probe") + ".w0.npz")
    assert f"samgraph_{getter} needs the config key hetero_batch = on" in r.stderr, r.stderr[-2000:]
