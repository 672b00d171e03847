"""edge_ids / edge_feat through the engine (arch1): every layer's edge ids are the numpy statement's
(tests/edge_positions_ref.py) on the batch's own (input_nodes[col], input_nodes[row]), the edge rows are table[eid] bit for
bit, a link_prediction batch hands out its positives' edge ids, exclude_seed_edges composes with all of it, and the twin
run without the keys delivers the same batch.

The graph is simple and symmetric (no parallel edges, no self-loops): ring edges, chords, and one hub whose list of 1100
entries is longer than the long-list threshold of xgnn_amd/csrc/edge_positions.hip (1024); the layers are longer than a
wave's 64 and a workgroup's 256 edges.  The edge table is an exact function of the edge id."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_positions_ref as ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features, feature_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "edge_driver.py")
NODES, HUB_DEG, BATCH, K = 1500, 1100, 48, 2
TABLES = {"dim3_f32": (3, np.float32, "F32"), "dim8_f16": (8, np.float16, "F16")}
DISTINCT = ("khop0", "khop3", "khop_labor", "weighted_khop_hash_dedup")  # the samplers that draw without replacement


def simple_graph():
    n = NODES
    nb = [{(v + 1) % n, (v - 1) % n, (v + 2) % n, (v - 2) % n} for v in range(n)]
    rng = np.random.RandomState(9)
    for v, w in zip(rng.randint(1, n, 3000).tolist(), rng.randint(1, n, 3000).tolist()):
        if v != w:
            nb[v].add(w), nb[w].add(v)
    for w in range(3, 3 + HUB_DEG - 4):  # the hub: node 0
        nb[0].add(w), nb[w].add(0)
    deg = np.array([len(s) for s in nb])
    assert deg[0] == HUB_DEG > 1024 and deg.min() >= 4 and all(v not in nb[v] for v in range(n))
    lists = [rng.permutation(sorted(s)) for s in nb]
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    return ip, np.concatenate(lists).astype(np.uint32)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    from xgnn_amd import datagen
    ip, ix = simple_graph()
    train = np.concatenate([[0], np.arange(5, 5 + 5 * (5 * BATCH - 1), 5)]).astype(np.uint32)  # 5 batches, the hub a seed
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=20, num_class=13))
    edges = np.random.RandomState(3).permutation(ix.size)[:4 * BATCH].astype(np.uint32)
    out = {}
    for name, (dim, dt, code) in TABLES.items():
        path = str(tmp_path_factory.mktemp(f"edge_ds_{name}"))
        table = feature_rows(np.arange(ix.size), dim, dt)
        datagen.write_dataset(path, g, feat=exact_features(NODES, 20, np.float32), label=(np.arange(NODES) * 7) % 13,
                              train_edges=edges, weights=1.0 + (np.arange(ix.size) % 7).astype(np.float32),
                              edge_feat=table, edge_feat_dtype=code)
        out[name] = dict(path=path, ip=ip, ix=ix, table=table, edges=edges)
    return out


def drive(d, prefix, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


#        sampler                     fanout     table       pipelines lookahead task    exclude  keys
CASES = [("khop0",                    "5 3",   "dim3_f32", 1, 0, "node", None,   "edge_feat"),
         ("khop3",                    "3 2 2", "dim8_f16", 2, 2, "node", None,   "edge_feat"),
         ("khop_labor",               "5 3",   "dim3_f32", 1, 2, "link", "both", "edge_feat"),
         ("khop1",                    "3 2 2", "dim8_f16", 2, 2, "link", "none", "edge_feat"),
         ("weighted_khop",            "5 3",   "dim8_f16", 1, 0, "node", None,   "edge_feat"),
         ("weighted_khop_hash_dedup", "3 2 2", "dim3_f32", 2, 2, "link", "both", "edge_feat"),
         ("khop3",                    "5 3",   "dim3_f32", 1, 2, "link", "both", "edge_ids"),
         ("khop0",                    "3 2 2", "dim8_f16", 2, 2, "link", "none", "edge_ids")]


def args_of(case):
    sampler, fanout, _, pipes, ahead, task, exclude, _ = case
    a = ["seed=21", f"batch_size={BATCH}", f"fanout={fanout}", "num_epoch=1", f"sample_type={sampler}", f"pipelines={pipes}",
         f"lookahead={ahead}"]
    if task == "link":
        a += ["task=link_prediction", f"num_negative={K}", f"exclude_seed_edges={exclude}"]
    return a


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x).replace(" ", "_") for x in c) for c in CASES])
def test_edge_ids_and_rows_of_every_layer(datasets, tmp_path, case):
    sampler, fanout, table_name, _, _, task, exclude, keys = case
    d = datasets[table_name]
    ip, ix, table = d["ip"], d["ix"], d["table"]
    L = len(fanout.split())
    got = drive(d, str(tmp_path / "keys"), args_of(case) + [f"{keys}=on"])
    twin = drive(d, str(tmp_path / "twin"), args_of(case))
    names = ["input_nodes", "output_nodes", "feat", "label"]
    for i in range(L):
        names += [f"row{i}", f"col{i}", f"num_src{i}", f"num_dst{i}"]
    if task == "link":
        names += ["seed_ids", "pos_src", "pos_dst", "neg_src", "neg_dst", "link_edge_ids"]
    same_batches(got, twin, names)
    assert not any(":eid" in k or ":efeat" in k for k in twin.files)
    longest, taken = 0, []
    for key in batch_keys(got):
        nodes = got[f"{key}:input_nodes"].view(np.uint32)
        barred = set()
        if task == "link":
            pos = got[f"{key}:link_edge_ids"].view(np.uint32)
            out = got[f"{key}:output_nodes"].view(np.uint32)
            B = pos.size
            assert out.size == (2 + K) * B
            # the positives' ids lead to their endpoints through the CSR, and through the pair ids to the batch's nodes
            np.testing.assert_array_equal(ix[pos], out[B:2 * B])
            np.testing.assert_array_equal(np.searchsorted(ip, pos, side="right") - 1, out[:B])
            np.testing.assert_array_equal(nodes[got[f"{key}:pos_src"]], out[:B])
            np.testing.assert_array_equal(nodes[got[f"{key}:pos_dst"]], out[B:2 * B])
            taken += pos.tolist()
            if exclude == "both":
                barred = set(pos.tolist()) | {ref.first_position(ip, ix, v, u) for u, v in zip(out[:B], out[B:2 * B])}
                assert ref.EMPTY not in barred
        for i in range(L):
            row, col = got[f"{key}:row{i}"].view(np.uint32), got[f"{key}:col{i}"].view(np.uint32)
            eid = got[f"{key}:eid{i}"].view(np.uint32)
            s, t = nodes[col], nodes[row]
            want, = ref.edge_positions(ip, ix, [t], [s])
            np.testing.assert_array_equal(eid, want, err_msg=f"batch {key} layer {i}")
            assert (eid != ref.EMPTY).all()
            assert (ix[eid] == t).all() and (ip[s] <= eid).all() and (eid < ip[s.astype(np.int64) + 1]).all()
            longest = max(longest, int((ip[s.astype(np.int64) + 1] - ip[s]).max()))
            if keys == "edge_feat":
                rows = got[f"{key}:efeat{i}"]
                assert rows.dtype == table.dtype and rows.shape == (eid.size, table.shape[1])
                np.testing.assert_array_equal(rows.view(np.uint8), table[eid].view(np.uint8), err_msg=f"batch {key} layer {i}")
            if task == "node" and sampler in DISTINCT:  # one seed's edges are distinct edges
                pairs = np.stack([col.astype(np.int64), eid.astype(np.int64)], 1)
                assert np.unique(pairs, axis=0).shape[0] == eid.size, f"batch {key} layer {i}"
            assert not barred & set(eid.tolist()), f"batch {key} layer {i}: a positive or its mirror is still there"
        assert max(got[f"{key}:row{i}"].size for i in range(L)) > 256
    assert longest == HUB_DEG  # the long-list path was taken
    if task == "link":  # the epoch hands out the shuffled train-edge set, once
        assert sorted(taken) == sorted(d["edges"].tolist())
