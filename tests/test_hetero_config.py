"""Config key hetero_batch on the host: which configurations config + data_init take (no GPU touched), every refusal by
name, what is wrong with a dataset's node types, and that every accessor dies by name without the key."""
import os
import shutil

import numpy as np
import pytest

from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen

T, N = 3, 600
TF = [[1] * 9, [1] * 8 + [0]]
TYPED = dict(_sample_type=10, type_fanout=TF, fanout=[9, 8])
ON = dict(TYPED, hetero_batch="on")
INFO = dict(SAMGRAPH_LOG_LEVEL="info")
GETTERS = {"get_graph_node_type": "0", "get_graph_node_local": "0", "get_graph_node_slot": "0",
           "get_graph_typed_nodes": "0, 0", "get_graph_feat_of_type": "0, 0", "get_graph_num_src_of_type": "0, 0, 0",
           "get_graph_num_dst_of_type": "0, 0, 0", "get_graph_rel_row": "0, 0, 0", "get_graph_rel_col": "0, 0, 0",
           "get_graph_rel_edge_ids": "0, 0, 0", "get_graph_rel_num_edges": "0, 0, 0", "num_node_type": "",
           "relation_src_type": "0", "relation_dst_type": "0"}


def write(path, ip, ix, et, nt, **kw):
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, N, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(path), g, feat=feature_rows(np.arange(N), 20), label=np.arange(N) % 13, edge_type=et,
                          num_edge_type=T * T, edge_feat=feature_rows(np.arange(ix.size), 3, np.float32), **kw)
    return str(path)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("hetero_cfg")
    ip, ix = powerlaw_csr(N, mean_deg=9, seed=2)
    nt = np.random.RandomState(1).randint(0, T, N).astype(np.uint8)
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, nt, T))
    d = dict(ok=write(root / "ok", ip, ix, et, nt, node_type=nt, num_node_type=T), nt=nt, ip=ip, ix=ix, et=et)
    d["plain"] = write(root / "plain", ip, ix, et, nt)  # typed edges, no node types at all
    for name in ("missing", "short", "over", "no_meta"):
        d[name] = str(root / name)
        shutil.copytree(d["ok"], d[name])
    os.remove(os.path.join(d["missing"], "node_type.bin"))
    nt[:-1].tofile(os.path.join(d["short"], "node_type.bin"))
    bad = nt.copy()
    bad[17] = T
    bad.tofile(os.path.join(d["over"], "node_type.bin"))
    meta = open(os.path.join(d["ok"], "meta.txt")).read()
    open(os.path.join(d["no_meta"], "meta.txt"), "w").write(meta.replace(f"NUM_NODE_TYPE\t{T}\n", ""))
    # two signatures: one node changes its type, the relations of its edges stay what they were
    d["two"] = str(root / "two")
    shutil.copytree(d["ok"], d["two"])
    v = int(np.flatnonzero(np.diff(ip.astype(np.int64)) > 0)[5])
    flipped = nt.copy()
    flipped[v] = (nt[v] + 1) % T
    flipped.tofile(os.path.join(d["two"], "node_type.bin"))
    d["flipped"] = v
    return d


ACCEPTED = [
    ("on", ON),
    ("off-elsewhere", dict(hetero_batch="off", _arch=3, trainer_ctx="cuda:1")),  # off: nothing is asked for
    ("hashed-two-pipelines", dict(ON, hash_table="hashed", pipelines=2, lookahead=2)),
    ("link", dict(ON, task="link_prediction", num_negative=2)),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(datasets, case):
    out = run_config(datasets["ok"], case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


def test_the_relation_table_is_derived_at_load(datasets):
    tail = "print('table', sam.num_node_type(), [(sam.relation_src_type(r), sam.relation_dst_type(r)) for r in range(9)])"
    out = run_config(datasets["ok"], ON, tail=tail, env_extra=INFO)
    assert out.returncode == 0, out.stderr[-2000:]
    present = set(np.unique(datasets["et"]).tolist())
    want = [(r % T, r // T) if r in present else (255, 255) for r in range(T * T)]
    assert f"table {T} {want}" in out.stdout, out.stdout
    assert "hetero_batch: 3 node types, 9 relations" in out.stderr and "took" in out.stderr


REFUSED = [
    ("arch0", dict(ARCH0, **ON), ["arch0", "is not built"]),
    ("arch3", dict(ON, _arch=3, trainer_ctx="cuda:1"), ["arch3", "is not built"]),
    ("arch4", dict(ON, _arch=4, sampler_ctx="cuda:1"), ["arch4", "is not built"]),
    ("arch5", dict(ON, _arch=5, num_sample_worker=1, num_train_worker=1), ["arch5", "is not built"]),
    ("arch6", dict(ON, _arch=6, num_worker=1), ["arch6", "is not built"]),
    ("khop0", dict(hetero_batch="on"), ["hetero_batch with _sample_type 0 is not built", "khop_typed"]),
    ("khop3", dict(hetero_batch="on", _sample_type=7), ["hetero_batch with _sample_type 7 is not built", "khop_typed"]),
    ("khop_labor", dict(hetero_batch="on", _sample_type=8), ["hetero_batch with _sample_type 8 is not built"]),
    ("edge_feat", dict(ON, edge_feat="on"), ["hetero_batch with edge_feat is not built"]),
    ("induced", dict(ON, induced_subgraph="on"), ["hetero_batch with induced_subgraph is not built"]),
    ("learnable", dict(ON, feat_learnable="sgd", feat_lr=0.1), ["hetero_batch with feat_learnable is not built"]),
    ("dist-graph", dict(ON, use_dist_graph=0.5), ["use_dist_graph", "ONE CSR"]),
    ("bad-value", dict(TYPED, hetero_batch="yes"), ["hetero_batch = yes", "on or off"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, extra, words = case
    out = run_config(datasets["ok"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])
    if case[0] not in ("dist-graph", "bad-value"):  # (khop_typed itself refuses a sharded graph first)
        assert "hetero_batch" in out.stderr


BAD_DATA = [
    ("missing", ["hetero_batch", "node_type.bin is missing"]),
    ("short", ["hetero_batch: node_type.bin has 599 bytes, NUM_NODE is 600"]),
    ("over", ["hetero_batch: node_type.bin: node 17 has the type 3, NUM_NODE_TYPE is 3"]),
    ("no_meta", ["hetero_batch: meta.txt lacks NUM_NODE_TYPE"]),
    ("plain", ["hetero_batch: meta.txt lacks NUM_NODE_TYPE"]),
]


@pytest.mark.parametrize("case", BAD_DATA, ids=[c[0] for c in BAD_DATA])
def test_node_types_that_are_wrong_are_fatal_by_name(datasets, case):
    out = run_config(datasets[case[0]], ON)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]
    for w in case[1]:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_a_relation_with_two_signatures_is_named_with_both(datasets):
    out = run_config(datasets["two"], ON)
    assert out.returncode < 0 and "configured" not in out.stdout
    assert "hetero_batch: relation " in out.stderr and "has two signatures: (source type " in out.stderr, out.stderr[-2000:]
    assert "and (source type " in out.stderr and "destination type " in out.stderr


@pytest.mark.parametrize("name", ["ok", "two", "over", "missing"])
def test_without_the_key_node_types_are_not_looked_at(datasets, name):
    """A khop_typed run on a dataset that carries node types -- right, wrong or none -- is what it was."""
    out = run_config(datasets[name], TYPED, env_extra=INFO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"] and "hetero_batch" not in out.stderr


@pytest.mark.parametrize("getter", sorted(GETTERS))
def test_without_the_key_every_accessor_dies_by_name(datasets, getter):
    out = run_config(datasets["ok"], TYPED, tail=f"sam.{getter}({GETTERS[getter]})")
    assert out.returncode < 0  # (the configuration was taken: the accessor is what dies)
    assert f"samgraph_{getter} needs the config key hetero_batch = on" in out.stderr, out.stderr[-2000:]
