"""typed_feat through the engine (arch1, khop_typed + hetero_batch, both tasks, 1 and 2 pipelines): the dataset has T = 3
node types with the tables (16 x F32, none, 40 x F16), written once with the types shuffled over the node ids (the engine
uploads a rank table) and once with the types contiguous (it does not: row = node - the type's first id).  For every batch
and type, get_graph_feat_of_type is table_t[rank[typed_nodes_t]] bit for bit, with the type's shape and dtype, a view of
one buffer at the definition's offsets (checked in tests/typed_feat_driver.py); feat_out_dtype = f32 widens the F16 type
exactly; the twin run with typed_feat = off delivers the same typed nodes, relation blocks, labels, pair ids and counts; and
get_graph_feat dies by name with the key on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import feat_formats as ff
import typed_feat_ref as ref
from engine_harness import batch_keys, same_batches
from feat_formats import F16, F32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "typed_feat_driver.py")
NODES, HUB_DEG, BATCH, K, SEED, T = 1500, 1100, 64, 2, 21, 3
R = T * T
TYPE_FANOUT = [[2, 1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1, 0]]  # by layer id
FANOUT = [sum(row) for row in TYPE_FANOUT]
L = len(FANOUT)
SPECS = [(16, F32), None, (40, F16)]


def make_dataset(path, contiguous):
    from xgnn_amd import datagen
    rng = np.random.RandomState(9)
    deg = rng.randint(4, 41, NODES)
    deg[0] = HUB_DEG
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = rng.randint(0, NODES, int(ip[-1])).astype(np.uint32)
    nt = rng.choice(T, NODES, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    if contiguous:
        nt.sort()
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, nt, T))
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, NODES, 5, dtype=np.uint32), meta=dict(feat_dim=4, num_class=13))
    edges = np.random.RandomState(3).permutation(ix.size)[:5 * BATCH].astype(np.uint32)
    rank = np.zeros(NODES, np.int64)
    tables, node_feat = [], []
    for t, spec in enumerate(SPECS):
        at = np.flatnonzero(nt == t)
        rank[at] = np.arange(at.size)
        if spec is None:
            tables.append(None)
            node_feat.append(None)
            continue
        bits = ref.hashed_bits(t, at.size, spec[0], spec[1])  # aperiodic: a row of the wrong type, rank or column shows
        bits[np.isnan(ff.to_f32(bits, spec[1]))] = 0  # (the host reader compares values of the F32 table nowhere; bits only)
        tables.append(bits)
        node_feat.append(bits.view(np.float32 if spec[1] == F32 else np.float16))
    datagen.write_dataset(path, g, feat=np.zeros((NODES, 4), np.float32), label=(np.arange(NODES) * 7) % 13,
                          train_edges=edges, edge_type=et, num_edge_type=R, node_type=nt, num_node_type=T,
                          node_feat=node_feat)
    return dict(path=path, nt=nt, rank=rank, tables=tables)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return {c: make_dataset(str(tmp_path_factory.mktemp("typed_feat_" + ("contig" if c else "shuffled"))), c)
            for c in (False, True)}


def drive(d, prefix, args, ok=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    env["SAMGRAPH_LOG_LEVEL"] = "info"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz"), r.stderr


def args_of(task, pipes=1, **keys):
    a = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=" + " ".join(map(str, FANOUT)), "num_epoch=1",
         "sample_type=khop_typed", f"pipelines={pipes}", "lookahead=2", f"task={task}", "hetero_batch=on",
         "type_fanout=" + "/".join(",".join(map(str, row)) for row in TYPE_FANOUT)]
    if task == "link_prediction":
        a.append(f"num_negative={K}")
    return a + [f"{k}={v}" for k, v in keys.items()]


def shared_names(task):
    names = ["input_nodes", "output_nodes", "label", "ntype", "local", "slot"]
    for i in range(L):
        names += [f"row{i}", f"col{i}", f"num_src{i}", f"num_dst{i}", f"eid{i}", f"etype{i}"]
        names += [f"rel_{w}{i}_{r}" for w in ("row", "col", "eid") for r in range(R)]
    for t in range(T):
        names += [f"typed{t}", f"src_of{t}", f"dst_of{t}"]
    if task == "link_prediction":
        names += ["seed_ids", "pos_src", "pos_dst", "neg_src", "neg_dst", "link_edge_ids"]
    return names


def check_rows(got, d, out_dts):
    """every batch, every type: the block is table_t[rank[typed_nodes_t]] delivered in out_dts[t]"""
    rows_seen = 0
    for key in batch_keys(got):
        total = 0
        for t, spec in enumerate(SPECS):
            nodes = got[f"{key}:typed{t}"].view(np.uint32)
            feat = got[f"{key}:feat{t}"]
            assert (d["nt"][nodes] == t).all()
            if spec is None:
                assert feat.shape == (nodes.size, 0) and str(got[f"{key}:feat_dtype{t}"]) == "none"
                continue
            dim, src = spec
            out = out_dts[t]
            assert int(got[f"{key}:feat_dim{t}"]) == dim and str(got[f"{key}:feat_dtype{t}"]) == ff.TORCH_NAME[out]
            want = d["tables"][t][d["rank"][nodes]]
            if out != src:
                want = ff.convert_bits(np.ascontiguousarray(want), src, out)
            np.testing.assert_array_equal(feat.view(ff.BITS[out]), want, err_msg=f"batch {key} type {t}")
            rows_seen += nodes.size
            total += nodes.size * dim * ref.ES[out]
        assert float(got[f"{key}:feature_bytes"]) >= total  # the end of the last block: the rows and at most 15 pad bytes each
        assert float(got[f"{key}:feature_bytes"]) < total + 16 * T
    assert rows_seen > 1000


#        contiguous  task                  pipelines
CASES = [(False, "node_classification", 1), (False, "link_prediction", 2),
         (True, "node_classification", 2), (True, "link_prediction", 1)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_every_type_arrives_from_its_own_table(datasets, tmp_path, case):
    contiguous, task, pipes = case
    d = datasets[contiguous]
    got, err = drive(d, str(tmp_path / "on"), args_of(task, pipes, typed_feat="on"))
    assert ("no rank table" in err) == contiguous and ("a rank table of 4 x NUM_NODE = 6000 bytes" in err) != contiguous, err[-2000:]
    assert "typed_feat: 3 tables" in err
    check_rows(got, d, [F32, None, F16])
    twin, _ = drive(d, str(tmp_path / "off"), args_of(task, pipes, typed_feat="off"))
    same_batches(got, twin, shared_names(task))  # typed nodes, relation blocks, labels, pair ids, counts: bit for bit
    assert not any(":feat_dtype" in k for k in twin.files) and any(k.endswith(":feat") for k in twin.files)


@pytest.mark.parametrize("contiguous", [False, True])
def test_feat_out_dtype_widens_the_f16_type_exactly(datasets, tmp_path, contiguous):
    got, _ = drive(datasets[contiguous], str(tmp_path / "f32"), args_of("node_classification", 1, typed_feat="on", feat_out_dtype="f32"))
    check_rows(got, datasets[contiguous], [F32, None, F32])


def test_get_graph_feat_dies_by_name_with_the_key_on(datasets, tmp_path):
    r = drive(datasets[False], str(tmp_path / "probe"), args_of("node_classification", 1, typed_feat="on") + ["probe=get_graph_feat"],
              ok=False)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "probe") + ".w0.npz")
    assert "samgraph_get_graph_feat with typed_feat = on: there is no single feature matrix" in r.stderr, r.stderr[-2000:]
