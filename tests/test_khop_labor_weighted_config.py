"""khop_labor_weighted on the host: the names, the twin's variate at the ends of the hash range, every refusal of the C
ABI before a device call, and which configurations config + data_init take -- every refusal by name, a bad weight by its
position."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import khop_labor_weighted_ref as ref
from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen
from xgnn_amd._lib import Graph, HashTable, lib

INVALID = -1  # GGMS_ERR_INVALID
P = C.c_void_p(1 << 20)  # never dereferenced: the checks come first


def test_names():
    import samgraph.torch as sam
    from xgnn_amd import common, ops
    assert sam.kKHopLaborWeighted == common.kKHopLaborWeighted == ops.KHOP_LABOR_WEIGHTED == 11
    assert sam.sample_types["khop_labor_weighted"] == 11


def test_variate_is_positive_and_strictly_decreasing():
    E = ref.variate(np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint64)).astype(object)
    assert E[0] == 33 << 32 and E[-1] == 1  # log2(1) = 0; v = 2^33 - 1 falls one unit short of 33
    assert all(a > b for a, b in zip(E, E[1:]))


def graph(num_part=0):
    g = Graph()
    g.indptr, g.indices, g.num_node, g.num_part = 1 << 20, 1 << 21, 100, num_part
    return g


def leaf(g, weight=P, fanout=5, ws_bytes=1 << 30):
    return lib().ggms_sample_khop_labor_weighted(C.byref(g), weight, P, 10, fanout, 7, P, P, P, P, P, ws_bytes, None)


@pytest.mark.parametrize("bad", [dict(fanout=128), dict(fanout=0), dict(weight=None), dict(ws_bytes=8)],
                         ids=["fanout-128", "fanout-0", "null-weight", "short-workspace"])
def test_leaf_refuses(bad):
    assert leaf(graph(), **bad) == INVALID and "invalid argument" in lib().ggms_last_error().decode()


def test_leaf_and_batch_refuse_a_sharded_graph():
    g = graph(num_part=2)
    assert leaf(g) == INVALID
    f = (C.c_size_t * 2)(5, 4)
    ptrs = (C.c_void_p * 2)(1 << 20, 1 << 20)
    ht = HashTable()
    ht.n2o_size = 1 << 30
    assert lib().ggms_sample_batch_labor_weighted(C.byref(g), P, 10, f, 2, C.byref(ht), ptrs, ptrs, ptrs, P, P, None, P,
                                                  1 << 40, None) == INVALID
    g = graph()
    assert lib().ggms_sample_batch_labor_weighted(C.byref(g), P, 10, f, 2, C.byref(ht), ptrs, ptrs, ptrs, P, None, None,
                                                  P, 1 << 40, None) == INVALID  # null weights


def test_the_generic_batch_call_names_the_new_one():
    f = (C.c_size_t * 2)(5, 4)
    ptrs = (C.c_void_p * 2)(1 << 20, 1 << 20)
    ht, g = HashTable(), graph()
    assert lib().ggms_sample_batch(11, C.byref(g), P, 10, f, 2, C.byref(ht), None, 0, ptrs, ptrs, P, None, P, 1 << 40,
                                   None) == INVALID
    assert "ggms_sample_batch_labor_weighted" in lib().ggms_last_error().decode()


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """ok; none (no file); short (4 bytes more); nan / small (position 17 holds a NaN / 2^-41)."""
    root = tmp_path_factory.mktemp("labor_weighted_cfg")
    ip, ix = powerlaw_csr(300, mean_deg=6, seed=1)
    w = np.exp2(np.random.RandomState(0).uniform(-8, 8, ix.size)).astype(np.float32)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 300, 3, dtype=np.uint32), meta=dict(feat_dim=8, num_class=5))
    datagen.write_dataset(str(root / "ok"), g, feat=feature_rows(np.arange(300), 8), label=np.arange(300) % 5, edge_weight=w)
    np.testing.assert_array_equal(np.fromfile(str(root / "ok" / "edge_weight.bin"), np.float32), w)
    assert not (root / "ok" / "prob_table.bin").exists()
    for name in ("none", "short", "nan", "small"):
        shutil.copytree(root / "ok", root / name)
    os.remove(root / "none" / "edge_weight.bin")
    with open(root / "short" / "edge_weight.bin", "ab") as f:
        f.write(b"\0" * 4)
    for name, bad in (("nan", np.nan), ("small", 2.0 ** -41)):
        v = w.copy()
        v[17] = bad
        v.tofile(str(root / name / "edge_weight.bin"))
    return {name: str(root / name) for name in ("ok", "none", "short", "nan", "small")}


@pytest.mark.parametrize("extra", [dict(), dict(task="link_prediction", pipelines=2, hash_table="hashed", edge_feat="off")],
                         ids=["plain", "link-hashed-pipelines"])
def test_accepted(datasets, extra):
    out = run_config(datasets["ok"], dict(extra, _sample_type=11))
    assert out.returncode == 0 and out.stdout.split() == ["configured", "5", "8"], out.stderr[-2000:]


W11 = dict(_sample_type=11)
REFUSED = [
    ("no-file", "none", W11, ["khop_labor_weighted", "edge_weight.bin is missing"]),
    ("wrong-size", "short", W11, ["edge_weight.bin has", "NUM_EDGE x 4"]),
    ("nan", "nan", W11, ["edge_weight.bin: position 17 holds", "[2^-40, 2^40]"]),
    ("out-of-range", "small", W11, ["edge_weight.bin: position 17 holds", "[2^-40, 2^40]"]),
    ("arch0", "ok", dict(W11, **ARCH0), ["arch0", "khop_labor_weighted"]),
    ("arch3", "ok", dict(W11, _arch=3, trainer_ctx="cuda:1"), ["arch3", "khop_labor_weighted", "arch1's sampling chain"]),
    ("dist-graph", "ok", dict(W11, use_dist_graph=0.5), ["khop_labor_weighted", "use_dist_graph", "ONE CSR"]),
    ("induced", "ok", dict(W11, induced_subgraph="on"), ["khop_labor_weighted", "induced_subgraph"]),
    ("hetero", "ok", dict(W11, hetero_batch="on"), ["hetero_batch", "_sample_type 11"]),
    ("inline-heads", "ok", dict(W11, inline_heads=1), ["khop_labor_weighted", "inline_heads = 1"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])
