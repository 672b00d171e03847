"""sample_type khop_typed on the host: which configurations config + data_init take (no GPU touched) and every refusal,
by name -- the deployments, a sharded graph, exclude_seed_edges, a type_fanout of the wrong length, with a value >= 128,
with a zero row or at odds with `fanout`, and an edge_type.bin that is missing, of another size, not sorted inside a
list or out of range."""
import os
import shutil

import numpy as np
import pytest

import khop_typed_ref as ref
from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen

TF = [[3, 1, 1], [2, 2, 0]]  # by layer id: config_run's fanout [5, 4] holds the rows' sums
T10 = dict(_sample_type=10, type_fanout=TF)


def test_python_names():
    import samgraph.torch as sam
    assert sam.kKHopTyped == 10 and sam.sample_types["khop_typed"] == 10
    assert callable(sam.get_graph_edge_type)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("typed_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    et = ref.sorted_types(ip, np.random.RandomState(2), 3)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(root / "ok"), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13,
                          edge_feat=feature_rows(np.arange(ix.size), 3), edge_type=et, num_edge_type=3)
    d = dict(ok=str(root / "ok"))
    for name in ("none", "short", "unsorted", "range", "nometa"):
        shutil.copytree(d["ok"], root / name)
        d[name] = str(root / name)
    os.remove(root / "none" / "edge_type.bin")
    with open(root / "short" / "edge_type.bin", "ab") as f:
        f.write(b"\0")
    deg = np.diff(ip.astype(np.int64))
    lists = [v for v in np.flatnonzero(deg >= 3) if et[ip[v]] != et[ip[v + 1] - 1]]
    v = int(lists[7])
    bad = et.copy()
    bad[ip[v]:ip[v + 1]] = bad[ip[v]:ip[v + 1]][::-1]
    bad.tofile(str(root / "unsorted" / "edge_type.bin"))
    d["unsorted_node"] = v
    w = int(lists[3])
    over = et.copy()
    over[ip[w + 1] - 1] = 3  # sorted still, but NUM_EDGE_TYPE is 3
    over.tofile(str(root / "range" / "edge_type.bin"))
    d["range_node"] = w
    meta = open(root / "nometa" / "meta.txt").read().replace("NUM_EDGE_TYPE\t3\n", "")
    open(root / "nometa" / "meta.txt", "w").write(meta)
    return d


ACCEPTED = [
    ("node-classification", dict(T10)),
    ("link-prediction-hashed-pipelines", dict(T10, task="link_prediction", hash_table="hashed", pipelines=2, num_negative=2)),
    ("edge_feat", dict(T10, edge_feat="on")),
    ("exclude-none", dict(T10, task="link_prediction", exclude_seed_edges="none", edge_ids="on")),
    ("flat-type_fanout-and-the-sums", dict(_sample_type=10, type_fanout=[3, 1, 1, 2, 2, 0], fanout=[5, 4])),
    ("khop_labor-on-the-same-data", dict(_sample_type=8, task="link_prediction", exclude_seed_edges="both")),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(datasets, case):
    out = run_config(datasets["ok"], case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


def test_the_front_end_fills_in_the_row_sums():
    """A list of lists: type_fanout travels flattened, fanout / num_fanout are the rows' sums unless given."""
    from xgnn_amd.common import SamGraphBasics

    seen = {}

    class Spy(SamGraphBasics):
        @property
        def C_LIB_CTYPES(self):
            class H:
                @staticmethod
                def samgraph_config(keys, vals, n):
                    seen.update({keys[i].decode(): vals[i].decode() for i in range(n)})
            return H
    Spy().config({"type_fanout": TF, "_sample_type": 10})
    assert seen == {"type_fanout": "3 1 1 2 2 0", "_sample_type": "10", "fanout": "5 4", "num_fanout": "2"}
    seen.clear()
    Spy().config({"type_fanout": TF, "fanout": [9, 9], "num_fanout": 2})
    assert seen["fanout"] == "9 9"  # a given fanout is passed on as it is: the engine refuses it


REFUSED = [
    ("arch0", "ok", dict(T10, **ARCH0), ["arch0", "khop_typed", "arch1's sampling chain"]),
    ("arch3", "ok", dict(T10, _arch=3, trainer_ctx="cuda:1"), ["arch3", "khop_typed", "arch1's sampling chain"]),
    ("arch4", "ok", dict(T10, _arch=4, sampler_ctx="cuda:1"), ["arch4", "khop_typed", "arch1's sampling chain"]),
    ("arch5", "ok", dict(T10, _arch=5, num_sample_worker=1, num_train_worker=1), ["arch5", "khop_typed", "arch1's sampling chain"]),
    ("arch6", "ok", dict(T10, _arch=6, num_worker=1), ["arch6", "khop_typed", "arch1's sampling chain"]),
    ("dist-graph", "ok", dict(T10, use_dist_graph=0.5), ["khop_typed", "use_dist_graph", "ONE CSR"]),
    ("exclude-self", "ok", dict(T10, task="link_prediction", exclude_seed_edges="self"),
     ["khop_typed", "exclude_seed_edges = self", "knows nothing of the position and type streams"]),
    ("exclude-both", "ok", dict(T10, task="link_prediction", exclude_seed_edges="both"),
     ["exclude_seed_edges = both", "knows nothing of the position and type streams"]),
    ("no-key", "ok", dict(_sample_type=10), ["khop_typed", "needs the config key type_fanout"]),
    ("length-not-rows", "ok", dict(_sample_type=10, type_fanout=[3, 1, 1, 2, 2]), ["type_fanout has 5 values", "num_layer (2) rows"]),
    ("length-other-R", "ok", dict(_sample_type=10, type_fanout=[3, 2, 2, 2], fanout=[5, 4]),
     ["type_fanout has 4 values", "num_layer x NUM_EDGE_TYPE is 2 x 3"]),
    ("too-many-types", "ok", dict(_sample_type=10, type_fanout=[1] * 66, fanout=[33, 33]), ["type_fanout has 66 values", "1 .. 32"]),
    ("value-128", "ok", dict(_sample_type=10, type_fanout=[[3, 128, 1], [2, 2, 0]]), ["type_fanout: the value 128", "0 (not sampled) .. 127"]),
    ("zero-row", "ok", dict(_sample_type=10, type_fanout=[3, 1, 1, 0, 0, 0], fanout=[5, 4]), ["type_fanout: row 1 is all zero"]),
    ("fanout-disagrees", "ok", dict(_sample_type=10, type_fanout=TF, fanout=[5, 5]),
     ["fanout[1] = 5 disagrees with type_fanout", "row 1 sums to 4"]),
    ("no-file", "none", dict(T10), ["khop_typed", "edge_type.bin is missing"]),
    ("wrong-size", "short", dict(T10), ["edge_type.bin has", "NUM_EDGE is"]),
    ("no-meta-key", "nometa", dict(T10), ["khop_typed", "meta.txt lacks NUM_EDGE_TYPE"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_an_unsorted_or_out_of_range_list_is_named_by_its_node(datasets):
    out = run_config(datasets["unsorted"], dict(T10))
    assert out.returncode < 0 and "configured" not in out.stdout
    assert f"the types of node {datasets['unsorted_node']}'s list are not non-decreasing" in out.stderr, out.stderr[-2000:]
    out = run_config(datasets["range"], dict(T10))
    assert out.returncode < 0 and "configured" not in out.stdout
    assert f"node {datasets['range_node']}'s list holds the type 3" in out.stderr, out.stderr[-2000:]
    assert "NUM_EDGE_TYPE is 3" in out.stderr
    # the file is only read for the sampler that needs it
    assert run_config(datasets["unsorted"], dict(_sample_type=8, task="link_prediction")).returncode == 0
