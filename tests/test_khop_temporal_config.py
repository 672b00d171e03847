"""sample_type khop_temporal on the host: which configurations config + data_init take (no GPU touched) and every
refusal, by name -- the deployments, the task, a sharded graph, exclude_seed_edges, and an edge_time.bin that is
missing, of another size or not sorted inside a list."""
import os
import shutil

import numpy as np
import pytest

import khop_temporal_ref as ref
from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen

T9 = dict(_sample_type=9, task="link_prediction")


def test_python_names():
    import samgraph.torch as sam
    assert sam.kKHopTemporal == 9 and sam.sample_types["khop_temporal"] == 9
    for name in ("get_graph_edge_time", "get_graph_node_cut", "get_graph_link_time"):
        assert callable(getattr(sam, name))


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("temporal_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    et = ref.sorted_times(ip, np.random.RandomState(2))
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(root / "ok"), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13,
                          edge_feat=feature_rows(np.arange(ix.size), 3), edge_time=et)
    d = dict(ok=str(root / "ok"))
    for name in ("none", "short", "unsorted"):
        shutil.copytree(d["ok"], root / name)
        d[name] = str(root / name)
    os.remove(root / "none" / "edge_time.bin")
    with open(root / "short" / "edge_time.bin", "ab") as f:
        f.write(b"\0" * 4)
    deg = np.diff(ip.astype(np.int64))
    v = int(np.flatnonzero(deg >= 3)[7])
    bad = et.copy()
    bad[ip[v] + 1] = bad[ip[v] + 2] + 1
    bad.tofile(str(root / "unsorted" / "edge_time.bin"))
    d["unsorted_node"] = v
    return d


ACCEPTED = [
    ("plain", dict(T9)),
    ("recent", dict(T9, temporal_pick="recent")),
    ("uniform-hashed-pipelines", dict(T9, temporal_pick="uniform", hash_table="hashed", pipelines=2, num_negative=2)),
    ("edge_feat", dict(T9, edge_feat="on")),
    ("exclude-none", dict(T9, exclude_seed_edges="none", edge_ids="on")),
    ("khop_labor-on-the-same-data", dict(_sample_type=8, task="link_prediction", exclude_seed_edges="both")),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(datasets, case):
    out = run_config(datasets["ok"], case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("arch0", "ok", dict(T9, **ARCH0), ["arch0", "khop_temporal"]),
    ("arch3", "ok", dict(T9, _arch=3, trainer_ctx="cuda:1"), ["arch3", "khop_temporal", "arch1's sampling chain"]),
    ("arch4", "ok", dict(T9, _arch=4, sampler_ctx="cuda:1"), ["arch4", "khop_temporal", "arch1's sampling chain"]),
    ("arch5", "ok", dict(T9, _arch=5, num_sample_worker=1, num_train_worker=1), ["arch5", "khop_temporal", "arch1's sampling chain"]),
    ("arch6", "ok", dict(T9, _arch=6, num_worker=1), ["arch6", "khop_temporal", "arch1's sampling chain"]),
    ("node-classification", "ok", dict(_sample_type=9), ["khop_temporal", "task = link_prediction", "node_classification"]),
    ("dist-graph", "ok", dict(T9, use_dist_graph=0.5), ["khop_temporal", "use_dist_graph", "ONE CSR"]),
    ("exclude-self", "ok", dict(T9, exclude_seed_edges="self"),
     ["exclude_seed_edges = self", "strictly-before already removes the positive, its mirror at the same time, and everything later."]),
    ("exclude-both", "ok", dict(T9, exclude_seed_edges="both"), ["exclude_seed_edges = both", "strictly-before already"]),
    ("bad-pick", "ok", dict(T9, temporal_pick="latest"), ["temporal_pick = latest", "uniform (the default) or recent"]),
    ("no-file", "none", dict(T9), ["khop_temporal", "edge_time.bin is missing"]),
    ("wrong-size", "short", dict(T9), ["edge_time.bin has", "NUM_EDGE x 4"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_an_unsorted_list_is_named_by_its_node(datasets):
    out = run_config(datasets["unsorted"], dict(T9))
    assert out.returncode < 0 and "configured" not in out.stdout
    assert f"the times of node {datasets['unsorted_node']}'s list are not non-decreasing" in out.stderr, out.stderr[-2000:]
    # the file is only read for the sampler that needs it
    assert run_config(datasets["unsorted"], dict(_sample_type=8, task="link_prediction")).returncode == 0
