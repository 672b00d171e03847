"""Config keys edge_ids / edge_feat on the host: datagen's edge table round trip, which configurations config + data_init
take (no GPU touched) and every refusal, by name."""
import os
import shutil

import numpy as np
import pytest

from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen

DIM = 3


def write(path, edge_feat=True, dtype=np.float32, name="F32", dim=DIM):
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    train = np.arange(0, 600, 3, dtype=np.uint32)
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=20, num_class=13))
    table = feature_rows(np.arange(ix.size), dim, dtype) if edge_feat else None
    datagen.write_dataset(str(path), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13,
                          weights=np.ones(ix.size, np.float32), edge_feat=table, edge_feat_dtype=name)
    return dict(path=str(path), ip=ip, ix=ix, table=table)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("edge_cfg")
    d = dict(f32=write(root / "f32"), f16=write(root / "f16", dtype=np.float16, name="F16", dim=8), none=write(root / "none", False))
    # a table of the wrong size, no meta key, a row-scaled table: copies of the F32 dataset with one thing changed
    for name in ("short", "nokey", "q8row"):
        shutil.copytree(d["f32"]["path"], root / name)
        d[name] = dict(path=str(root / name))
    with open(root / "short" / "edge_feat.bin", "ab") as f:
        f.write(b"\0" * 4)
    for name, drop, add in (("nokey", "EDGE_FEAT_DIM", ""), ("q8row", "EDGE_FEAT_DATA_TYPE", "EDGE_FEAT_DATA_TYPE\tQ8ROW\n")):
        lines = [ln for ln in open(root / name / "meta.txt") if not ln.startswith(drop)]
        open(root / name / "meta.txt", "w").write("".join(lines) + add)
    return d


def test_write_dataset_round_trip(datasets):
    for key, dim, dt, name in (("f32", DIM, np.float32, "F32"), ("f16", 8, np.float16, "F16")):
        d = datasets[key]
        meta = dict(ln.split() for ln in open(os.path.join(d["path"], "meta.txt")))
        assert meta["EDGE_FEAT_DIM"] == str(dim) and meta["EDGE_FEAT_DATA_TYPE"] == name
        assert int(meta["NUM_EDGE"]) == d["ix"].size
        f = os.path.join(d["path"], "edge_feat.bin")
        assert os.path.getsize(f) == d["ix"].size * dim * np.dtype(dt).itemsize
        np.testing.assert_array_equal(np.fromfile(f, dt).reshape(-1, dim), d["table"])
    meta = open(os.path.join(datasets["none"]["path"], "meta.txt")).read()
    assert "EDGE_FEAT" not in meta and not os.path.exists(os.path.join(datasets["none"]["path"], "edge_feat.bin"))


def test_a_one_dimensional_table_is_dim_1(tmp_path):
    ip, ix = powerlaw_csr(50, mean_deg=4, seed=1)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(10, dtype=np.uint32), meta=dict(feat_dim=4, num_class=2))
    datagen.write_dataset(str(tmp_path), g, edge_feat=np.arange(ix.size, dtype=np.float32), minimal=True)
    assert "EDGE_FEAT_DIM\t1\n" in open(tmp_path / "meta.txt").read()
    assert os.path.getsize(tmp_path / "edge_feat.bin") == 4 * ix.size
    with pytest.raises(AssertionError, match="one row per edge"):
        datagen.write_dataset(str(tmp_path), g, edge_feat=np.zeros((ix.size + 1, 2), np.float32), minimal=True)


ACCEPTED = [
    ("edge_ids", "none", dict(edge_ids="on")),
    ("edge_ids-off", "none", dict(edge_ids="off", _arch=3, trainer_ctx="cuda:1")),  # off: nothing is asked for
    ("edge_feat", "f32", dict(edge_feat="on")),
    ("edge_feat-f16", "f16", dict(edge_feat="on", edge_ids="on")),
    ("edge_feat-khop3", "f32", dict(edge_feat="on", _sample_type=7)),
    ("edge_ids-weighted", "f32", dict(edge_ids="on", _sample_type=2)),
    ("edge_feat-link", "f32", dict(edge_feat="on", task="link_prediction", exclude_seed_edges="both")),
    ("no-keys-with-a-table", "f32", {}),  # the meta keys are read, the table is not
    ("no-keys-q8row-meta", "q8row", {}),
    ("edge_ids-q8row-meta", "q8row", dict(edge_ids="on")),  # ids need no table
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(datasets, case):
    _, ds, extra = case
    out = run_config(datasets[ds]["path"], extra)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("arch0", "f32", dict(ARCH0, edge_ids="on"), ["arch0", "edge_ids"]),
    ("arch3", "f32", dict(_arch=3, trainer_ctx="cuda:1", edge_ids="on"), ["arch3", "edge_ids"]),
    ("arch4", "f32", dict(_arch=4, sampler_ctx="cuda:1", edge_feat="on"), ["arch4", "edge_feat"]),
    ("arch5", "f32", dict(_arch=5, num_sample_worker=1, num_train_worker=1, edge_ids="on"), ["arch5", "edge_ids"]),
    ("arch6", "f32", dict(_arch=6, num_worker=1, edge_feat="on"), ["arch6", "edge_feat"]),
    ("dist-graph", "f32", dict(use_dist_graph=0.5, edge_ids="on"), ["edge_ids", "use_dist_graph", "ONE CSR"]),
    ("random-walk", "f32", dict(_sample_type=3, random_walk_length=3, random_walk_restart_prob=0.5, num_random_walk=4,
                                num_neighbor=5, edge_ids="on"), ["edge_ids", "random_walk", "not edges of the graph"]),
    ("khop2", "f32", dict(_sample_type=5, edge_feat="on"), ["edge_feat", "khop2", "permutes indices"]),
    ("bad-value", "f32", dict(edge_ids="yes"), ["edge_ids = yes", "on or off"]),
    ("bad-value-feat", "f32", dict(edge_feat=1), ["edge_feat = 1", "on or off"]),
    ("no-file", "none", dict(edge_feat="on"), ["edge_feat", "EDGE_FEAT_DIM"]),
    ("no-meta-key", "nokey", dict(edge_feat="on"), ["edge_feat", "meta.txt lacks EDGE_FEAT_DIM"]),
    ("wrong-size", "short", dict(edge_feat="on"), ["edge_feat.bin has", "NUM_EDGE x"]),
    ("q8row", "q8row", dict(edge_feat="on"), ["edge_feat", "Q8ROW", "plain gather"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds]["path"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_a_missing_file_is_named(datasets, tmp_path):
    shutil.copytree(datasets["f32"]["path"], tmp_path / "d")
    os.remove(tmp_path / "d" / "edge_feat.bin")
    out = run_config(str(tmp_path / "d"), dict(edge_feat="on"))
    assert out.returncode < 0 and "edge_feat.bin is missing" in out.stderr, out.stderr[-2000:]
