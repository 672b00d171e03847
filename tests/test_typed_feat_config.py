"""Config key typed_feat on the host: which configurations config + data_init take (no GPU touched), every refusal by
name, what is wrong with a dataset's typed tables, that a typed dataset without the key runs as before, and that the new
accessors die by name without the key."""
import os
import shutil

import numpy as np
import pytest

from config_run import run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen

torch = pytest.importorskip("torch")

T, N = 3, 600
TF = [[1] * 9, [1] * 8 + [0]]
TYPED = dict(_sample_type=10, type_fanout=TF, fanout=[9, 8])
HETERO = dict(TYPED, hetero_batch="on")
ON = dict(HETERO, typed_feat="on")
INFO = dict(SAMGRAPH_LOG_LEVEL="info")


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("typed_feat_cfg")
    ip, ix = powerlaw_csr(N, mean_deg=9, seed=2)
    nt = np.random.RandomState(1).randint(0, T, N).astype(np.uint8)
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, nt, T))
    counts = np.bincount(nt, minlength=T)
    rs = np.random.RandomState(4)
    node_feat = [rs.standard_normal((counts[0], 16)).astype(np.float32), None,
                 torch.from_numpy(rs.standard_normal((counts[2], 40)).astype(np.float32)).to(torch.bfloat16)]
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, N, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    d = dict(counts=counts, ok=str(root / "ok"))
    datagen.write_dataset(d["ok"], g, feat=feature_rows(np.arange(N), 20), label=np.arange(N) % 13, edge_type=et,
                          num_edge_type=T * T, node_type=nt, num_node_type=T, node_feat=node_feat)
    for name in ("no_dim", "no_dtype", "missing", "short", "long", "fp8", "f64", "sorted"):
        d[name] = str(root / name)
        shutil.copytree(d["ok"], d[name])
    meta = open(os.path.join(d["ok"], "meta.txt")).read()

    def rewrite(name, old, new):
        assert old in meta
        open(os.path.join(d[name], "meta.txt"), "w").write(meta.replace(old, new))

    rewrite("no_dim", "NODE_FEAT_DIM_1\t0\n", "")
    rewrite("no_dtype", "NODE_FEAT_DATA_TYPE_2\tBF16\n", "")
    rewrite("fp8", "NODE_FEAT_DATA_TYPE_2\tBF16\n", "NODE_FEAT_DATA_TYPE_2\tF8E4M3\n")
    rewrite("f64", "NODE_FEAT_DATA_TYPE_0\tF32\n", "NODE_FEAT_DATA_TYPE_0\tF64\n")
    os.remove(os.path.join(d["missing"], "node_feat_2.bin"))
    raw = np.fromfile(os.path.join(d["ok"], "node_feat_0.bin"), np.uint8)
    raw[:-4].tofile(os.path.join(d["short"], "node_feat_0.bin"))
    np.concatenate([raw, raw[:64]]).tofile(os.path.join(d["long"], "node_feat_0.bin"))
    # the same tables over contiguous types: relations re-derived, no rank table
    snt = np.sort(nt)
    six, set_, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, snt, T))
    datagen.write_dataset(d["sorted"], g | dict(indices=six), feat=feature_rows(np.arange(N), 20), label=np.arange(N) % 13,
                          edge_type=set_, num_edge_type=T * T, node_type=snt, num_node_type=T, node_feat=node_feat)
    return d


ACCEPTED = [
    ("on", ON),
    ("off", dict(HETERO, typed_feat="off")),
    ("two-pipelines-link", dict(ON, pipelines=2, lookahead=2, task="link_prediction", num_negative=2)),
    ("out-dtype", dict(ON, feat_out_dtype="f32")),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(datasets, case):
    out = run_config(datasets["ok"], case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


def test_what_the_load_says_and_what_the_accessors_return(datasets):
    tail = "print('types', [(sam.feat_dim_of_type(t), str(sam.feat_dtype_of_type(t))) for t in range(3)])"
    out = run_config(datasets["ok"], ON, tail=tail, env_extra=INFO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "types [(16, 'torch.float32'), (0, 'torch.float32'), (40, 'torch.bfloat16')]" in out.stdout, out.stdout
    nbytes = int(datasets["counts"][0]) * 64 + int(datasets["counts"][2]) * 80
    assert f"typed_feat: 3 tables, {nbytes} bytes of HBM; a rank table of 4 x NUM_NODE = 2400 bytes is uploaded" in out.stderr
    out = run_config(datasets["sorted"], dict(ON, feat_out_dtype="f16"), tail=tail, env_extra=INFO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "types [(16, 'torch.float16'), (0, 'torch.float16'), (40, 'torch.float16')]" in out.stdout, out.stdout
    assert "node_type.bin is non-decreasing in the node id: no rank table" in out.stderr


REFUSED = [
    ("no-hetero", dict(TYPED, typed_feat="on"), {}, ["typed_feat without hetero_batch = on is not built"]),
    ("khop0", dict(typed_feat="on"), {}, ["typed_feat without hetero_batch = on is not built"]),
    ("learnable", dict(ON, feat_learnable="sgd", feat_lr=0.1), {}, ["typed_feat with feat_learnable is not built"]),
    ("store-dtype", dict(ON, feat_store_dtype="F16"), {}, ["typed_feat with feat_store_dtype is not built"]),
    ("empty-feat", ON, dict(SAMGRAPH_EMPTY_FEAT="8"), ["typed_feat with SAMGRAPH_EMPTY_FEAT is not built"]),
    ("fake-dim", ON, dict(SAMGRAPH_FAKE_FEAT_DIM="64"), ["typed_feat with SAMGRAPH_FAKE_FEAT_DIM is not built"]),
    ("bad-value", dict(HETERO, typed_feat="yes"), {}, ["typed_feat = yes", "on or off"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, extra, env, words = case
    out = run_config(datasets["ok"], extra, env_extra=env)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_bad_data_is_fatal_by_name(datasets):
    c0 = int(datasets["counts"][0])
    cases = [
        ("no_dim", ["typed_feat: meta.txt lacks NODE_FEAT_DIM_1"]),
        ("no_dtype", ["typed_feat: meta.txt lacks NODE_FEAT_DATA_TYPE_2"]),
        ("missing", ["typed_feat: ", "node_feat_2.bin is missing"]),
        ("short", [f"typed_feat: node_feat_0.bin has {c0 * 64 - 4} bytes, (nodes of type 0) x NODE_FEAT_DIM_0 x the element "
                   f"size is {c0} x 16 x 4 = {c0 * 64}"]),
        ("long", [f"typed_feat: node_feat_0.bin has {c0 * 64 + 64} bytes", f"= {c0 * 64}"]),
        ("fp8", ["typed_feat with NODE_FEAT_DATA_TYPE_2 = F8E4M3 is not built", "F32, F16 or BF16"]),
        ("f64", ["typed_feat with NODE_FEAT_DATA_TYPE_0 = F64 is not built"]),
    ]
    for name, words in cases:
        out = run_config(datasets[name], ON)
        assert out.returncode < 0 and "configured" not in out.stdout, (name, out.stderr[-2000:])
        for w in words:
            assert w in out.stderr, (name, w, out.stderr[-2000:])


@pytest.mark.parametrize("name", ["ok", "missing", "short", "fp8", "no_dim"])
def test_without_the_key_a_typed_dataset_runs_as_before(datasets, name):
    """The typed tables -- right, wrong or absent -- are not looked at; feat.bin is the table."""
    for extra in (HETERO, TYPED, {}):
        out = run_config(datasets[name], extra, env_extra=INFO)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split() == ["configured", "13", "20"] and "typed_feat" not in out.stderr


@pytest.mark.parametrize("getter", ["feat_dim_of_type", "feat_dtype_of_type"])
def test_without_the_key_the_new_accessors_die_by_name(datasets, getter):
    out = run_config(datasets["ok"], HETERO, tail=f"sam.{getter}(0)")
    assert out.returncode < 0  # (the configuration was taken: the accessor is what dies)
    assert f"samgraph_{getter} needs the config key typed_feat = on" in out.stderr, out.stderr[-2000:]
