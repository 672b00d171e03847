"""exclude_seed_edges through the engine (arch1, task = link_prediction): the layers of a `self` / `both` run are the
numpy filter (tests/link_exclude_ref.py) of the `none` run's layers with the batch's own positives, nothing else of a
batch changes, the excluded count is the reference's -- and certainly at least the batch's positives on a graph whose
lists are sampled whole -- whatever the pipelines and the sampler, and a run without the key is the `none` run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import link_exclude_ref as ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features
from test_gpu_link_engine import write as write_powerlaw

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "link_exclude_driver.py")  # tests/link_driver.py + the excluded count
LAYERS = ["row0", "col0", "row1", "col1"]
REST = ["input_nodes", "output_nodes", "feat", "label", "seed_ids", "pos_src", "pos_dst", "neg_src", "neg_dst",
        "num_src0", "num_dst0", "num_src1", "num_dst1"]
# dataset A: 300 nodes, every degree at most the fanout
A_NODES, A_BATCH, A_K = 300, 32, 2
A_ARGS = ["seed=11", f"batch_size={A_BATCH}", "fanout=8 8", "num_epoch=2", "task=link_prediction", f"num_negative={A_K}"]
# dataset B: the powerlaw graph of test_gpu_link_engine.py
B_BATCH, B_K = 64, 3
B_ARGS = ["seed=42", f"batch_size={B_BATCH}", "fanout=5 4", "num_epoch=2", "task=link_prediction", f"num_negative={B_K}"]


def drive(d, prefix, args, log=False):
    """One run of the driver: (its batches, its stderr -- with the engine's info lines if `log`)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    if log:
        env["SAMGRAPH_LOG_LEVEL"] = "info"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz"), r.stderr


def ring_with_chords():
    """A symmetric graph without multi-edges or self-loops: v -- v +- 1, v +- 2 (mod 300), chords v -- v + 150 for even
    v < 150 and v -- v + 75 for v = 0, 3, .., 72: degrees 4 to 6."""
    n = A_NODES
    nb = [{(v + 1) % n, (v - 1) % n, (v + 2) % n, (v - 2) % n} for v in range(n)]
    for v in range(0, 150, 2):
        nb[v].add(v + 150), nb[v + 150].add(v)
    for v in range(0, 75, 3):
        nb[v].add(v + 75), nb[v + 75].add(v)
    deg = np.array([len(s) for s in nb])
    assert deg.min() == 4 and deg.max() == 6 and all(v in nb[w] for v in range(n) for w in nb[v])
    rng = np.random.RandomState(2)
    lists = [rng.permutation(sorted(s)) for s in nb]  # lists in no particular order
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    return ip, np.concatenate(lists).astype(np.uint32)


@pytest.fixture(scope="module")
def ring(tmp_path_factory):
    from xgnn_amd import datagen
    path = str(tmp_path_factory.mktemp("link_exclude_ring"))
    ip, ix = ring_with_chords()
    train = np.arange(0, A_NODES, 3, dtype=np.uint32)
    feat = exact_features(A_NODES, 20, np.float32)
    label = (np.arange(A_NODES, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=20, num_class=13))
    edges = np.random.RandomState(3).permutation(ix.size)[:4 * A_BATCH].astype(np.uint32)  # 4 batches an epoch
    datagen.write_dataset(path, g, feat=feat, label=label, train_edges=edges)
    return dict(ip=ip, ix=ix, path=path)


@pytest.fixture(scope="module")
def ring_runs(ring, tmp_path_factory):
    return {mode: drive(ring, str(tmp_path_factory.mktemp(f"ring_{mode}") / "out"), A_ARGS + [f"exclude_seed_edges={mode}"],
                        log=True)
            for mode in ("none", "self", "both")}


@pytest.fixture(scope="module")
def powerlaw(tmp_path_factory):
    return write_powerlaw(tmp_path_factory.mktemp("link_exclude_powerlaw"), True)


@pytest.fixture(scope="module")
def powerlaw_none(powerlaw, tmp_path_factory):
    return drive(powerlaw, str(tmp_path_factory.mktemp("powerlaw_none") / "out"), B_ARGS + ["exclude_seed_edges=none"])[0]


def check_filtered(got, base, which):
    """Every batch of `got` is the batch of `base` with the reference's filter on its layers and nothing else changed;
    its excluded count is the reference's.  -> the excluded counts."""
    assert batch_keys(got) == batch_keys(base) and len(batch_keys(got)) >= 4
    same_batches(got, base, REST)
    counts = []
    for key in batch_keys(base):
        src, dst = base[f"{key}:pos_src"].view(np.uint32), base[f"{key}:pos_dst"].view(np.uint32)
        layers = [(base[f"{key}:row{i}"], base[f"{key}:col{i}"]) for i in range(2)]
        want, dropped = ref.drop_pair_edges(src, dst, which, layers)
        for i in range(2):
            np.testing.assert_array_equal(got[f"{key}:row{i}"].view(np.uint32), want[i][0], err_msg=f"{key}:row{i}")
            np.testing.assert_array_equal(got[f"{key}:col{i}"].view(np.uint32), want[i][1], err_msg=f"{key}:col{i}")
            # no kept edge is a positive (or a mirror)
            kept = set(zip(got[f"{key}:col{i}"].view(np.uint32).tolist(), got[f"{key}:row{i}"].view(np.uint32).tolist()))
            assert not kept & ref.pair_set(src, dst, which), f"batch {key} layer {i}"
        assert int(got[f"{key}:num_excluded"]) == sum(dropped), f"batch {key}"
        counts.append(sum(dropped))
    return counts


@pytest.mark.parametrize("mode", ["self", "both"])
def test_ring_layers_are_the_filtered_layers(ring_runs, mode):
    """Every list of the ring is sampled whole (degree <= fanout), so the first layer of every batch holds every
    positive, and its mirror: at least B edges go under `self`, at least 2 B under `both`."""
    base, _ = ring_runs["none"]
    got, log = ring_runs[mode]
    counts = check_filtered(got, base, ref.WHICH_OF[mode])
    print(f"{mode}: excluded per batch {counts}")
    for key, n in zip(batch_keys(got), counts):
        B = got[f"{key}:pos_src"].size
        assert B == A_BATCH and n >= B * (2 if mode == "both" else 1), (key, n)
    # one line per epoch, next to the forced-negatives line
    steps = int(got["steps_per_epoch"])
    for epoch in range(2):
        assert f"epoch {epoch}: {sum(counts[epoch * steps:(epoch + 1) * steps])} sampled edges excluded" in log, log[-2000:]


def test_ring_none_excludes_nothing(ring_runs):
    base, log = ring_runs["none"]
    assert all(int(base[f"{key}:num_excluded"]) == 0 for key in batch_keys(base)) and "edges excluded" not in log
    # ... although every positive is there to be excluded
    for key in batch_keys(base):
        pairs = ref.pair_set(base[f"{key}:pos_src"], base[f"{key}:pos_dst"], ref.FORWARD)
        first = set(zip(base[f"{key}:col1"].view(np.uint32).tolist(), base[f"{key}:row1"].view(np.uint32).tolist()))
        assert pairs <= first


def test_powerlaw_both(powerlaw, powerlaw_none, tmp_path):
    """Lists longer than the fanout: whether a positive is sampled is the sampler's draw -- equality only."""
    got, _ = drive(powerlaw, str(tmp_path / "out"), B_ARGS + ["exclude_seed_edges=both"])
    print("excluded per batch", check_filtered(got, powerlaw_none, 3))


def test_powerlaw_both_does_not_depend_on_the_pipelines(powerlaw, powerlaw_none, tmp_path):
    got, _ = drive(powerlaw, str(tmp_path / "out"), B_ARGS + ["exclude_seed_edges=both", "pipelines=2", "lookahead=2"])
    check_filtered(got, powerlaw_none, 3)


def test_powerlaw_both_with_khop_labor(powerlaw, tmp_path):
    labor = B_ARGS + ["sample_type=khop_labor"]
    base, _ = drive(powerlaw, str(tmp_path / "none"), labor)
    got, _ = drive(powerlaw, str(tmp_path / "both"), labor + ["exclude_seed_edges=both"])
    print("excluded per batch", check_filtered(got, base, 3))


def test_without_the_key_is_the_none_run(powerlaw, powerlaw_none, tmp_path):
    plain, _ = drive(powerlaw, str(tmp_path / "out"), B_ARGS)
    same_batches(plain, powerlaw_none, LAYERS + REST + ["num_excluded"])
