"""task = link_prediction through the engine (arch1): every epoch hands out the train edge set once, every batch's
negatives are the numpy replay (tests/link_ref.py) with the salt of the batch's key, the pair ids lead back to the global
endpoints and to their feature rows -- whatever the number of pipelines -- and a run without the key is untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import link_ref as ref
from engine_harness import batch_keys, same_batches
from graphgen import exact_features, powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "link_driver.py")
SEED, EPOCHS, BATCH, K, NUM_NODE, NUM_EDGE_SET = 42, 2, 64, 3, 2000, 700
COMMON = [f"seed={SEED}", f"batch_size={BATCH}", "fanout=5 4", f"num_epoch={EPOCHS}"]
LINK = COMMON + ["task=link_prediction", f"num_negative={K}"]


def write(path, train_edges):
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(NUM_NODE, mean_deg=15, seed=5)
    train = np.random.RandomState(5).permutation(NUM_NODE)[:500].astype(np.uint32)
    feat = exact_features(NUM_NODE, 20, np.float32)
    label = (np.arange(NUM_NODE, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=20, num_class=13))
    edges = np.random.RandomState(6).permutation(ix.size)[:NUM_EDGE_SET].astype(np.uint32) if train_edges else None
    datagen.write_dataset(str(path), g, feat=feat, label=label, train_edges=edges)
    return dict(ip=ip, ix=ix, feat=feat, edges=edges, path=str(path))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = write(tmp_path_factory.mktemp("link_engine_ds"), True)
    assert os.path.getsize(os.path.join(d["path"], "train_edge_set.bin")) == 4 * NUM_EDGE_SET
    return d


def drive(d, prefix, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


@pytest.fixture(scope="module")
def link_run(dataset, tmp_path_factory):
    return drive(dataset, str(tmp_path_factory.mktemp("link_run") / "out"), LINK)


def endpoints_of(npz, key):
    """(B, the batch's B (2 + K) output nodes): sources, destinations, negatives."""
    out = npz[f"{key}:output_nodes"].view(np.uint32)
    B = out.size // (2 + K)
    assert out.size == B * (2 + K)
    return B, out


def check_epoch_cover(d, npz, edge_set, steps):
    """Every epoch hands out the edge set once: a batch's positives are recovered from its sources and destinations
    through the CSR (multi-edges of the set share endpoints: any of them not yet taken)."""
    ip, ix = d["ip"], d["ix"]
    keys = batch_keys(npz)
    assert int(npz["steps_per_epoch"]) == steps == (edge_set.size + BATCH - 1) // BATCH
    assert keys == list(range(EPOCHS * steps))
    orders = []
    for epoch in range(EPOCHS):
        left = {}
        for e in edge_set.tolist():
            u, v = ref.edge_endpoints(ip, ix, e)
            left.setdefault((u, v), []).append(e)
        taken = []
        for key in range(epoch * steps, (epoch + 1) * steps):
            B, out = endpoints_of(npz, key)
            assert B == (BATCH if key % steps < steps - 1 else edge_set.size - BATCH * (steps - 1))
            for u, v in zip(out[:B].tolist(), out[B:2 * B].tolist()):
                assert left.get((u, v)), f"batch {key}: ({u}, {v}) is not an edge of the set still to be handed out"
                taken.append(left[(u, v)].pop())
        assert sorted(taken) == sorted(edge_set.tolist())  # a permutation of the set
        orders.append(taken)
    assert orders[0] != orders[1]  # reshuffled
    return orders


def test_epochs_are_permutations_and_negatives_are_the_replay(dataset, link_run):
    d, npz = dataset, link_run
    ip, ix = d["ip"], d["ix"]
    steps = (NUM_EDGE_SET + BATCH - 1) // BATCH
    assert int(npz["num_negative"]) == K
    check_epoch_cover(d, npz, d["edges"], steps)
    for key in batch_keys(npz):
        out = npz[f"{key}:output_nodes"].view(np.uint32)
        B = out.size // (2 + K)
        salt = ref.engine_salt(SEED, key // steps, key % steps)
        # the edge id of a positive: among the positions of (u, v) in the set, the one whose negatives these are
        # (multi-edges share endpoints, not variates)
        for i in range(B):
            u, v = int(out[i]), int(out[B + i])
            cands = [e for e in range(int(ip[u]), int(ip[u + 1])) if ix[e] == v]
            got = out[2 * B + i * K: 2 * B + (i + 1) * K].tolist()
            assert any(ref.negatives(ip, ix, e, K, ref.EXCLUDE, salt)[0].tolist() == got for e in cands), (key, i)


def test_pairs_lead_to_the_global_endpoints_and_their_rows(dataset, link_run):
    d, npz = dataset, link_run
    for key in batch_keys(npz):
        out = npz[f"{key}:output_nodes"].view(np.uint32)
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        B = out.size // (2 + K)
        src, dst, neg = ref.split(out, K)
        ids = npz[f"{key}:seed_ids"].view(np.uint32)
        np.testing.assert_array_equal(ids, ref.first_occurrence_ranks(out)[0])
        np.testing.assert_array_equal(nodes[npz[f"{key}:pos_src"].view(np.uint32)], src)
        np.testing.assert_array_equal(nodes[npz[f"{key}:pos_dst"].view(np.uint32)], dst)
        np.testing.assert_array_equal(nodes[npz[f"{key}:neg_dst"].view(np.uint32)], neg)
        np.testing.assert_array_equal(nodes[npz[f"{key}:neg_src"].view(np.uint32)], np.repeat(src[:, None], K, 1))
        assert npz[f"{key}:neg_dst"].shape == (B, K)
        # feature rows of pos_src are the table's rows of the global sources; the first layer's col uses the same ids
        np.testing.assert_array_equal(npz[f"{key}:feat"][npz[f"{key}:pos_src"].view(np.uint32)], d["feat"][src])
        assert int(npz[f"{key}:num_dst1"]) == out.size and set(npz[f"{key}:col1"].tolist()) <= set(ids.tolist())
        assert npz[f"{key}:label"].size == out.size


def test_batches_do_not_depend_on_the_pipelines(dataset, link_run, tmp_path):
    two = drive(dataset, str(tmp_path / "out"), LINK + ["pipelines=2", "lookahead=2"])
    same_batches(two, link_run, ["input_nodes", "output_nodes", "row0", "col0", "row1", "col1", "seed_ids", "pos_src",
                                 "pos_dst", "neg_src", "neg_dst", "feat"])


def test_without_the_file_every_edge_is_covered(tmp_path):
    d = write(tmp_path / "ds", False)
    assert not os.path.exists(os.path.join(d["path"], "train_edge_set.bin"))
    E = d["ix"].size
    npz = drive(d, str(tmp_path / "out"), [f"seed={SEED}", "batch_size=4096", "fanout=2 2", f"num_epoch={EPOCHS}",
                                           "task=link_prediction", f"num_negative={K}", "negative_mode=uniform"])
    steps = (E + 4095) // 4096
    assert int(npz["steps_per_epoch"]) == steps and batch_keys(npz) == list(range(EPOCHS * steps))
    for epoch in range(EPOCHS):
        pairs = []
        for key in range(epoch * steps, (epoch + 1) * steps):
            out = npz[f"{key}:output_nodes"].view(np.uint32)
            B = out.size // (2 + K)
            pairs += list(zip(out[:B].tolist(), out[B:2 * B].tolist()))
        src = np.repeat(np.arange(NUM_NODE), np.diff(d["ip"].astype(np.int64)))
        assert sorted(pairs) == sorted(zip(src.tolist(), d["ix"].tolist()))  # every edge once, multi-edges included


def test_default_task_is_untouched(dataset, tmp_path):
    """No `task` key and task = node_classification give the same batches, byte for byte: the node-classification batches
    of the train set (the dataset's train_edge_set.bin is not looked at)."""
    plain = drive(dataset, str(tmp_path / "plain"), COMMON)
    named = drive(dataset, str(tmp_path / "named"), COMMON + ["task=node_classification"])
    same_batches(named, plain, ["input_nodes", "output_nodes", "label", "row0", "col0", "row1", "col1", "feat"])
    assert int(plain["num_negative"]) == 0 and int(plain["steps_per_epoch"]) == (500 + BATCH - 1) // BATCH
    for key in batch_keys(plain):
        assert plain[f"{key}:output_nodes"].size <= BATCH
