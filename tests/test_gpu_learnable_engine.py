"""Config key feat_learnable through the engine (arch1): tests/learn_driver.py trains a learnable table with a
deterministic "gradient", and the run is replayed in numpy (tests/update_rows_ref.py) under the engine's ordering rule:

    a batch's rows reflect exactly the updates whose call preceded the sample_once call that enqueued the batch.

In the driver's loop (sample_once; get_next_batch; update_graph_feat) with lookahead = h, call j of sample_once enqueues
batch j + h (call 0: batches 0 .. h), so batch j is gathered from the table as updates 0 .. j-h-1 left it; h = 0 is the
fully up-to-date table.  Every batch's delivered rows, the live table at the end and the Adagrad state are compared bit
for bit; the sampled structure equals that of a run without the key."""
import os
import subprocess
import sys

import numpy as np
import pytest

import update_rows_ref as ref
from engine_harness import batch_keys
from graphgen import exact_features, powerlaw_csr
from learn_driver import gradient

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "learn_driver.py")
NUM_NODE, DIM, EPOCHS, BATCH = 3000, 20, 2, 64
LR, EPS = 0.05, 1e-6
COMMON = ["seed=42", f"batch_size={BATCH}", "fanout=5 4", f"num_epoch={EPOCHS}"]
TASKS = {"node": [], "link": ["task=link_prediction", "num_negative=2"]}
SCHEDULES = [(0, 1), (2, 1), (2, 2)]  # (lookahead, pipelines)
RULES = {"sgd": ref.SGD, "adagrad": ref.ADAGRAD}
STRUCTURE = ["input_nodes", "output_nodes", "row0", "col0", "row1", "col1"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    path = str(tmp_path_factory.mktemp("learn_engine_ds"))
    ip, ix = powerlaw_csr(NUM_NODE, mean_deg=15, seed=5)
    train = np.random.RandomState(5).permutation(NUM_NODE)[:500].astype(np.uint32)
    feat = (exact_features(NUM_NODE, DIM, np.float32) / np.float32(65536.0) - np.float32(100.0)).astype(np.float32)
    label = (np.arange(NUM_NODE, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=DIM, num_class=13))
    edges = np.random.RandomState(6).permutation(ix.size)[:600].astype(np.uint32)
    datagen.write_dataset(path, g, feat=feat, label=label, train_edges=edges)
    return dict(feat=feat, path=path)


def drive(d, prefix, mode, args, ok=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix, mode] + COMMON + args,
                       capture_output=True, text=True, timeout=300, env=env)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


@pytest.fixture(scope="module")
def keyless(dataset, tmp_path_factory):
    """The same runs without the key, one per task (the sampled structure depends on neither lookahead nor pipelines)."""
    return {task: drive(dataset, str(tmp_path_factory.mktemp(f"keyless_{task}") / "out"), "run", args)
            for task, args in TASKS.items()}


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} elements differ, first at {np.argwhere(diff)[0]}: " \
                           f"got {got[diff][0]!r}, want {want[diff][0]!r}"


def replay(npz, feat0, rule, lookahead):
    """The run again in numpy; asserts every batch's delivered rows and returns (table, state) at the end."""
    table, state = feat0.copy(), np.zeros_like(feat0)
    keys = batch_keys(npz)
    assert keys == list(range(len(keys))) and len(keys) >= 2 * (lookahead + 2)
    updates, applied, moved = [], 0, 0
    for j in keys:
        while applied < j - lookahead:  # updates 0 .. j - lookahead - 1 precede the call that enqueued batch j
            ref.update_rows(table, state, *updates[applied], rule, LR, EPS)
            applied += 1
        nodes = npz[f"{j}:input_nodes"].view(np.uint32)
        want = table[nodes]
        same_bits(npz[f"{j}:feat"], want, f"batch {j} (updates 0 .. {applied - 1} applied)")
        moved += int((want.view(np.uint32) != feat0[nodes].view(np.uint32)).any(axis=1).sum())
        updates.append((nodes, gradient(want, nodes)))
    assert moved > 0  # later batches did meet updated rows: the comparison above saw the table move
    for nodes, grad in updates[applied:]:
        ref.update_rows(table, state, nodes, grad, rule, LR, EPS)
    return table, state


@pytest.mark.parametrize("lookahead,pipelines", SCHEDULES, ids=[f"lookahead{h}-pipelines{p}" for h, p in SCHEDULES])
@pytest.mark.parametrize("rule", list(RULES), ids=list(RULES))
@pytest.mark.parametrize("task", list(TASKS), ids=list(TASKS))
def test_run_equals_its_replay(dataset, keyless, tmp_path, task, rule, lookahead, pipelines):
    args = TASKS[task] + [f"feat_learnable={rule}", f"feat_lr={LR}", f"feat_eps={EPS}", f"lookahead={lookahead}",
                          f"pipelines={pipelines}"]
    npz = drive(dataset, str(tmp_path / "out"), "run", args)
    table, state = replay(npz, dataset["feat"], RULES[rule], lookahead)
    same_bits(npz["store_feat"], table, "get_store_feat at the end")
    assert (npz["store_feat"].view(np.uint32) != dataset["feat"].view(np.uint32)).any()
    if rule == "adagrad":
        same_bits(npz["store_state"], state, "get_store_state at the end")
    else:
        assert "store_state" not in npz.files
    same_bits(npz["dataset_feat"], dataset["feat"], "get_dataset_feat: the mapped file")
    # the feature does not touch sampling
    plain = keyless[task]
    assert batch_keys(npz) == batch_keys(plain)
    for key in batch_keys(npz):
        for name in STRUCTURE:
            np.testing.assert_array_equal(npz[f"{key}:{name}"], plain[f"{key}:{name}"], err_msg=f"{key}:{name}")
        same_bits(plain[f"{key}:feat"], dataset["feat"][plain[f"{key}:input_nodes"].view(np.uint32)], f"keyless batch {key}")


LEARN = ["feat_learnable=sgd", f"feat_lr={LR}"]


@pytest.mark.parametrize("mode,words", [
    ("bad_shape", ["update_graph_feat", f", {DIM})"]),
    ("bad_shape_abi", ["samgraph_update_graph_feat", f", {DIM})", "delivered"]),
    ("extract_start", ["extract_start", "feat_learnable"])])
def test_misuse_ends_the_process_with_a_message(dataset, tmp_path, mode, words):
    r = drive(dataset, str(tmp_path / "out"), mode, LEARN, ok=False)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "out") + ".w0.npz")
    for w in words:
        assert w in r.stderr, (w, r.stderr[-2000:])
    if mode != "extract_start":  # both shapes: the gradient's row count and the batch's differ by one
        import re
        shapes = [int(n) for n in re.findall(r"\((\d+), %d\)" % DIM, r.stderr)]
        assert len(shapes) >= 2 and abs(shapes[0] - shapes[1]) == 1, r.stderr[-2000:]


def test_store_views_need_the_key(dataset, tmp_path):
    code = f"""
import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import samgraph.torch as sam
from engine_driver import base_config
cfg = base_config(sam, {dataset['path']!r}, "arch1", {{}})
cfg.update(sampler_ctx="cuda:0", trainer_ctx="cuda:0")
sam.config(cfg); sam.init()
sam.get_store_feat()
"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0 and "samgraph_get_store_feat" in r.stderr and "feat_learnable" in r.stderr, r.stderr[-2000:]
