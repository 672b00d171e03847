"""negative_mode = typed_uniform | typed_exclude through the engine (arch1, khop_typed, hetero_batch, 1 and 2 pipelines) on
test_gpu_hetero_engine's data set: every batch's output nodes are the numpy statement (tests/link_typed_ref.py) replayed
from the batch's own positive edge ids under link_ref.engine_salt; get_graph_link_rel is edge_type[link_edge_ids]; and a
control run with negative_mode = exclude on the same data is link_ref's, as before.

The relation table names a relation's ends in message-passing terms: a list's OWNER -- the positive's source u -- has
relation_dst_type(rel), a list ENTRY -- the positive's destination v -- relation_src_type(rel).  The negatives stand in
for v: their type is node_type[v] = relation_src_type(rel); both ends are checked against the table."""
import os
import subprocess
import sys

import numpy as np
import pytest

import link_ref as ref
import link_typed_ref as tref
from engine_harness import batch_keys
from test_gpu_hetero_engine import BATCH, K, ROOT, SEED, T, args_of, dataset  # noqa: F401  (fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "tests", "link_typed_driver.py")
MODES = {"typed_uniform": tref.TYPED_UNIFORM, "typed_exclude": tref.TYPED_EXCLUDE, "exclude": ref.EXCLUDE}


def drive(d, prefix, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER, d["path"], prefix] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.w0.npz")


@pytest.mark.parametrize("pipes", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_every_batch_is_the_twins_replay(dataset, tmp_path, mode, pipes):  # noqa: F811
    d = dataset
    ip, ix, et, nt = d["ip"], d["ix"], d["et"], d["nt"]
    got = drive(d, str(tmp_path / "run"), args_of("link_prediction", pipes, hetero_batch="on", negative_mode=mode))
    steps = int(got["steps_per_epoch"])
    assert batch_keys(got) == list(range(steps)) and steps == 5
    for key in batch_keys(got):
        eids = got[f"{key}:link_edge_ids"].view(np.uint32)
        out = got[f"{key}:output_nodes"].view(np.uint32)
        salt = ref.engine_salt(SEED, key // steps, key % steps)
        if mode == "exclude":  # the control: the untyped leaf, and no relations handed out
            np.testing.assert_array_equal(out, ref.link_seeds(ip, ix, eids, K, ref.EXCLUDE, salt)[0], err_msg=f"batch {key}")
            assert f"{key}:link_rel" not in got.files
            continue
        want, want_rel, _ = tref.link_seeds_typed(ip, ix, et, nt, T, eids, K, MODES[mode], salt)
        np.testing.assert_array_equal(out, want, err_msg=f"batch {key}")
        rel = got[f"{key}:link_rel"]
        np.testing.assert_array_equal(rel, et[eids])
        np.testing.assert_array_equal(rel, want_rel)
        src, dst, neg = ref.split(out, K)
        rel_src, rel_dst = np.asarray(got[f"{key}:rel_src"])[rel], np.asarray(got[f"{key}:rel_dst"])[rel]
        assert eids.size == BATCH and (nt[src] == rel_dst).all() and (nt[dst] == rel_src).all()
        assert (nt[neg] == rel_src[:, None]).all()
