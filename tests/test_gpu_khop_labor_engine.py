"""khop_labor through the engine: every batch is the numpy replay (tests/khop_labor_ref.py) of its seeds with the batch
salt of (seed, epoch, global batch index) -- whatever pipeline, process or deployment drew it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import khop_labor_ref as ref
from engine_harness import ARCH6_ENV, ARCH6_KEYS, DRIVER, ONE_GPU, batch_keys, same_batches
from test_engine import make_dataset

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED, EPOCHS, FANOUT = 42, 2, [5, 4]
COMMON = [f"seed={SEED}", "batch_size=64", "fanout=" + " ".join(map(str, FANOUT)), f"num_epoch={EPOCHS}",
          "sample_type=khop_labor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("labor_engine_ds"))


def drive(d, prefix, arch, keys=None, env=None):
    """One run of tests/feat_driver.py with one worker; its batches."""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}, **(env or {}))
    cmd = [d["path"], prefix, arch, "1"] + COMMON + [f"{k}={v}" for k, v in (keys or {}).items()]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER] + cmd, capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f"{prefix}.t0.npz" if arch == "arch5" else f"{prefix}.w0.npz")


def check_replay(d, npz):
    keys = batch_keys(npz)
    steps = (d["train"].size + 63) // 64
    assert keys == list(range(EPOCHS * steps))
    for key in keys:
        seeds = npz[f"{key}:output_nodes"].view(np.uint32)
        want = ref.sample_batch(d["ip"], d["ix"], seeds, FANOUT, ref.batch_salt(SEED, key // steps, key % steps))
        np.testing.assert_array_equal(npz[f"{key}:input_nodes"].view(np.uint32), want["input_nodes"], err_msg=f"{key}")
        for i, wl in enumerate(want["layers"]):
            np.testing.assert_array_equal(npz[f"{key}:row{i}"].view(np.uint32), wl["row"], err_msg=f"{key}: row{i}")
            np.testing.assert_array_equal(npz[f"{key}:col{i}"].view(np.uint32), wl["col"], err_msg=f"{key}: col{i}")
            assert (int(npz[f"{key}:num_src{i}"]), int(npz[f"{key}:num_dst{i}"])) == (wl["num_src"], wl["num_dst"])


@pytest.fixture(scope="module")
def arch1_run(dataset, tmp_path_factory):
    return drive(dataset, str(tmp_path_factory.mktemp("labor_arch1") / "out"), "arch1")


def test_arch1_batches_are_the_replay(dataset, arch1_run):
    check_replay(dataset, arch1_run)


def test_batches_do_not_depend_on_the_pipelines(dataset, arch1_run, tmp_path):
    two = drive(dataset, str(tmp_path / "out"), "arch1", dict(pipelines=2, lookahead=2))
    same_batches(two, arch1_run)


@pytest.mark.parametrize("arch,keys,env", [("arch3", {}, ONE_GPU), ("arch5", {}, ONE_GPU), ("arch6", ARCH6_KEYS, ARCH6_ENV)],
                         ids=["arch3", "arch5", "arch6"])
def test_other_deployments_are_the_replay(dataset, tmp_path, arch, keys, env):
    check_replay(dataset, drive(dataset, str(tmp_path / "out"), arch, keys, env))
