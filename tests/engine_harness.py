"""What the engine tests of the feature-table formats share (test_gpu_feat_convert_engine.py, test_gpu_fp8_engine.py,
test_gpu_q8row_engine.py, test_gpu_quantize_engine.py): one run of tests/feat_driver.py, the keyless twin runs, and the check of a run's batches against the family's statement of its
table (feat_formats.Table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from feat_formats import ALL_ONES, BITS, KEYS, TORCH_NAME, assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "feat_driver.py")
KHOP3 = ["seed=7", "batch_size=64", "fanout=5 4", "num_epoch=1"]  # the default sampler
KHOP0 = KHOP3 + ["sample_type=khop0"]
ONE_GPU = dict(SAMGRAPH_FORCE_DEVICE="0")
ARCH6_ENV = dict(ONE_GPU, HSA_ENABLE_IPC_MODE_LEGACY="0")
ARCH6_KEYS = dict(cache_percentage="0.25", gpu_extract="True")
SAMPLING = ["input_nodes", "output_nodes", "label", "row0", "col0", "row1", "col1", "num_src0", "num_dst0", "num_src1",
            "num_dst1"]


def drive(d, prefix, arch, keys, env=None, common=KHOP0, table=False, ok=True):
    """One run of the driver on dataset `d`; the batches of every worker (arch6: 2 workers, arch5: 1 trainer, else 1).
    table: the record also holds what the engine says about its feature table.  ok=False: the run may fail, and the
    completed process is returned instead."""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}, **(env or {}))
    workers = 2 if arch == "arch6" else 1
    cmd = [d["path"], prefix, arch, str(workers)] + ["table"] * table + common + [f"{k}={v}" for k, v in keys.items()]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER] + cmd, capture_output=True, text=True,
                       timeout=300, env=env)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    assert "feat_store_dtype" not in keys or "feature table quantised on GPU" in r.stderr, r.stderr[-2000:]
    return [np.load(f"{prefix}.t0.npz")] if arch == "arch5" else [np.load(f"{prefix}.w{w}.npz") for w in range(workers)]


@pytest.fixture(scope="module")
def twin(datasets, tmp_path_factory):
    """twin(arch, key, common): the keyless run on datasets[key] -- the same graph, labels and train set as every other
    dataset of the module -- once per argument list."""
    runs = {}

    def get(arch, key, common=KHOP0):
        if (arch, key, tuple(common)) not in runs:
            keys, env = {"arch6": (ARCH6_KEYS, ARCH6_ENV), "arch5": ({}, ONE_GPU), "arch1": ({}, None)}[arch]
            prefix = str(tmp_path_factory.mktemp(f"twin_{arch}") / "out")
            runs[(arch, key, tuple(common))] = drive(datasets[key], prefix, arch, keys, env, common)
        return runs[(arch, key, tuple(common))]
    return get


def batch_keys(npz):
    return sorted({int(k.split(":")[0]) for k in npz.files if ":" in k})


def same_batches(got, want, names=SAMPLING):
    assert batch_keys(got) == batch_keys(want) and len(batch_keys(got)) >= 4
    for key in batch_keys(got):
        for name in names:
            np.testing.assert_array_equal(got[f"{key}:{name}"], want[f"{key}:{name}"], err_msg=f"{key}:{name}")


def check_batches(npz, plain, d, out_dt, row_mask=ALL_ONES):
    """Sampling outputs equal the twin run's; the feature rows are the table rows (& row_mask) of input_nodes as the
    table's format decodes into out_dt, bit for bit and NaN where NaN is due (out_dt = the table's own dtype, no key:
    the stored bytes); feature bytes are counted in the delivered dtype, whatever a stored row takes."""
    same_batches(npz, plain)
    table = d["table"]
    for key in batch_keys(npz):
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        rows = nodes & np.uint32(row_mask)
        assert str(npz[f"{key}:feat_dtype"]) == TORCH_NAME[out_dt]
        got = npz[f"{key}:feat_bits"].view(BITS[out_dt])
        nan = table.nan(rows) if out_dt != table.fmt else np.zeros(got.shape, bool)
        assert_bits(got, table.want(out_dt, rows), nan, f"batch {key}", dt=out_dt, codes=table.code_of(rows))
        assert float(npz[f"{key}:feature_bytes"]) == nodes.size * table.dim * np.dtype(BITS[out_dt]).itemsize


def run_and_check(datasets, twin, tmp_path, arch, key, out_dt, twin_key, keys=None, env=None, common=KHOP0, row_mask=ALL_ONES):
    """One run on datasets[key] delivering out_dt (its own dtype: no feat_out_dtype), every worker's batches checked
    against the keyless run on datasets[twin_key] in the same deployment (arch3: arch1's); the runs."""
    keys = dict(keys or {}, **({} if out_dt == key[0] else dict(feat_out_dtype=KEYS[out_dt])))
    runs = drive(datasets[key], str(tmp_path / "out"), arch, keys, env, common)
    for run, plain in zip(runs, twin("arch1" if arch == "arch3" else arch, twin_key, common)):
        check_batches(run, plain, datasets[key], out_dt, row_mask)
    return runs


def check_miss_bytes(npz, d, cache_percentage, row_bytes=None):
    """Bytes read from the host tier: whole STORED rows (the table's dtype; Q8ROW: trailer and pad included) of the
    input nodes outside the degree-ranked cache (row_bytes: of the table the engine made of d's, where it made one)."""
    from xgnn_amd import datagen
    num_node = d["ip"].size - 1
    cached = np.zeros(num_node, bool)
    cached[datagen.degree_rank(d["ip"])[: int(num_node * cache_percentage)]] = True
    for key in batch_keys(npz):
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        assert float(npz[f"{key}:miss_bytes"]) == int((~cached[nodes]).sum()) * (row_bytes or d["table"].row_bytes)
