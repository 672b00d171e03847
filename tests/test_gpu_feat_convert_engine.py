"""Config key `feat_out_dtype` through the engine: the batch's feature rows are the CPU conversion of the table's rows,
delivered in the configured torch dtype, and nothing else of the batch changes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from feat_convert_common import BF16, BITS, F16, F32, KEYS, NAMES, assert_same_bits, convert_bits, write_feat_dataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "feat_convert_driver.py")
COMMON = ["seed=7", "batch_size=64", "fanout=5 4", "num_epoch=1"]
TORCH_NAME = {F32: "torch.float32", F16: "torch.float16", BF16: "torch.bfloat16"}
ARCH6_ENV = dict(SAMGRAPH_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")


def _drive(d, prefix, arch, workers, keys, env=None):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}, **(env or {}))
    r = subprocess.run([sys.executable, DRIVER, d["path"], prefix, arch, str(workers)] + COMMON +
                       [f"{k}={v}" for k, v in keys.items()], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [np.load(f"{prefix}.w{w}.npz") for w in range(workers)]


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("feat_convert_ds")
    return {(F16, 20): write_feat_dataset(root / "f16", F16, 20), (F32, 20): write_feat_dataset(root / "f32", F32, 20),
            (BF16, 20): write_feat_dataset(root / "bf16", BF16, 20), (BF16, 7): write_feat_dataset(root / "bf16x7", BF16, 7)}


@pytest.fixture(scope="module")
def plain_arch1(datasets, tmp_path_factory):
    """The run without the key (F16 table): every arch1 / arch3 case samples the same graph with the same seed."""
    return _drive(datasets[(F16, 20)], str(tmp_path_factory.mktemp("plain1") / "out"), "arch1", 1, {})


@pytest.fixture(scope="module")
def plain_arch6(datasets, tmp_path_factory):
    return _drive(datasets[(F16, 20)], str(tmp_path_factory.mktemp("plain6") / "out"), "arch6", 2,
                  dict(cache_percentage="0.25", gpu_extract="True"), ARCH6_ENV)


def _keys(npz):
    return sorted({int(k.split(":")[0]) for k in npz.files})


def _check(npz, plain, d, out_dt, row_mask=0xFFFFFFFF):
    """Sampling outputs equal the keyless run's; feat = the CPU conversion of the table rows of input_nodes."""
    assert _keys(npz) == _keys(plain) and len(_keys(npz)) >= 4
    dim = d["feat"].shape[1]
    for key in _keys(npz):
        for name in ["input_nodes", "output_nodes", "label", "row0", "col0", "row1", "col1", "num_src0", "num_dst0",
                     "num_src1", "num_dst1"]:
            np.testing.assert_array_equal(npz[f"{key}:{name}"], plain[f"{key}:{name}"], err_msg=f"{key}:{name}")
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        assert str(npz[f"{key}:feat_dtype"]) == TORCH_NAME[out_dt]
        got = npz[f"{key}:feat_bits"].view(BITS[out_dt])
        assert_same_bits(got, convert_bits(d["feat"][nodes & np.uint32(row_mask)], d["dtype"], out_dt), out_dt, f"batch {key}")
        # bytes written to the batch, in the delivered dtype
        assert float(npz[f"{key}:feature_bytes"]) == nodes.size * dim * np.dtype(BITS[out_dt]).itemsize


ARCH1 = [(F16, 20, F32), (F32, 20, BF16), (F32, 20, F16), (BF16, 20, F32), (BF16, 7, F32)]


@pytest.mark.parametrize("table,dim,out_dt", ARCH1, ids=[f"{NAMES[t]}x{n}-{NAMES[o]}" for t, n, o in ARCH1])
def test_arch1(datasets, plain_arch1, tmp_path, table, dim, out_dt):
    d = datasets[(table, dim)]
    npz, = _drive(d, str(tmp_path / "out"), "arch1", 1, dict(feat_out_dtype=KEYS[out_dt]))
    _check(npz, plain_arch1[0], d, out_dt)


def test_arch1_mock_table_converts(datasets, plain_arch1, tmp_path):
    """SAMGRAPH_EMPTY_FEAT=6: a 64-row stand-in table (the first rows of feat.bin), row = node & 63."""
    d = datasets[(F16, 20)]
    npz, = _drive(d, str(tmp_path / "out"), "arch1", 1, dict(feat_out_dtype="f32"), dict(SAMGRAPH_EMPTY_FEAT="6"))
    _check(npz, plain_arch1[0], d, F32, row_mask=63)


ARCH6 = [dict(cache_percentage="0.25", gpu_extract="True"),
         dict(cache_percentage="0.4", part_cache="True", gpu_extract="True", replicate_percentage="0.5"),
         dict(cache_percentage="1.0", part_cache="True", gpu_extract="True")]


@pytest.mark.parametrize("opts", ARCH6, ids=["cached-with-misses", "tiered", "full-cache"])
def test_arch6_two_workers_one_gpu(datasets, plain_arch6, tmp_path, opts):
    """F16 table -> f32 through ggms_extract_cached_convert (table / no table) and ggms_extract_tiered_convert."""
    from xgnn_amd import datagen
    d = datasets[(F16, 20)]
    runs = _drive(d, str(tmp_path / "out"), "arch6", 2, dict(opts, feat_out_dtype="f32"), ARCH6_ENV)
    rank = datagen.degree_rank(d["ip"])
    cached = np.zeros(d["ip"].size - 1, bool)
    cached[rank[: int((d["ip"].size - 1) * float(opts["cache_percentage"]))]] = True
    for w in range(2):
        _check(runs[w], plain_arch6[w], d, F32)
        for key in _keys(runs[w]):  # bytes read from the host tier, in the TABLE's dtype: 2-byte elements
            nodes = runs[w][f"{key}:input_nodes"].view(np.uint32)
            assert float(runs[w][f"{key}:miss_bytes"]) == int((~cached[nodes]).sum()) * 20 * 2


def test_arch3_two_contexts_one_gpu(datasets, plain_arch1, tmp_path):
    d = datasets[(F32, 20)]
    npz, = _drive(d, str(tmp_path / "out"), "arch3", 1, dict(feat_out_dtype="bf16"), dict(SAMGRAPH_FORCE_DEVICE="0"))
    _check(npz, plain_arch1[0], d, BF16)


def test_without_the_key_an_f16_table_is_cast_to_float32_as_before(datasets, plain_arch1):
    d = datasets[(F16, 20)]
    npz = plain_arch1[0]
    for key in _keys(npz):
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        assert str(npz[f"{key}:feat_dtype"]) == "torch.float32"
        assert_same_bits(npz[f"{key}:feat_bits"].view(np.uint32), convert_bits(d["feat"][nodes], F16, F32), F32)
        assert float(npz[f"{key}:feature_bytes"]) == nodes.size * 20 * 2  # the gather itself wrote f16 rows
