"""Config key `feat_store_dtype` through the engine (samgraph.torch): an F32 / F16 dataset quantised by the trainer GPU
at init behaves like its twin that datagen.quantize_features wrote on the CPU and a run without the key loaded from
disk -- the same batches bit for bit, the same table, the same row and miss bytes.  The driver is
tests/feat_driver.py.  The datasets are feat_formats.write_dataset's; where the store is Q8ROW their NaN / inf
elements are replaced (write_finite_dataset): a row-scaled table has no code for them."""
import functools
import os

import numpy as np
import pytest

from engine_harness import ONE_GPU, SAMPLING, batch_keys, check_miss_bytes, drive, same_batches
from feat_formats import BF16, F16, F32, from_f32, stride, write_dataset, write_finite_dataset
from xgnn_amd import datagen

pytestmark = pytest.mark.gpu


run = functools.partial(drive, table=True)  # every record also holds what the engine says about its table


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("quantize_engine")
    ds = {"f32x20": write_finite_dataset(root / "f32x20", F32, 20), "f32x128": write_finite_dataset(root / "f32x128", F32, 128),
          "f16x128": write_dataset(root / "f16x128", F16, 128), "raw_f32x128": write_dataset(root / "raw", F32, 128),
          "nan_f32x20": write_finite_dataset(root / "nan", F32, 20, bad_rows={1234: np.nan})}
    for name, fmt in [("f32x20", "Q8ROW"), ("f32x128", "Q8ROW"), ("f16x128", "F8E4M3")]:
        ds[f"{name}:{fmt}"] = dict(path=datagen.quantize_features(ds[name]["path"], str(root / f"{name}_{fmt}"), fmt))
    return ds


def _same_run(got, twin):
    """Every batch and what the engine says about its table: the key's run and the run on the CPU-quantised twin."""
    same_batches(got, twin, SAMPLING + ["feat_bits", "feat_dtype", "miss_bytes", "feature_bytes"])
    for name in ("table_bytes", "table_dtype", "table_shape", "feat_row_bytes"):
        np.testing.assert_array_equal(got[name], twin[name], err_msg=name)


def test_arch1_q8row_from_f32(datasets, tmp_path):
    d = datasets["f32x20"]
    got, = run(d, str(tmp_path / "key"), "arch1", dict(feat_store_dtype="Q8ROW", feat_out_dtype="f32"))
    twin, = run(datasets["f32x20:Q8ROW"], str(tmp_path / "twin"), "arch1", dict(feat_out_dtype="f32"))
    plain, = run(d, str(tmp_path / "plain"), "arch1", {})
    _same_run(got, twin)
    same_batches(got, plain, SAMPLING)  # sampling does not depend on how the table is stored
    assert str(got["table_dtype"]) == "torch.uint8" and got["table_shape"].tolist() == [3000, 32] and int(got["feat_row_bytes"]) == 32
    cpu_file = np.fromfile(os.path.join(datasets["f32x20:Q8ROW"]["path"], "feat.bin"), np.uint8)
    np.testing.assert_array_equal(got["table_bytes"].ravel(), cpu_file)
    assert str(got[f"{batch_keys(got)[0]}:feat_dtype"]) == "torch.float32"


@pytest.mark.parametrize("out_key,batch_dtype", [(dict(feat_out_dtype="f16"), "torch.float16"), ({}, "torch.float8_e4m3fn")],
                         ids=["f16", "as-stored"])
def test_arch1_fp8_from_f16(datasets, tmp_path, out_key, batch_dtype):
    got, = run(datasets["f16x128"], str(tmp_path / "key"), "arch1", dict(out_key, feat_store_dtype="F8E4M3"))
    twin, = run(datasets["f16x128:F8E4M3"], str(tmp_path / "twin"), "arch1", out_key)
    _same_run(got, twin)
    assert str(got[f"{batch_keys(got)[0]}:feat_dtype"]) == batch_dtype
    assert str(got["table_dtype"]) == "torch.float8_e4m3fn" and int(got["feat_row_bytes"]) == 128


def test_arch1_bf16_from_f32_without_feat_out_dtype(datasets, tmp_path):
    d = datasets["raw_f32x128"]
    got, = run(d, str(tmp_path / "key"), "arch1", dict(feat_store_dtype="BF16"))
    want = from_f32(np.array(d["feat"].view(np.float32)), BF16)  # table.to(bfloat16), as bits
    nan = np.isnan(d["feat"].view(np.float32))
    for key in batch_keys(got):
        assert str(got[f"{key}:feat_dtype"]) == "torch.bfloat16"
        nodes = got[f"{key}:input_nodes"].view(np.uint32)
        bits = got[f"{key}:feat_bits"].view(np.uint16)
        assert bits.shape == (nodes.size, 128)
        assert np.array_equal(bits[~nan[nodes]], want[nodes][~nan[nodes]])
        assert np.isnan((bits.astype(np.uint32) << 16).view(np.float32)[nan[nodes]]).all()
    assert int(got["feat_row_bytes"]) == 256 and str(got["table_dtype"]) == "torch.bfloat16"


def test_arch3_q8row_with_a_cache(datasets, tmp_path):
    keys = dict(cache_percentage="0.25", feat_out_dtype="f16")
    d = datasets["f32x128"]
    got, = run(d, str(tmp_path / "key"), "arch3", dict(keys, feat_store_dtype="Q8ROW"), ONE_GPU)
    twin, = run(datasets["f32x128:Q8ROW"], str(tmp_path / "twin"), "arch3", keys, ONE_GPU)
    _same_run(got, twin)
    check_miss_bytes(got, d, 0.25, stride(128))  # whole stored rows, trailer and pad included


def test_arch4_q8row(datasets, tmp_path):
    got, = run(datasets["f32x20"], str(tmp_path / "key"), "arch4", dict(feat_store_dtype="Q8ROW", feat_out_dtype="f32"), ONE_GPU)
    twin, = run(datasets["f32x20:Q8ROW"], str(tmp_path / "twin"), "arch4", dict(feat_out_dtype="f32"), ONE_GPU)
    _same_run(got, twin)


def test_a_nan_row_aborts_q8row_and_names_the_row(datasets, tmp_path):
    d = datasets["nan_f32x20"]
    r = run(d, str(tmp_path / "q8"), "arch1", dict(feat_store_dtype="Q8ROW", feat_out_dtype="f32"), ok=False)
    assert r.returncode != 0 and "feat_store_dtype" in r.stderr and "row 1234" in r.stderr and "NaN or inf" in r.stderr, \
        r.stderr[-2000:]
    got, = run(d, str(tmp_path / "e5m2"), "arch1", dict(feat_store_dtype="F8E5M2"))  # FP8 has a code for NaN
    assert str(got[f"{batch_keys(got)[0]}:feat_dtype"]) == "torch.float8_e5m2" and len(batch_keys(got)) >= 4
