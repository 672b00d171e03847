"""ggms_quantize_rows and the config key `feat_store_dtype` on a host without a GPU: the entry point is exported, bound
and refuses what it must before it launches anything; datagen.quantize_features(device=None) writes the bytes it always
wrote; and config + data_init refuse the key wherever the engine cannot quantise, naming the key and the reason."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import xgnn_amd
from config_run import ARCH0, run_config
from feat_formats import F16, F32, cpu_fp8, cpu_q8row, write_dataset, write_finite_dataset
from xgnn_amd import _lib, datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_HIP = 0, -1, -2
U8, BF16, F8E4M3, Q8ROW = 3, 7, 16, 18


def test_entry_point_exported_and_bound():
    h = C.CDLL(xgnn_amd.LIB_PATH)
    assert hasattr(h, "ggms_quantize_rows") and "ggms_quantize_rows" in _lib.SYMBOLS
    assert "ggms_quantize_rows" in open(os.path.join(ROOT, "include", "ggms.h")).read()
    assert xgnn_amd.lib().ggms_abi_version() == 3


def _call(out, out_dt, src, src_dt, rows, dim):
    return xgnn_amd.lib().ggms_quantize_rows(C.c_void_p(out), out_dt, C.c_void_p(src), src_dt, rows, dim, 0, None, None)


def test_invalid_arguments_launch_nothing():
    """Host buffers stand in for device memory: an argument error returns before any pointer is used."""
    src = np.zeros(64, np.float32)
    out = np.zeros(64, np.uint64)
    s, o = src.ctypes.data, out.ctypes.data
    assert _call(o, Q8ROW, s, U8, 2, 8) == ERR_INVALID          # U8 source
    assert _call(o, F32, s, F32, 2, 8) == ERR_INVALID           # F32 -> F32
    assert _call(o, F16, s, F16, 2, 8) == ERR_INVALID           # src_dtype == out_dtype
    assert _call(o, F32, s, F16, 2, 8) == ERR_INVALID           # F32 is no output
    assert _call(o + 1, Q8ROW, s, F32, 2, 8) == ERR_INVALID     # Q8ROW out at an odd address
    assert _call(o + 4, Q8ROW, s, F32, 2, 8) == ERR_INVALID     # ... and at 4 mod 8
    assert _call(o, Q8ROW, s + 2, F16, 2, 8) == ERR_INVALID     # src at 2 mod 4
    assert _call(o + 1, BF16, s, F32, 2, 8) == ERR_INVALID      # a 16-bit output at an odd address
    assert _call(o, Q8ROW, s, F32, 2, 0) == ERR_INVALID         # dim 0
    assert b"quantize_rows" in xgnn_amd.lib().ggms_last_error()
    assert _call(o, Q8ROW, s, F32, 0, 8) == OK                  # no rows


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present: the valid call would run")
@pytest.mark.parametrize("out_dt", [F16, BF16, F8E4M3, Q8ROW])
def test_valid_call_without_a_gpu_is_a_hip_error(out_dt):
    src = np.zeros(64, np.float32)
    out = np.zeros(64, np.uint64)
    assert _call(out.ctypes.data, out_dt, src.ctypes.data, F32, 2, 8) == ERR_HIP


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("quantize_host")
    return {"f32": write_finite_dataset(root / "f32x20", F32, 20), "f16": write_finite_dataset(root / "f16x128", F16, 128),
            "raw": write_dataset(root / "raw_f32x20", F32, 20)}


@pytest.mark.parametrize("name,fmt", [("f32", "Q8ROW"), ("f16", "Q8ROW"), ("raw", "F8E4M3"), ("raw", "F8E5M2"), ("f16", "F8E4M3")])
def test_cpu_path_writes_the_bytes_it_always_wrote(datasets, tmp_path, name, fmt):
    d = datasets[name]
    values = d.get("values", d["feat"].view(np.float32) if d["dtype"] == F32 else None)
    out = datagen.quantize_features(d["path"], str(tmp_path / "q"), fmt, chunk_rows=1000, device=None)
    want = cpu_q8row(values) if fmt == "Q8ROW" else cpu_fp8(values, fmt)
    assert open(os.path.join(out, "feat.bin"), "rb").read() == want.tobytes()
    meta = open(os.path.join(out, "meta.txt")).read()
    assert meta.endswith(f"FEAT_DATA_TYPE\t{fmt}\n") and meta.count("FEAT_DATA_TYPE") == 1
    assert open(os.path.join(out, "indices.bin"), "rb").read() == open(os.path.join(d["path"], "indices.bin"), "rb").read()


def test_cpu_path_keeps_its_three_formats(datasets, tmp_path):
    with pytest.raises(AssertionError):
        datagen.quantize_features(datasets["f32"]["path"], str(tmp_path / "q"), "F16")


# ---- config + data_init: tests/test_q8row_config.py's mechanism ------------------------------------------------------


@pytest.fixture(scope="module")
def cfg_datasets(datasets, tmp_path_factory):
    import shutil
    root = tmp_path_factory.mktemp("quantize_cfg")
    out = dict(datasets)
    out["q8"] = dict(path=datagen.quantize_features(datasets["f32"]["path"], str(root / "q8"), "Q8ROW"))
    out["fp8"] = dict(path=datagen.quantize_features(datasets["f32"]["path"], str(root / "fp8"), "F8E5M2"))
    nofeat = root / "nofeat"
    shutil.copytree(datasets["f32"]["path"], nofeat)
    os.remove(nofeat / "feat.bin")
    out["nofeat"] = dict(path=str(nofeat))
    return out


REFUSED = [
    ("arch0", "f32", dict(ARCH0, feat_store_dtype="F8E4M3"), None, ["arch0", "GPU"]),
    ("arch5", "f32", dict(_arch=5, num_sample_worker=1, num_train_worker=1, feat_store_dtype="F8E4M3"), None, ["arch5", "fork"]),
    ("arch6", "f32", dict(_arch=6, num_worker=1, cache_percentage=0.25, gpu_extract="True", feat_store_dtype="Q8ROW",
                          feat_out_dtype="f32"), None, ["arch6", "fork"]),
    ("unknown-value", "f32", dict(feat_store_dtype="INT4"), None, ["INT4", "unknown"]),
    ("lower-case-value", "f32", dict(feat_store_dtype="q8row", feat_out_dtype="f32"), None, ["q8row", "unknown"]),
    ("q8row-table", "q8", dict(feat_store_dtype="F8E4M3", feat_out_dtype="f32"), None, ["FEAT_DATA_TYPE", "F32 or F16"]),
    ("fp8-table", "fp8", dict(feat_store_dtype="Q8ROW", feat_out_dtype="f32"), None, ["FEAT_DATA_TYPE", "F32 or F16"]),
    ("same-type", "f16", dict(feat_store_dtype="F16"), None, ["FEAT_DATA_TYPE", "already"]),
    ("empty-feat", "f32", dict(feat_store_dtype="F8E5M2"), dict(SAMGRAPH_EMPTY_FEAT="6"), ["stand-in", "SAMGRAPH_EMPTY_FEAT"]),
    ("fake-feat-dim", "f32", dict(feat_store_dtype="F8E5M2"), dict(SAMGRAPH_FAKE_FEAT_DIM="32"), ["stand-in", "SAMGRAPH_FAKE_FEAT_DIM"]),
    ("no-feat-bin", "nofeat", dict(feat_store_dtype="BF16"), None, ["stand-in", "feat.bin"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_feat_store_dtype_refused_by_key_and_reason(cfg_datasets, case):
    _, name, extra, env, words = case
    out = run_config(cfg_datasets[name]["path"], extra, env_extra=env)
    assert out.returncode < 0 and "configured" not in out.stdout, (out.stdout, out.stderr[-2000:])  # SIGABRT, like every fatal
    assert "feat_store_dtype" in out.stderr, out.stderr[-2000:]
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


@pytest.mark.parametrize("arch", [dict(), dict(_arch=3, trainer_ctx='cuda:1'), dict(_arch=4, sampler_ctx='cuda:1')],
                         ids=["arch1", "arch3", "arch4"])
def test_q8row_store_without_feat_out_dtype_dies_in_the_existing_words(cfg_datasets, arch):
    out = run_config(cfg_datasets["f32"]["path"], dict(arch, feat_store_dtype="Q8ROW"))
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]
    assert "FEAT_DATA_TYPE Q8ROW needs the config key feat_out_dtype (f32 | f16 | bf16)" in out.stderr, out.stderr[-2000:]


ACCEPTED = [("arch1-q8row", "f32", dict(feat_store_dtype="Q8ROW", feat_out_dtype="f16")),
            ("arch1-fp8", "f16", dict(feat_store_dtype="F8E4M3")),
            ("arch3-bf16", "f32", dict(_arch=3, trainer_ctx='cuda:1', cache_percentage=0.25, feat_store_dtype="BF16")),
            ("arch4-f16", "f32", dict(_arch=4, sampler_ctx='cuda:1', feat_store_dtype="F16"))]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_feat_store_dtype_accepted_on_the_host(cfg_datasets, case):
    """config + data_init touch no GPU: the table is still the one on disk, quantised when the trainer GPU is set up."""
    _, name, extra = case
    out = run_config(cfg_datasets[name]["path"], extra)
    assert out.returncode == 0 and out.stdout.split()[:1] == ["configured"], out.stderr[-2000:]
