"""feat_out_dtype and FEAT_DATA_TYPE BF16 on the host: which configurations config + data_init take (no GPU touched)
and which they refuse, naming the key and the reason."""
import numpy as np
import pytest

from config_run import run_config
from feat_formats import BF16, F16, write_dataset
from test_engine import make_dataset


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("feat_convert_cfg")
    return {"F32": make_dataset(root / "f32"), "U8": make_dataset(root / "u8", dtype=np.uint8),
            "F16": write_dataset(root / "f16", F16, 20), "BF16": write_dataset(root / "bf16", BF16, 20)}


REFUSED = [
    ("arch0", "F32", dict(_arch=0, sampler_ctx='cpu:0', trainer_ctx='cpu:0', feat_out_dtype='f16'), ["arch0", "CPU"]),
    ("dynamic-cache", "F32", dict(_arch=4, sampler_ctx='cuda:1', _cache_policy=6, feat_out_dtype='bf16'),
     ["arch4", "dynamic_cache"]),
    ("host-staged-partial-cache", "F32", dict(_arch=6, num_worker=1, cache_percentage=0.3, feat_out_dtype='f16'),
     ["arch6", "host-staged", "gpu_extract"]),
    ("host-staged-no-cache", "F16", dict(_arch=6, num_worker=1, feat_out_dtype='f32'), ["arch6", "host-staged"]),
    ("u8-table", "U8", dict(feat_out_dtype='f32'), ["FEAT_DATA_TYPE U8"]),
    ("f64", "F32", dict(feat_out_dtype='f64'), ["f64", "f32, f16 or bf16"]),
    ("int8", "F32", dict(feat_out_dtype='int8'), ["int8", "f32, f16 or bf16"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_feat_out_dtype_refused_by_key_and_reason(datasets, case):
    _, table, extra, words = case
    out = run_config(datasets[table]["path"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    assert "feat_out_dtype" in out.stderr, out.stderr[-2000:]
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


ACCEPTED = [
    ("arch1-f16-to-f32", "F16", dict(feat_out_dtype='f32')),
    ("arch1-f32-to-bf16", "F32", dict(feat_out_dtype='bf16')),
    ("arch1-bf16-to-f16", "BF16", dict(feat_out_dtype='f16')),
    ("arch1-own-dtype", "F16", dict(feat_out_dtype='f16')),
    ("arch3", "F32", dict(_arch=3, trainer_ctx='cuda:1', feat_out_dtype='bf16')),
    ("arch4-no-cache", "F32", dict(_arch=4, sampler_ctx='cuda:1', feat_out_dtype='f16')),
    ("arch6-gpu-extract", "F16", dict(_arch=6, num_worker=1, cache_percentage=0.25, gpu_extract="True", feat_out_dtype='f32')),
    ("arch6-full-cache", "F16", dict(_arch=6, num_worker=1, cache_percentage=1.0, feat_out_dtype='f32')),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_feat_out_dtype_accepted(datasets, case):
    _, table, extra = case
    out = run_config(datasets[table]["path"], extra)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


def test_bf16_table_loads(datasets):
    """FEAT_DATA_TYPE BF16: the dataset tensor is the mapped file, (N, dim) bfloat16, two bytes per element."""
    d = datasets["BF16"]
    tail = """
import torch
f = sam.get_dataset_feat()
print('feat', tuple(f.shape), f.dtype, f.element_size(), int(f.view(torch.int16)[17, 3]) & 0xffff)
"""
    out = run_config(d["path"], {}, tail)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"feat (3000, 20) torch.bfloat16 2 {int(d['feat'][17, 3])}" in out.stdout, out.stdout


def test_bf16_dtype_code():
    from xgnn_amd import lib
    assert lib().ggms_dtype_bytes(7) == 2
    assert [lib().ggms_dtype_bytes(c) for c in (8, -1, 99)] == [0, 0, 0]
