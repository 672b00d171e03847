"""feat_out_dtype and FEAT_DATA_TYPE BF16 on the host: which configurations config + data_init take (no GPU touched)
and which they refuse, naming the key and the reason."""
import os
import subprocess
import sys

import numpy as np
import pytest

from feat_convert_common import BF16, F16, F32, write_feat_dataset
from test_engine import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {'_arch': 1, 'sampler_ctx': 'cuda:0', 'trainer_ctx': 'cuda:0', '_sample_type': 0, 'batch_size': 64,
        'num_epoch': 1, '_cache_policy': 0, 'cache_percentage': 0.0, 'max_sampling_jobs': 1, 'max_copying_jobs': 1,
        'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2,
        'fanout': [5, 4]}


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("feat_convert_cfg")
    return {"F32": make_dataset(root / "f32"), "U8": make_dataset(root / "u8", dtype=np.uint8),
            "F16": write_feat_dataset(root / "f16", F16, 20), "BF16": write_feat_dataset(root / "bf16", BF16, 20)}


def _run(path, extra, tail=""):
    cfg = dict(BASE, dataset_path=path)
    cfg.update(extra)
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import samgraph.torch as sam
sam.config({cfg!r})
sam.data_init()
print('configured', sam.num_class(), sam.feat_dim())
{tail}
"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)


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
    out = _run(datasets[table]["path"], extra)
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
    out = _run(datasets[table]["path"], extra)
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
    out = _run(d["path"], {}, tail)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"feat (3000, 20) torch.bfloat16 2 {int(d['feat'][17, 3])}" in out.stdout, out.stdout


def test_bf16_dtype_code():
    from xgnn_amd import lib
    assert lib().ggms_dtype_bytes(7) == 2
    assert [lib().ggms_dtype_bytes(c) for c in (8, -1, 99)] == [0, 0, 0]
