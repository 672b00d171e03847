"""FEAT_DATA_TYPE Q8ROW on the host: which configurations config + data_init take (no GPU touched), which they refuse --
a row-scaled table NEEDS feat_out_dtype; with the key the refusals are the ones every converting table gets, in their
words -- and what the engine sizes: a table of rows x stride bytes, a batch buffer of dim x batch dtype."""
import os

import pytest

from config_run import ARCH0, run_config
from feat_formats import Q8ROW, stride, write_dataset


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("q8row_cfg")
    return {dim: write_dataset(root / f"q8x{dim}", Q8ROW, dim) for dim in (20, 128)}


ARCH6 = dict(_arch=6, num_worker=1, cache_percentage=0.25, gpu_extract="True")
NO_KEY = [("arch1", {}), ("arch0", ARCH0), ("arch3", dict(_arch=3, trainer_ctx='cuda:1')), ("arch6-gpu-extract", ARCH6),
          ("arch4-dynamic-cache", dict(_arch=4, sampler_ctx='cuda:1', _cache_policy=6))]


@pytest.mark.parametrize("case", NO_KEY, ids=[c[0] for c in NO_KEY])
def test_q8row_table_without_feat_out_dtype_is_fatal(datasets, case):
    out = run_config(datasets[20]["path"], case[1])
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    assert "feat_out_dtype" in out.stderr and "Q8ROW" in out.stderr, out.stderr[-2000:]


REFUSED = [
    ("arch0", dict(ARCH0, feat_out_dtype='f16'), ["arch0", "CPU"]),
    ("host-staged-partial-cache", dict(_arch=6, num_worker=1, cache_percentage=0.3, feat_out_dtype='f16'),
     ["arch6", "host-staged", "gpu_extract"]),
    ("host-staged-no-cache", dict(_arch=6, num_worker=1, feat_out_dtype='f32'), ["arch6", "host-staged"]),
    ("dynamic-cache", dict(_arch=4, sampler_ctx='cuda:1', _cache_policy=6, feat_out_dtype='bf16'), ["arch4", "dynamic_cache"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_q8row_table_refused_in_the_existing_words(datasets, case):
    _, extra, words = case
    out = run_config(datasets[20]["path"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]
    assert "feat_out_dtype" in out.stderr, out.stderr[-2000:]
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


ACCEPTED = [("arch1-f32", 20, dict(feat_out_dtype='f32'), 4), ("arch1-bf16", 128, dict(feat_out_dtype='bf16'), 2),
            ("arch3-f16", 128, dict(_arch=3, trainer_ctx='cuda:1', feat_out_dtype='f16'), 2),
            ("arch4-f32", 20, dict(_arch=4, sampler_ctx='cuda:1', feat_out_dtype='f32'), 4),
            ("arch6-gpu-extract-f16", 20, dict(ARCH6, feat_out_dtype='f16'), 2),
            ("arch6-full-cache-f32", 128, dict(_arch=6, num_worker=1, cache_percentage=1.0, feat_out_dtype='f32'), 4)]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_q8row_table_accepted_and_sized(datasets, case):
    """Table: 3000 rows of stride bytes, handed out as uint8 (rows, stride), the mapped file.  Batch buffer rows:
    dim x the batch dtype, whatever a stored row takes."""
    _, dim, extra, out_es = case
    d = datasets[dim]
    tail = """
import torch
f = sam.get_dataset_feat()
print('feat', tuple(f.shape), f.dtype, f.numel() * f.element_size(), f[:40].flatten().tolist() == EXPECT)
print('row bytes', sam.feat_row_bytes(), sam.feat_row_bytes(delivered=True))
""".replace("EXPECT", repr(d["table"].stored[:40].ravel().tolist()))
    out = run_config(d["path"], extra, tail)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[:3] == ["configured", "13", str(dim)]
    assert f"feat (3000, {stride(dim)}) torch.uint8 {3000 * stride(dim)} True" in out.stdout, out.stdout
    assert f"row bytes {stride(dim)} {dim * out_es}" in out.stdout, out.stdout
    assert os.path.getsize(os.path.join(d["path"], "feat.bin")) == 3000 * stride(dim)


def test_a_table_one_byte_short_of_rows_x_stride_is_refused(datasets, tmp_path):
    """data_init maps num_node x stride bytes of feat.bin: a file that holds a byte less does not load."""
    import shutil
    short = tmp_path / "short"
    shutil.copytree(datasets[20]["path"], short)
    with open(short / "feat.bin", "r+b") as f:
        f.truncate(3000 * stride(20) - 1)
    out = run_config(str(short), dict(feat_out_dtype='f32'))
    assert out.returncode < 0 and "feat.bin" in out.stderr and "smaller" in out.stderr, out.stderr[-2000:]
