"""FEAT_DATA_TYPE F8E4M3 / F8E5M2 on the host: which configurations config + data_init take (no GPU touched) and which
they refuse, in the words the refusals had before FP8 tables existed."""
import pytest

from config_run import ARCH0, run_config
from feat_formats import E4M3, E5M2, write_dataset


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("fp8_cfg")
    return {"F8E4M3": write_dataset(root / "e4m3", E4M3, 20), "F8E5M2": write_dataset(root / "e5m2", E5M2, 20)}


ACCEPTED = [("arch1-no-key", "F8E4M3", {}), ("arch0-no-key", "F8E5M2", ARCH0)]
for _out in ("f32", "f16", "bf16"):
    ACCEPTED += [
        (f"arch1-{_out}", "F8E4M3", dict(feat_out_dtype=_out)),
        (f"arch3-{_out}", "F8E5M2", dict(_arch=3, trainer_ctx='cuda:1', feat_out_dtype=_out)),
        (f"arch6-gpu-extract-{_out}", "F8E4M3",
         dict(_arch=6, num_worker=1, cache_percentage=0.25, gpu_extract="True", feat_out_dtype=_out)),
        (f"arch6-full-cache-{_out}", "F8E5M2", dict(_arch=6, num_worker=1, cache_percentage=1.0, feat_out_dtype=_out)),
    ]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_fp8_table_accepted(datasets, case):
    _, table, extra = case
    out = run_config(datasets[table]["path"], extra)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("arch0", "F8E4M3", dict(ARCH0, feat_out_dtype='f16'), ["arch0", "CPU"]),
    ("host-staged-partial-cache", "F8E4M3", dict(_arch=6, num_worker=1, cache_percentage=0.3, feat_out_dtype='f16'),
     ["arch6", "host-staged", "gpu_extract"]),
    ("host-staged-no-cache", "F8E5M2", dict(_arch=6, num_worker=1, feat_out_dtype='f32'), ["arch6", "host-staged"]),
    ("dynamic-cache", "F8E5M2", dict(_arch=4, sampler_ctx='cuda:1', _cache_policy=6, feat_out_dtype='bf16'),
     ["arch4", "dynamic_cache"]),
    ("fp8-as-output", "F8E4M3", dict(feat_out_dtype='f8e4m3'), ["f8e4m3", "f32, f16 or bf16"]),
    ("fp8-as-output-e5m2", "F8E5M2", dict(feat_out_dtype='f8e5m2'), ["f8e5m2", "f32, f16 or bf16"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_fp8_table_refused_in_the_existing_words(datasets, case):
    _, table, extra, words = case
    out = run_config(datasets[table]["path"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    assert "feat_out_dtype" in out.stderr, out.stderr[-2000:]
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


@pytest.mark.parametrize("table", ["F8E4M3", "F8E5M2"])
def test_fp8_table_loads_as_the_mapped_file(datasets, table):
    """The dataset tensor is (N, dim) of the torch FP8 dtype, one byte per element, the file's bytes."""
    d = datasets[table]
    tail = """
import torch
f = sam.get_dataset_feat()
print('feat', tuple(f.shape), f.dtype, f.element_size(), f.view(torch.uint8)[:300].flatten().tolist() == EXPECT)
""".replace("EXPECT", repr(d["feat"][:300].ravel().tolist()))
    out = run_config(d["path"], {}, tail)
    assert out.returncode == 0, out.stderr[-2000:]
    name = {"F8E4M3": "torch.float8_e4m3fn", "F8E5M2": "torch.float8_e5m2"}[table]
    assert f"feat (3000, 20) {name} 1 True" in out.stdout, out.stdout
