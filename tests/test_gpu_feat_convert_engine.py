"""Config key `feat_out_dtype` through the engine: the batch's feature rows are the CPU conversion of the table's rows,
delivered in the configured torch dtype, and nothing else of the batch changes (tests/engine_harness.py).  The twin of
every run is the keyless run on the F16 dataset: the same graph, the same seed, the default sampler."""
import numpy as np
import pytest

from engine_harness import ARCH6_ENV, ARCH6_KEYS, KHOP3, ONE_GPU, batch_keys, check_miss_bytes, run_and_check, twin  # noqa: F401 (twin: a fixture)
from feat_formats import BF16, F16, F32, NAMES, assert_bits, write_dataset

pytestmark = pytest.mark.gpu

PLAIN = (F16, 20)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("feat_convert_ds")
    return {(dt, dim): write_dataset(root / f"{NAMES[dt]}x{dim}", dt, dim) for dt, dim in [(F16, 20), (F32, 20), (BF16, 20), (BF16, 7)]}


ARCH1 = [(F16, 20, F32), (F32, 20, BF16), (F32, 20, F16), (BF16, 20, F32), (BF16, 7, F32)]


@pytest.mark.parametrize("table,dim,out_dt", ARCH1, ids=[f"{NAMES[t]}x{n}-{NAMES[o]}" for t, n, o in ARCH1])
def test_arch1(datasets, twin, tmp_path, table, dim, out_dt):
    run_and_check(datasets, twin, tmp_path, "arch1", (table, dim), out_dt, PLAIN, common=KHOP3)


def test_arch1_mock_table_converts(datasets, twin, tmp_path):
    """SAMGRAPH_EMPTY_FEAT=6: a 64-row stand-in table (the first rows of feat.bin), row = node & 63."""
    run_and_check(datasets, twin, tmp_path, "arch1", (F16, 20), F32, PLAIN, env=dict(SAMGRAPH_EMPTY_FEAT="6"), common=KHOP3,
                  row_mask=63)


ARCH6 = [dict(ARCH6_KEYS), dict(cache_percentage="0.4", part_cache="True", gpu_extract="True", replicate_percentage="0.5"),
         dict(cache_percentage="1.0", part_cache="True", gpu_extract="True")]


@pytest.mark.parametrize("opts", ARCH6, ids=["cached-with-misses", "tiered", "full-cache"])
def test_arch6_two_workers_one_gpu(datasets, twin, tmp_path, opts):
    """F16 table -> f32 through ggms_extract_cached_convert (table / no table) and ggms_extract_tiered_convert."""
    for run in run_and_check(datasets, twin, tmp_path, "arch6", (F16, 20), F32, PLAIN, opts, ARCH6_ENV, KHOP3):
        check_miss_bytes(run, datasets[(F16, 20)], float(opts["cache_percentage"]))  # in the TABLE's dtype: 2-byte elements


def test_arch3_two_contexts_one_gpu(datasets, twin, tmp_path):
    run_and_check(datasets, twin, tmp_path, "arch3", (F32, 20), BF16, PLAIN, env=ONE_GPU, common=KHOP3)


def test_without_the_key_an_f16_table_is_cast_to_float32_as_before(datasets, twin):
    table = datasets[PLAIN]["table"]
    npz, = twin("arch1", PLAIN, KHOP3)
    for key in batch_keys(npz):
        nodes = npz[f"{key}:input_nodes"].view(np.uint32)
        assert str(npz[f"{key}:feat_dtype"]) == "torch.float32"
        assert_bits(npz[f"{key}:feat_bits"].view(np.uint32), table.want(F32, nodes), table.nan(nodes), f"batch {key}", dt=F32)
        assert float(npz[f"{key}:feature_bytes"]) == nodes.size * 20 * 2  # the gather itself wrote f16 rows
