"""khop_labor on the host: the reference's hash and salt vectors, the marginal uniformity of its selection, the argument
errors of the leaf (no GPU touched), and which deployments take `_sample_type` 8."""
import ctypes as C

import numpy as np
import pytest

import khop_labor_ref as ref
from config_run import ARCH0, run_config
from test_engine import make_dataset
from xgnn_amd._lib import Graph, lib

INVALID = -1  # GGMS_ERR_INVALID
KHOP_LABOR = 8


def test_fmix32_and_salt_vectors():
    known = {0: 0, 1: 0x514E28B7, 2: 0x30F4C306, 0xFFFFFFFF: 0x81F16F39, 0x9E3779B9: 0x92CA2F0E}
    assert [int(v) for v in ref.fmix32(np.array(list(known), np.uint64))] == list(known.values())
    assert ref.batch_salt(42, 3, 17) == 0xDA2897D6
    assert [ref.layer_salt(0xDA2897D6, i) for i in range(3)] == [0x4329F67E, 0x0C6EC80C, 0x14D8859C]
    assert ref.batch_salt(42 + (7 << 32), 3, 17) == 0xDA2897D6  # lo32(seed)


def test_type_code_and_no_rng_pool():
    import samgraph.torch as sam
    from xgnn_amd import ops
    assert sam.sample_types['khop_labor'] == sam.kKHopLabor == ops.KHOP_LABOR == KHOP_LABOR
    f = (C.c_size_t * 3)(15, 10, 5)
    assert lib().ggms_random_states_count(KHOP_LABOR, f, 3, 8000, 0) == 0
    assert lib().ggms_sample_workspace_bytes(KHOP_LABOR, 1000, 10) > 0
    assert lib().ggms_sample_batch_workspace_bytes(KHOP_LABOR, 1000, f, 3, None) > 0


def _distinct_ids(d, seed):
    return np.random.RandomState(seed).permutation(1 << 20)[:d].astype(np.uint32)


@pytest.mark.parametrize("ids,k", [(_distinct_ids(40, 1), 10), (_distinct_ids(64, 2), 5), (_distinct_ids(200, 3), 15),
                                   (_distinct_ids(33, 4), 32), (np.arange(1000, 1040, dtype=np.uint32), 10)],
                         ids=["40-10", "64-5", "200-15", "33-32", "consecutive-40-10"])
def test_each_position_is_selected_uniformly(ids, k):
    """Over the batch salts 0 .. 4095 (layer 0) every position of a list of distinct ids is selected 4096 k / d times,
    within 5 standard deviations of the binomial."""
    d, n = ids.size, 4096
    count = np.zeros(d, np.int64)
    for s in range(n):
        pos = ref.select_positions(ids, k, ref.layer_salt(s, 0))
        assert pos.size == k and np.all(np.diff(pos) > 0)
        count[pos] += 1
    p = k / d
    dev = np.abs(count - n * p) / np.sqrt(n * p * (1 - p))
    print(f"d {d} k {k}: worst deviation {dev.max():.2f} sd")
    assert dev.max() <= 5.0


def test_selection_rules_of_the_reference():
    ids = np.array([7] * 200 + [9, 11], np.uint32)  # multi-edges tie on the hash and break by position
    for salt in range(50):
        pos = ref.select_positions(ids, 5, salt)
        first7 = pos[pos < 200]
        assert np.array_equal(first7, np.arange(first7.size))
    assert np.array_equal(ref.select_positions(ids[:4], 5, 3), np.arange(4))
    assert ref.select_positions(ids[:0], 5, 3).size == 0


def test_leaf_argument_errors():
    l = lib()
    g = Graph()
    p = C.c_void_p(1 << 20)  # never dereferenced: the checks come first
    big = 1 << 30
    call = l.ggms_sample_khop_labor
    assert call(C.byref(g), p, 10, 0, 1, p, p, p, p, big, None) == INVALID          # fanout 0
    assert b"fanout" in l.ggms_last_error()
    assert call(C.byref(g), p, 10, 128, 1, p, p, p, p, big, None) == INVALID        # fanout beyond 127
    assert call(C.byref(g), p, 10, 5, 1, None, p, p, p, big, None) == INVALID       # no out_src
    assert call(C.byref(g), p, 10, 5, 1, p, None, p, p, big, None) == INVALID       # no out_dst
    assert call(C.byref(g), p, 10, 5, 1, p, p, None, p, big, None) == INVALID       # no count word
    assert call(C.byref(g), None, 10, 5, 1, p, p, p, p, big, None) == INVALID       # no input
    assert call(None, p, 10, 5, 1, p, p, p, p, big, None) == INVALID                # no graph
    need = l.ggms_sample_workspace_bytes(KHOP_LABOR, 10, 5)
    assert call(C.byref(g), p, 10, 5, 1, p, p, p, p, need - 4, None) == INVALID     # workspace too small
    assert call(C.byref(g), p, 10, 5, 1, p, p, p, None, big, None) == INVALID       # no workspace
    # the batch entry point takes the type (the next check, the workspace, is what refuses this call) and the
    # prefetching one keeps refusing it by name
    f = (C.c_size_t * 2)(5, 4)
    assert l.ggms_sample_batch_prefetch(KHOP_LABOR, None, None, 0, f, 2, None, None, 0, None, None, None, None, 0, None,
                                        None, None, 0, None) == INVALID
    assert b"sample type 8" in l.ggms_last_error()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("labor_ds"))


def test_arch1_takes_the_type(dataset):
    out = run_config(dataset["path"], dict(_sample_type=KHOP_LABOR))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


@pytest.mark.parametrize("arch,extra", [("arch0", ARCH0), ("arch4", dict(_arch=4, sampler_ctx='cuda:1', trainer_ctx='cuda:0'))])
def test_refused_by_key(dataset, arch, extra):
    out = run_config(dataset["path"], dict(extra, _sample_type=KHOP_LABOR))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert arch in out.stderr and "_sample_type" in out.stderr, out.stderr[-2000:]
