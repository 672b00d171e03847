"""arch4 on the host: which configurations config + data_init take (no GPU touched) and which they refuse, naming the key;
the host arithmetic of the prefetching sampler's capacity and workspace rules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_engine import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {'_arch': 4, 'sampler_ctx': 'cuda:1', 'trainer_ctx': 'cuda:0', '_sample_type': 0, 'batch_size': 64,
        'num_epoch': 1, '_cache_policy': 0, 'cache_percentage': 0.0, 'max_sampling_jobs': 1, 'max_copying_jobs': 1,
        'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2,
        'fanout': [5, 4]}
KHOP0, KHOP1, WEIGHTED_KHOP, RANDOM_WALK, PREFIX, KHOP2, HASH_DEDUP, KHOP3 = range(8)
DYNAMIC, DEGREE = 6, 0


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from xgnn_amd import datagen
    d = make_dataset(tmp_path_factory.mktemp("arch4_ds"))
    g = dict(indptr=d["ip"], indices=d["ix"], train_set=d["train"], meta=dict(feat_dim=d["feat"].shape[1], num_class=13))
    datagen.write_dataset(d["path"], g, feat=d["feat"], label=d["label"], weights=datagen.edge_weights(g, "default", seed=3))
    return d


def _run(path, extra=None):
    cfg = dict(BASE, dataset_path=path)
    cfg.update(extra or {})
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import samgraph.torch as sam
sam.config({cfg!r})
sam.data_init()
print('configured', sam.num_class(), sam.feat_dim())
"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)


def _layers(n):
    return {'num_layer': n, 'num_fanout': n, 'fanout': [5, 4, 3][:n]}


@pytest.mark.parametrize("sample_type", [KHOP0, KHOP1, WEIGHTED_KHOP])
@pytest.mark.parametrize("num_layer", [2, 3])
@pytest.mark.parametrize("policy", [DEGREE, DYNAMIC])
def test_arch4_accepted(dataset, sample_type, num_layer, policy):
    """khop0 / khop1 / weighted_khop over 2 and 3 layers, with and without dynamic_cache (cache_percentage 0)."""
    out = _run(dataset["path"], dict(_sample_type=sample_type, _cache_policy=policy, **_layers(num_layer)))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("same-context", dict(sampler_ctx='cuda:0', trainer_ctx='cuda:0'), "sampler_ctx"),
    ("cpu-context", dict(sampler_ctx='cpu:0'), "sampler_ctx"),
    ("one-layer", _layers(1), "num_layer"),
    ("khop2", dict(_sample_type=KHOP2), "_sample_type"),
    ("khop3", dict(_sample_type=KHOP3), "_sample_type"),
    ("random-walk", dict(_sample_type=RANDOM_WALK, random_walk_length=3, random_walk_restart_prob=0.5,
                         num_random_walk=4, num_neighbor=5), "_sample_type"),
    ("prefix", dict(_sample_type=PREFIX), "_sample_type"),
    ("hash-dedup", dict(_sample_type=HASH_DEDUP), "_sample_type"),
    ("dynamic-with-cache", dict(_cache_policy=DYNAMIC, cache_percentage=0.2), "cache_percentage"),
    ("static-cache", dict(_cache_policy=DEGREE, cache_percentage=0.2), "cache_percentage"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_arch4_refused_by_key(dataset, case):
    _, extra, key = case
    out = _run(dataset["path"], extra)
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "arch4" in out.stderr and key in out.stderr, out.stderr[-2000:]


def _capacity(h, num_seeds, fanouts, ip, budget):
    f = (C.c_size_t * len(fanouts))(*fanouts)
    ip = np.ascontiguousarray(ip, dtype=np.uint32)
    me, mi = C.c_size_t(0), C.c_size_t(0)
    rc = h.ggms_sample_batch_prefetch_capacity(num_seeds, f, len(fanouts), ip.ctypes.data_as(C.c_void_p), ip.size - 1,
                                               budget, C.byref(me), C.byref(mi))
    return rc, me.value, mi.value


def test_prefetch_capacity_rule_is_host_arithmetic():
    """k = the unique bound after L - 1 layers (capped at N); edges = min(sum of the k largest degrees, budget);
    input nodes = min(N, k + edges).  Refused below 2 layers."""
    from xgnn_amd import lib
    h = lib()
    rs = np.random.RandomState(3)
    for N, seeds, fan in [(1000, 10, [5, 4]), (50, 30, [3, 2]), (100000, 64, [10, 5, 3]), (7, 1, [1, 1])]:
        deg = rs.zipf(1.8, N).clip(0, 5000).astype(np.uint64)
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
        k = seeds
        for f in fan[1:][::-1]:  # layers L-1 .. 1 (fanouts indexed by layer id)
            k += k * f
        k = min(k, N)
        top = int(np.sort(deg)[::-1][:k].sum())
        for budget in [0, 1, top // 2, top, top + 10, 1 << 40]:
            rc, me, mi = _capacity(h, seeds, fan, ip, budget)
            assert rc == 0
            assert me == min(top, budget), (N, budget)
            assert mi == min(N, k + me), (N, budget)
    rc, _, _ = _capacity(h, 10, [5], np.array([0, 1], np.uint32), 10)
    assert rc == -1


def test_prefetch_workspace_rule_is_host_arithmetic():
    """The workspace grows with the expansion's capacity (keys, their ids, the fill's scratch: >= 16 B per edge) and
    exceeds the plain batch's; below 2 layers there is none."""
    from xgnn_amd import lib
    from xgnn_amd._lib import SampleExtra
    h = lib()
    f = (C.c_size_t * 2)(5, 4)
    ex = SampleExtra()
    plain = h.ggms_sample_batch_workspace_bytes(KHOP0, 81, f, 2, C.byref(ex))
    prev = 0
    for e in [0, 1, 1000, 1 << 20, 1 << 24]:
        ws = h.ggms_sample_batch_prefetch_workspace_bytes(KHOP0, 81, f, 2, C.byref(ex), e)
        assert ws > plain and ws >= prev and ws >= 16 * e
        prev = ws
    assert h.ggms_sample_batch_prefetch_workspace_bytes(KHOP0, 81, (C.c_size_t * 1)(5), 1, C.byref(ex), 100) == 0


@pytest.mark.parametrize("sample_type,num_layer,what", [(KHOP3, 2, b"sample type"), (KHOP2, 2, b"sample type"),
                                                        (RANDOM_WALK, 2, b"sample type"), (KHOP0, 1, b"num_layer")])
def test_prefetch_sampler_refuses_without_a_gpu(sample_type, num_layer, what):
    """Argument errors named in ggms_last_error before anything is enqueued."""
    from xgnn_amd import lib
    h = lib()
    f = (C.c_size_t * 2)(5, 4)
    rc = h.ggms_sample_batch_prefetch(sample_type, None, None, 0, f, num_layer, None, None, 0, None, None, None, None,
                                      0, None, None, None, 0, None)
    assert rc == -1
    assert what in h.ggms_last_error()
