"""presample_static on the host: the closure operator's workspace rule (host arithmetic, no GPU), and which deployments
take the policy at config + data_init (no GPU touched) and which refuse it, naming it."""
import os
import subprocess
import sys

import pytest

from test_engine import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {'_sample_type': 7, 'batch_size': 64, 'num_epoch': 1, '_cache_policy': 4, 'cache_percentage': 0.3,
        'presample_epoch': 1, 'max_sampling_jobs': 1, 'max_copying_jobs': 1, 'omp_thread_num': 1, 'num_layer': 2,
        'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2, 'fanout': [5, 4]}
ARCH = {
    0: {'_arch': 0, 'sampler_ctx': 'cpu:0', 'trainer_ctx': 'cpu:0'},
    3: {'_arch': 3, 'sampler_ctx': 'cuda:0', 'trainer_ctx': 'cuda:1'},
    5: {'_arch': 5, 'num_sample_worker': 2, 'num_train_worker': 2},
    6: {'_arch': 6, 'num_worker': 2, 'part_cache': 'True', 'gpu_extract': 'True'},
}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("presample_static_ds"))


def _run(path, arch, extra=None):
    cfg = dict(BASE, dataset_path=path, **ARCH[arch])
    cfg.update(extra or {})
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import samgraph.torch as sam
sam.config({cfg!r})
sam.data_init()
print('configured', sam.num_class(), sam.feat_dim())
"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=base)


def test_closure_workspace_rule_is_host_only():
    """Exported and pure host arithmetic: at least the frontier's edge prefix (one word per node) plus the scratch of
    the degree scan (8 control words, one 64-bit descriptor per 1024-node tile, tile sums and prefixes)."""
    from xgnn_amd import lib
    h = lib()
    prev = 0
    for n in [0, 1, 1000, 1024, 1025, 4096, 300_000, 111_059_956, (1 << 32) - 1]:
        tiles = (n + 1023) // 1024
        ws = h.ggms_khop_closure_workspace_bytes(n)
        assert ws >= 4 * n + 4 * (12 + 4 * (tiles + 1)), n
        assert ws >= prev
        prev = ws


def test_closure_refuses_bad_arguments_without_a_gpu():
    """A zero stamp (the value every word of a fresh visit array holds) and a short workspace are argument errors,
    reported before anything is enqueued."""
    import ctypes as C
    from xgnn_amd import lib
    from xgnn_amd._lib import Graph
    h = lib()
    g = Graph()
    g.num_node = 100
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert h.ggms_khop_closure(C.byref(g), None, 0, 2, p, 0, None, p, p, p, 64 * 8, None) == -1
    assert b"stamp" in h.ggms_last_error()
    assert h.ggms_khop_closure(C.byref(g), None, 0, 2, p, 1, None, p, p, p, 8, None) == -1
    assert b"workspace_bytes" in h.ggms_last_error()


@pytest.mark.parametrize("arch", [3, 5, 6])
def test_presample_static_passes_config_and_data_init(dataset, arch):
    """The deployments that rank on a GPU take cache_policy = presample_static."""
    out = _run(dataset["path"], arch)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


def test_arch0_refuses_presample_static(dataset):
    """The CPU engine has no closure kernel (the reference's cpu/cpu_engine.cc:159 refuses it too)."""
    out = _run(dataset["path"], 0)
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "presample_static" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("arch", [0, 3, 5, 6])
def test_dynamic_cache_is_refused(dataset, arch):
    """dynamic_cache needs arch4 and a per-batch cache replacement manager: refused everywhere, by name."""
    out = _run(dataset["path"], arch, {'_cache_policy': 6})
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "dynamic" in out.stderr, out.stderr[-2000:]
