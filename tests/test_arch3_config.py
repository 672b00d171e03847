"""arch3 (one sampler GPU, one trainer GPU) at configuration time: what is accepted and what is refused
(GPUEngine::ArchCheck, cuda/cuda_engine.cc:410-435).  config + data_init touch no GPU, so all of this runs anywhere."""
import os
import subprocess
import sys

import pytest

from test_engine import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("arch3_ds"))


def _run(path, extra, env=None):
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import samgraph.torch as sam
cfg = {{'dataset_path': {path!r}, '_arch': sam.kArch3, '_sample_type': sam.kKHop3, 'batch_size': 64, 'num_epoch': 1,
  '_cache_policy': sam.kCacheByDegree, 'cache_percentage': 0.3, 'max_sampling_jobs': 1, 'max_copying_jobs': 1,
  'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2, 'fanout': [5, 4],
  'sampler_ctx': 'cuda:0', 'trainer_ctx': 'cuda:1'}}
cfg.update({extra!r})
sam.config(cfg)
sam.data_init()
print('configured', sam.num_class(), sam.feat_dim())
"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                          env=dict(base, **(env or {})))


@pytest.mark.parametrize("env", [{}, {"SAMGRAPH_FORCE_DEVICE": "0"}])
@pytest.mark.parametrize("extra", [{}, {"cache_percentage": 0.0}, {"_cache_policy": 2, "presample_epoch": 1},
                                   {"sampler_ctx": "cuda:3", "trainer_ctx": "cuda:1"}])
def test_arch3_config_and_data_init_pass(dataset, extra, env):
    """The builtin arch3 contexts (cuda:0 samples, cuda:1 trains) pass config and data_init, with and without the
    one-GPU rehearsal hook, which maps both contexts onto one device AFTER they have been compared."""
    out = _run(dataset["path"], extra, env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


@pytest.mark.parametrize("extra,env,message", [
    ({"trainer_ctx": "cuda:0"}, {}, "sampler_ctx and trainer_ctx are the same GPU (cuda:0)"),
    ({"sampler_ctx": "cuda:1"}, {"SAMGRAPH_FORCE_DEVICE": "0"}, "sampler_ctx and trainer_ctx are the same GPU (cuda:1)"),
    ({"sampler_ctx": "cpu:0"}, {}, "must both be GPU contexts (cuda:N), got cpu:0 and cuda:1"),
    ({"trainer_ctx": "cpu:0"}, {}, "must both be GPU contexts (cuda:N), got cuda:0 and cpu:0"),
    ({"part_cache": "True"}, {}, "arch3: part_cache is an arch6 key"),
    ({"gpu_extract": "True"}, {}, "arch3: gpu_extract is an arch6 key"),
    ({"use_dist_graph": 0.5}, {}, "arch3: use_dist_graph is an arch6 key"),
    ({}, {"SAMGRAPH_LOG_NODE_ACCESS_SIMPLE": "1"}, "a GPU cache (cache_percentage > 0) cannot be combined with node access"),
    ({}, {"SAMGRAPH_LOG_NODE_ACCESS": "1"}, "a GPU cache (cache_percentage > 0) cannot be combined with node access"),
])
def test_arch3_refusals(dataset, extra, env, message):
    """Each refusal ends the process at config with a message (a failed CHECK aborts, logging.cc:69-73)."""
    out = _run(dataset["path"], extra, env)
    assert out.returncode != 0 and "configured" not in out.stdout
    assert message in out.stderr, out.stderr[-2000:]


def test_arch3_node_access_logging_without_a_cache_is_accepted(dataset):
    """Node access logging is refused only together with a GPU cache, as in the reference."""
    out = _run(dataset["path"], {"cache_percentage": 0.0}, {"SAMGRAPH_LOG_NODE_ACCESS_SIMPLE": "1"})
    assert out.returncode == 0, out.stderr[-2000:]
