"""config + data_init on the host, in a process of their own (a refused configuration aborts it): shared by the config
tests of the feature-table formats."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {'_arch': 1, 'sampler_ctx': 'cuda:0', 'trainer_ctx': 'cuda:0', '_sample_type': 0, 'batch_size': 64,
        'num_epoch': 1, '_cache_policy': 0, 'cache_percentage': 0.0, 'max_sampling_jobs': 1, 'max_copying_jobs': 1,
        'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2,
        'fanout': [5, 4]}
ARCH0 = dict(_arch=0, sampler_ctx='cpu:0', trainer_ctx='cpu:0')


def run_config(path, extra, tail="", env_extra=None):
    """BASE + `extra` on the dataset at `path`: the completed process, which printed 'configured <classes> <dim>' (and
    ran `tail`, a piece of Python that may use `sam`) if the engine took the configuration."""
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
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
