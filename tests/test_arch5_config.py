"""arch5 (sampler processes + trainer processes joined by a batch queue) at configuration time: what is accepted and
what is refused (operation.cc:112-121), steps_per_epoch() after data_init, and the DistShuffler's slice rule
(dist/dist_shuffler.cc:37-90) as a Python twin.  config + data_init touch no GPU, so all of this runs anywhere."""
import os
import subprocess
import sys

import pytest

from test_engine import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dist_shuffler_slices(num_data, batch_size, num_sampler):
    """Per sampler: (first global step, number of steps, first train-set position, number of seeds).  An epoch has
    ceil(num_data / batch_size) steps (drop_last false); the first (steps % S) samplers take one step more, and every
    slice ends at the train set (the last batch of an epoch may be short)."""
    steps = (num_data + batch_size - 1) // batch_size
    large, small = steps % num_sampler, steps // num_sampler
    out = []
    for w in range(num_sampler):
        n = small + 1 if w < large else small
        first = (small + 1) * w if w < large else small * w + large
        data_off = first * batch_size
        out.append((first, n, data_off, max(0, min(n * batch_size, num_data - data_off))))
    return out


def test_dist_shuffler_twin_hand_worked():
    # 15 steps over 4 samplers: 4, 4, 4, 3 (the reference's own comment, dist_shuffler.cc:59-65)
    assert [s[1] for s in dist_shuffler_slices(15 * 10, 10, 4)] == [4, 4, 4, 3]
    assert [s[0] for s in dist_shuffler_slices(15 * 10, 10, 4)] == [0, 4, 8, 12]
    # a short last batch belongs to the last sampler: 143 seeds in batches of 10 = 15 steps, the last one of 3
    assert dist_shuffler_slices(143, 10, 4) == [(0, 4, 0, 40), (4, 4, 40, 40), (8, 4, 80, 40), (12, 3, 120, 23)]
    # one sampler: the whole epoch
    assert dist_shuffler_slices(143, 10, 1) == [(0, 15, 0, 143)]
    # more samplers than steps: 3 steps over 5 samplers, the last two idle; the third's slice ends at the train set
    assert dist_shuffler_slices(21, 10, 5) == [(0, 1, 0, 10), (1, 1, 10, 10), (2, 1, 20, 1), (3, 0, 30, 0),
                                               (3, 0, 30, 0)]
    # every step exactly once, in order
    for n, bs, S in [(500, 64, 1), (500, 64, 2), (500, 64, 3), (500, 64, 8), (64, 64, 3), (1, 7, 2)]:
        sl = dist_shuffler_slices(n, bs, S)
        assert [s[0] for s in sl] == [sum(x[1] for x in sl[:w]) for w in range(S)]
        assert sum(s[1] for s in sl) == (n + bs - 1) // bs and sum(s[3] for s in sl) == n


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("arch5_ds"))


def _run(path, extra, env=None):
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import samgraph.torch as sam
cfg = {{'dataset_path': {path!r}, '_arch': sam.kArch5, '_sample_type': sam.kKHop3, 'batch_size': 64, 'num_epoch': 1,
  '_cache_policy': sam.kCacheByDegree, 'cache_percentage': 0.3, 'max_sampling_jobs': 1, 'max_copying_jobs': 1,
  'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5, 'num_fanout': 2, 'fanout': [5, 4],
  'num_sample_worker': 2, 'num_train_worker': 2}}
cfg.update({extra!r})
for k in [k for k, v in cfg.items() if v is None]:
    del cfg[k]
sam.config(cfg)
sam.data_init()
print('configured', sam.num_class(), sam.feat_dim(), sam.steps_per_epoch(), sam.num_epoch())
"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("SAMGRAPH_")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                          env=dict(base, **(env or {})))


@pytest.mark.parametrize("extra", [{}, {"have_switcher": 0}, {"cache_percentage": 0.0}, {"cache_percentage": 1.0},
                                   {"_cache_policy": 2, "presample_epoch": 1}, {"queue_depth": 1},
                                   {"queue_depth": 9, "queue_timeout_s": 2.5}, {"unified_memory": "False"},
                                   {"num_sample_worker": 1, "num_train_worker": 15},
                                   {"sampler_ctx": None, "trainer_ctx": None, "part_cache": "False"},
                                   {"_sample_type": 3, "num_fanout": None, "fanout": None, "random_walk_length": 3,
                                    "random_walk_restart_prob": 0.5, "num_random_walk": 4, "num_neighbor": 5}])
def test_arch5_config_and_data_init_pass(dataset, extra):
    """The multi_gpu scripts' keys pass config and data_init (no GPU touched); steps_per_epoch() is then
    ceil(num_train / batch_size) = ceil(500 / 64) = 8 (dist_engine.cc:139-142)."""
    out = _run(dataset["path"], extra)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20", "8", "1"]


def test_arch5_steps_per_epoch_is_not_padded(dataset):
    """No alignment to the worker count (that is arch6's DistAlignedShuffler): 500 seeds in batches of 100 = 5 steps
    whatever S and T are."""
    for s, t in [(1, 1), (2, 1), (3, 4), (4, 3)]:
        out = _run(dataset["path"], {"batch_size": 100, "num_sample_worker": s, "num_train_worker": t})
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split()[3] == "5"


@pytest.mark.parametrize("extra,message", [
    ({"have_switcher": 1}, "arch5: have_switcher = 1: the switcher is not built"),
    ({"part_cache": "True"}, "arch5: part_cache is an arch6 key"),
    ({"gpu_extract": "True"}, "arch5: gpu_extract is an arch6 key"),
    ({"use_dist_graph": 0.5}, "arch5: use_dist_graph is an arch6 key"),
    ({"unified_memory": "True"}, "arch5: unified_memory is not built"),
    ({"num_sample_worker": 9, "num_train_worker": 8}, "arch5: num_sample_worker + num_train_worker = 17: at most 16"),
    ({"num_sample_worker": 0}, "arch5: num_sample_worker and num_train_worker must both be >= 1"),
    ({"num_train_worker": 0}, "arch5: num_sample_worker and num_train_worker must both be >= 1"),
    ({"num_train_worker": None}, "arch5 needs num_sample_worker/num_train_worker"),
    ({"queue_depth": 0}, "arch5: queue_depth = 0"),
    ({"queue_timeout_s": 0}, "arch5: queue_timeout_s = 0"),
])
def test_arch5_refusals(dataset, extra, message):
    """Each refusal ends the process at config with a message that names the key."""
    out = _run(dataset["path"], extra)
    assert out.returncode != 0 and "configured" not in out.stdout
    assert message in out.stderr, out.stderr[-2000:]
