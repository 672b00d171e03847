"""Config keys induced_subgraph / induced_max_edges on the host: which configurations config + data_init take (no GPU
touched), every refusal by name, and the default capacity."""
import re

import numpy as np
import pytest

from config_run import ARCH0, BASE, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen
from xgnn_amd._lib import lib

ON = dict(induced_subgraph="on")
INFO = dict(SAMGRAPH_LOG_LEVEL="info")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    path = tmp_path_factory.mktemp("induced_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(path), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13,
                          weights=np.ones(ix.size, np.float32), edge_feat=feature_rows(np.arange(ix.size), 3, np.float32),
                          edge_time=np.zeros(ix.size, np.uint32))
    return dict(path=str(path), num_edge=int(ix.size))


ACCEPTED = [
    ("on", ON),
    ("off-elsewhere", dict(induced_subgraph="off", _arch=3, trainer_ctx="cuda:1")),  # off: nothing is asked for
    ("capacity", dict(ON, induced_max_edges=12345)),
    ("largest-capacity", dict(ON, induced_max_edges=2 ** 32 - 1025)),
    ("edge_feat", dict(ON, edge_feat="on")),
    ("khop3", dict(ON, _sample_type=7)),
    ("khop_labor-hashed", dict(ON, _sample_type=8, hash_table="hashed")),
    ("link", dict(ON, task="link_prediction", exclude_seed_edges="none")),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(dataset, case):
    out = run_config(dataset["path"], case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("arch0", dict(ARCH0, **ON), ["arch0", "induced_subgraph is not built"]),
    ("arch3", dict(ON, _arch=3, trainer_ctx="cuda:1"), ["arch3", "induced_subgraph is not built"]),
    ("arch4", dict(ON, _arch=4, sampler_ctx="cuda:1"), ["arch4", "induced_subgraph is not built"]),
    ("arch5", dict(ON, _arch=5, num_sample_worker=1, num_train_worker=1), ["arch5", "induced_subgraph is not built"]),
    ("arch6", dict(ON, _arch=6, num_worker=1), ["arch6", "induced_subgraph is not built"]),
    ("dist-graph", dict(ON, use_dist_graph=0.5), ["induced_subgraph", "use_dist_graph", "ONE CSR"]),
    ("khop2", dict(ON, _sample_type=5), ["induced_subgraph", "khop2", "permutes indices"]),
    ("khop_temporal", dict(ON, _sample_type=9, task="link_prediction"), ["induced_subgraph", "khop_temporal", "leaks"]),
    ("exclude-self", dict(ON, task="link_prediction", exclude_seed_edges="self"),
     ["induced_subgraph with exclude_seed_edges = self", "does not compact an id stream", "holds its positive edges"]),
    ("exclude-both", dict(ON, task="link_prediction", exclude_seed_edges="both"),
     ["induced_subgraph with exclude_seed_edges = both", "does not compact an id stream", "holds its positive edges"]),
    ("capacity-0", dict(ON, induced_max_edges=0), ["induced_max_edges = 0", "1 .. 2^32 - 1025"]),
    ("capacity-2^32-1024", dict(ON, induced_max_edges=2 ** 32 - 1024), ["induced_max_edges = 4294966272", "1 .. 2^32 - 1025"]),
    ("capacity-2^40", dict(ON, induced_max_edges=2 ** 40), ["induced_max_edges = ", "1 .. 2^32 - 1025"]),
    ("capacity-word", dict(ON, induced_max_edges="many"), ["induced_max_edges = many"]),
    ("capacity-alone", dict(induced_max_edges=100), ["induced_max_edges without induced_subgraph = on"]),
    ("bad-value", dict(induced_subgraph="yes"), ["induced_subgraph = yes", "on or off"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(dataset, case):
    _, extra, words = case
    out = run_config(dataset["path"], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def layer_capacities(num_seeds, fanout):
    L = len(fanout)
    import ctypes as C
    c_f = (C.c_size_t * L)(*fanout)
    max_in, max_e, max_u = (C.c_size_t * L)(), (C.c_size_t * L)(), C.c_size_t()
    assert lib().ggms_sample_batch_capacity(num_seeds, c_f, L, max_in, max_e, C.byref(max_u)) == 0
    return list(max_e)


def capacity_of(out):
    m = re.search(r"induced_subgraph: induced_max_edges = (\d+) \((config|default)", out.stderr)
    assert out.returncode == 0 and m, out.stderr[-2000:]
    return int(m.group(1)), m.group(2)


def test_default_capacity_is_the_layers_capacity_capped_at_num_edge(dataset):
    """The sum of the layers' edge capacities at the batch bounds; on a graph with fewer edges than that, NUM_EDGE."""
    seeds = int(BASE["batch_size"] * 1.25) + 1  # the engine's seed bound
    want = sum(layer_capacities(seeds, BASE["fanout"]))
    assert 0 < want < dataset["num_edge"]
    assert capacity_of(run_config(dataset["path"], ON, env_extra=INFO)) == (want, "default")
    big = dict(ON, batch_size=200, fanout=[15, 10])
    assert sum(layer_capacities(251, [15, 10])) > dataset["num_edge"]
    assert capacity_of(run_config(dataset["path"], big, env_extra=INFO)) == (dataset["num_edge"], "default")
    assert capacity_of(run_config(dataset["path"], dict(ON, induced_max_edges=777), env_extra=INFO)) == (777, "config")
    link = dict(ON, task="link_prediction", num_negative=3)  # the seed list: endpoints and negatives
    want = min(sum(layer_capacities(BASE["batch_size"] * 5, BASE["fanout"])), dataset["num_edge"])
    assert capacity_of(run_config(dataset["path"], link, env_extra=INFO)) == (want, "default")
