"""sample_type random_walk_metapath on the host: its code in the three Python tables, what config + data_init take and
refuse by name (no GPU touched), and the C argument checks: GGMS_ERR_INVALID with a message before any device call."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import khop_typed_ref as typed
from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import _lib, datagen, lib

NAME = "random_walk_metapath"
W12 = dict(_sample_type=12, metapath=[0, 1], random_walk_length=2, random_walk_restart_prob=0.5, num_random_walk=3,
           num_neighbor=4)


def test_python_names():
    import samgraph.torch as sam
    from xgnn_amd import common, ops
    assert sam.sample_types[NAME] == common.kRandomWalkMetapath == ops.RANDOM_WALK_METAPATH == 12
    assert callable(ops.sample_walk_metapath) and callable(ops.WalkMetapathBatchSampler)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("walk_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(root / "ok"), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13,
                          edge_type=typed.sorted_types(ip, np.random.RandomState(2), 3), num_edge_type=3)
    shutil.copytree(root / "ok", root / "none")
    os.remove(root / "none" / "edge_type.bin")
    return dict(ok=str(root / "ok"), none=str(root / "none"))


@pytest.mark.parametrize("extra", [{}, dict(hash_table="hashed", pipelines=2), dict(metapath=[2] * 8)], ids=str)
def test_accepted(datasets, extra):
    out = run_config(datasets["ok"], dict(W12, **extra))
    assert out.returncode == 0 and out.stdout.split() == ["configured", "13", "20"], out.stderr[-2000:]


OTHER_ARCH = dict(arch0=ARCH0, arch3=dict(_arch=3, trainer_ctx="cuda:1"), arch4=dict(_arch=4, sampler_ctx="cuda:1"),
                  arch5=dict(_arch=5, num_sample_worker=1, num_train_worker=1), arch6=dict(_arch=6, num_worker=1))
REFUSED = [(a, "ok", dict(W12, **kw), [a, NAME, "arch1's sampling chain"]) for a, kw in OTHER_ARCH.items()] + [
    ("dist-graph", "ok", dict(W12, use_dist_graph=0.5), [NAME, "use_dist_graph", "ONE CSR"]),
    ("no-file", "none", W12, [NAME, "edge_type.bin is missing"]),
    ("no-key", "ok", {k: v for k, v in W12.items() if k != "metapath"}, [NAME, "needs the config key metapath"]),
    ("empty", "ok", dict(W12, metapath=""), ["metapath has 0 relation ids"]),
    ("nine", "ok", dict(W12, metapath=[0] * 9), ["metapath has 9 relation ids", "1 .. 8"]),
    ("not-a-relation", "ok", dict(W12, metapath=[0, 3]), ["metapath: entry 1 is the relation 3", "NUM_EDGE_TYPE is 3"]),
    ("out-of-range", "ok", dict(W12, metapath=[0, 40]), ["metapath: the value 40 is out of range"]),
    ("hetero_batch", "ok", dict(W12, hetero_batch="on"), ["hetero_batch with _sample_type 12", "khop_typed"]),
    ("typed_feat", "ok", dict(W12, typed_feat="on"), ["typed_feat without hetero_batch"]),
    ("inline_heads", "ok", dict(W12, inline_heads=1), [NAME, "inline_heads = 1"]),
    ("link_prediction", "ok", dict(W12, task="link_prediction"), ["task = link_prediction", NAME]),  # random_walk's
    ("edge_ids", "ok", dict(W12, edge_ids="on"), ["edge_ids", NAME]),                                 # random_walk's
    ("restart_prob", "ok", dict(W12, random_walk_restart_prob=1.5), ["random_walk_restart_prob = 1.5"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


C_REFUSED = [(dict(num_part=2), "unsharded"), (dict(edge_type=None), "edge_type is NULL"), (dict(R=0), "num_type 0"),
             (dict(R=33), "num_type 33"), (dict(path=[]), "metapath_len 0"), (dict(path=[0] * 9), "metapath_len 9"),
             (dict(path=[0, 3]), "metapath[1] = 3"), (dict(T=0), "num_traversal 0"), (dict(W=0), "num_walk 0"),
             (dict(K=0), "K 0"), (dict(p=-0.25), "restart_prob"), (dict(p=1.5), "restart_prob"),
             (dict(p=float("nan")), "restart_prob"), (dict(ws=64), "workspace_bytes 64")]


@pytest.mark.parametrize("case", C_REFUSED, ids=[c[1].replace(" ", "-") for c in C_REFUSED])
def test_c_argument_checks_touch_no_device(case):
    """Every pointer is a made-up address: a call that went past its checks would fault or report a HIP error."""
    a = dict(num_part=0, edge_type=0x1000, R=3, path=[0, 1], T=2, W=3, K=4, p=0.5, ws=None)
    a.update(case[0])
    h, fake = lib(), C.c_void_p(0x1000)
    need = h.ggms_sample_walk_metapath_workspace_bytes(10, a["T"], a["W"], a["K"])
    g = _lib.Graph(0x1000, 0x1000, None, None, a["num_part"], 0, 100, 0)
    path = (C.c_uint32 * max(len(a["path"]), 1))(*a["path"])
    rc = h.ggms_sample_walk_metapath(C.byref(g), a["edge_type"], a["R"], path, len(a["path"]), fake, 10, a["T"], a["p"],
                                     a["W"], a["K"], 7, fake, fake, fake, fake, fake, need if a["ws"] is None else a["ws"],
                                     None)
    assert rc == -1 and case[1] in h.ggms_last_error().decode(), h.ggms_last_error().decode()  # GGMS_ERR_INVALID
