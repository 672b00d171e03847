"""sample_type khop_typed_temporal on the host: its code in the three Python tables, what config + data_init take and
refuse by name (no GPU touched), datagen's (type, time) order, and the C argument checks: GGMS_ERR_INVALID with a message
before any device call."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import _lib, datagen, lib

NAME = "khop_typed_temporal"
T13 = dict(_sample_type=13, type_fanout=[[3, 1, 1], [2, 2, 0]], task="link_prediction")


def test_python_names():
    import samgraph.torch as sam
    from xgnn_amd import common, ops
    assert sam.sample_types[NAME] == common.kKHopTypedTemporal == ops.KHOP_TYPED_TEMPORAL == 13
    assert callable(ops.sample_khop_typed_temporal) and callable(ops.TypedTemporalBatchSampler)
    assert all(name in _lib.SYMBOLS for name in (
        "ggms_sample_khop_typed_temporal", "ggms_sample_khop_typed_temporal_workspace_bytes",
        "ggms_sample_batch_typed_temporal", "ggms_sample_batch_typed_temporal_workspace_bytes"))


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("tt_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    rng = np.random.RandomState(2)
    # unsorted arrays through datagen.sort_lists_by_type_time: the CSR the sampler wants
    ix, et, tm, perm = datagen.sort_lists_by_type_time(ip, ix, rng.randint(0, 3, ix.size), rng.randint(1, 500, ix.size))
    assert perm.size == ix.size
    assert datagen.first_unsorted_list(ip, et) is None and datagen.first_unsorted_segment(ip, et, tm) is None
    assert datagen.first_unsorted_list(ip, tm) is not None  # the whole lists are NOT sorted by time
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    kw = dict(feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13, edge_type=et, num_edge_type=3)
    datagen.write_dataset(str(root / "ok"), g, edge_time=tm, **kw)
    for name, gone in (("no_time", "edge_time.bin"), ("no_type", "edge_type.bin")):
        shutil.copytree(root / "ok", root / name)
        os.remove(root / name / gone)
    # one segment's times out of order: datagen refuses it by node and position, and so does the engine
    v = next(v for v in range(600) if ip[v + 1] - ip[v] >= 2 and et[ip[v]] == et[ip[v] + 1] and tm[ip[v]] != tm[ip[v] + 1])
    bad = tm.copy()
    bad[ip[v]], bad[ip[v] + 1] = tm[ip[v] + 1], tm[ip[v]]
    with pytest.raises(AssertionError, match=f"node {v}'s list.*position {ip[v] + 1}.*sort_lists_by_type_time"):
        datagen.write_dataset(str(root / "bad"), g, edge_time=bad, **kw)
    shutil.copytree(root / "ok", root / "unsorted")
    bad.tofile(root / "unsorted" / "edge_time.bin")
    return dict(ok=str(root / "ok"), no_time=str(root / "no_time"), no_type=str(root / "no_type"),
                unsorted=str(root / "unsorted"), unsorted_at=(v, int(ip[v]) + 1))


@pytest.mark.parametrize("extra", [{}, dict(temporal_pick="recent", hash_table="hashed", pipelines=2)], ids=str)
def test_accepted(datasets, extra):
    out = run_config(datasets["ok"], dict(T13, **extra))
    assert out.returncode == 0 and out.stdout.split() == ["configured", "13", "20"], out.stderr[-2000:]


OTHER_ARCH = dict(arch0=ARCH0, arch3=dict(_arch=3, trainer_ctx="cuda:1"), arch4=dict(_arch=4, sampler_ctx="cuda:1"),
                  arch5=dict(_arch=5, num_sample_worker=1, num_train_worker=1), arch6=dict(_arch=6, num_worker=1))
REFUSED = [(a, "ok", dict(T13, **kw), [a, NAME, "arch1's sampling chain"]) for a, kw in OTHER_ARCH.items()] + [
    ("dist-graph", "ok", dict(T13, use_dist_graph=0.5), [NAME, "use_dist_graph", "ONE CSR"]),
    ("exclude", "ok", dict(T13, exclude_seed_edges="self"), [NAME, "exclude_seed_edges = self", "strictly-before"]),
    ("induced", "ok", dict(T13, induced_subgraph="on"), ["induced_subgraph", NAME, "leaks the future"]),
    ("inline_heads", "ok", dict(T13, inline_heads=1), [NAME, "inline_heads = 1"]),
    ("node_classification", "ok", dict(T13, task="node_classification"), [NAME, "needs task = link_prediction"]),
    ("no-key", "ok", {k: v for k, v in T13.items() if k != "type_fanout"}, [NAME, "needs the config key type_fanout"]),
    ("pick", "ok", dict(T13, temporal_pick="latest"), ["temporal_pick = latest"]),
    ("no-time-file", "no_time", T13, [NAME, "edge_time.bin is missing"]),
    ("no-type-file", "no_type", T13, [NAME, "edge_type.bin is missing"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(datasets, case):
    _, ds, extra, words = case
    out = run_config(datasets[ds], extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


def test_times_out_of_order_in_a_segment_are_named(datasets):
    v, p = datasets["unsorted_at"]
    out = run_config(datasets["unsorted"], T13)
    assert out.returncode < 0 and "configured" not in out.stdout
    for w in (NAME, f"the times of node {v}'s list", f"(position {p})", "datagen.sort_lists_by_type_time"):
        assert w in out.stderr, (w, out.stderr[-2000:])


C_REFUSED = [(dict(num_part=2), "num_part == 0"), (dict(edge_type=None), "edge_type"), (dict(edge_time=None), "edge_time"),
             (dict(R=0), "num_type >= 1"), (dict(R=33), "num_type >= 1"), (dict(tf=[1, 128, 1]), "kLaborMaxFanout"),
             (dict(tf=[0, 0, 0]), "fanout > 0"), (dict(pick=2), "GGMS_PICK_RECENT"), (dict(ws=64), "workspace_bytes")]


@pytest.mark.parametrize("case", C_REFUSED, ids=[str(sorted(c[0].items())[0]) for c in C_REFUSED])
def test_c_argument_checks_touch_no_device(case):
    """Every pointer is a made-up address: a call that went past its checks would fault or report a HIP error."""
    a = dict(num_part=0, edge_type=0x1000, edge_time=0x1000, R=3, tf=[2, 1, 1], pick=0, ws=None)
    a.update(case[0])
    h, fake = lib(), C.c_void_p(0x1000)
    need = h.ggms_sample_khop_typed_temporal_workspace_bytes(10, 3)
    assert need - h.ggms_sample_khop_typed_workspace_bytes(10, 3) == (1 + 3) * 10 * 4  # the cut, and R more words per seed
    g = _lib.Graph(0x1000, 0x1000, None, None, a["num_part"], 0, 100, 0)
    tf = (C.c_uint32 * 3)(*a["tf"])
    rc = h.ggms_sample_khop_typed_temporal(C.byref(g), a["edge_type"], a["edge_time"], a["R"], tf, fake, fake, 10, a["pick"],
                                           7, fake, fake, fake, fake, fake, fake, need if a["ws"] is None else a["ws"], None)
    assert rc == -1 and case[1] in h.ggms_last_error().decode(), h.ggms_last_error().decode()  # GGMS_ERR_INVALID
    # the batch call names itself where ggms_sample_batch is asked for type 13; 42 stays unknown
    f = (C.c_size_t * 1)(4)
    for t, word in ((13, "ggms_sample_batch_typed_temporal"), (42, "invalid argument")):
        assert h.ggms_sample_batch(t, C.byref(g), fake, 10, f, 1, C.cast(fake, C.POINTER(_lib.HashTable)),
                                   None, 0, C.cast(fake, C.POINTER(C.c_void_p)), C.cast(fake, C.POINTER(C.c_void_p)), fake,
                                   None, fake, 1 << 20, None) == -1
        assert word in h.ggms_last_error().decode()
