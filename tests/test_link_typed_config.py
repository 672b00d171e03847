"""Typed negatives on the host: the numpy statement against a brute-force loop (and its negatives' types), the argument
errors of ggms_link_seeds_typed through pointers that are never dereferenced, the engine's refusals by name, and
ops.type_lists against numpy."""
import ctypes as C

import numpy as np
import pytest

import link_ref as ref
import link_typed_ref as tref
from test_hetero_config import ON, datasets  # noqa: F401  (fixture)
from config_run import run_config
from xgnn_amd import lib
from xgnn_amd._lib import Graph

INVALID = -1  # GGMS_ERR_INVALID
LINK = dict(ON, task="link_prediction", num_negative=2)


@pytest.fixture(scope="module")
def graph():
    return tref.edge_case_graph()


@pytest.mark.parametrize("mode", [tref.TYPED_UNIFORM, tref.TYPED_EXCLUDE])
def test_the_twin_equals_a_plain_loop(graph, mode):
    ip, ix, et, nt, T, cases = graph
    K, salt = 5, 0xBEEF
    eids = np.array(sorted(cases.values()) + [int(ip[-1])], np.uint32)
    out, rel, forced = tref.link_seeds_typed(ip, ix, et, nt, T, eids, K, mode, salt)
    src, dst, neg = ref.split(out, K)
    assert (nt[neg[:-1]] == nt[dst[:-1]][:, None]).all()  # every negative is of its positive destination's type
    assert src[-1] == dst[-1] == ref.EMPTY and (neg[-1] == ref.EMPTY).all()
    want_forced = 0
    for i, e in enumerate(eids[:-1].tolist()):
        u = max(w for w in range(ip.size - 1) if ip[w] <= e)
        pool = [w for w in range(nt.size) if nt[w] == nt[ix[e]]]
        seg = [int(ix[p]) for p in range(ip[u], ip[u + 1]) if et[p] == et[e]] + [u]
        for j in range(K):
            tries = [pool[int(ref.cand(e, j, a, salt, len(pool)))] for a in range(8 if mode == tref.TYPED_EXCLUDE else 1)]
            ok = [w for w in tries if w not in seg] if mode == tref.TYPED_EXCLUDE else tries
            want_forced += not ok
            assert neg[i, j] == (ok[0] if ok else tries[-1]), (e, j)
        assert (src[i], dst[i], rel[i]) == (u, ix[e], et[e])
    assert forced == want_forced and rel[-1] == 0xFF


def test_argument_errors():
    l = lib()
    p = C.c_void_p(1 << 20)  # never dereferenced: the checks come first
    g, sharded = Graph(), Graph()
    g.indptr, g.indices, g.num_node = 1 << 22, 1 << 23, 1000
    sharded.indptr, sharded.indices, sharded.num_node, sharded.num_part = 1 << 22, 1 << 23, 1000, 2
    good = dict(graph=C.byref(g), et=p, nt=p, nodes=p, base=p, T=3, eids=p, B=10, K=5, mode=3, out=p)
    call = lambda **kw: (lambda a: l.ggms_link_seeds_typed(a["graph"], a["et"], a["nt"], a["nodes"], a["base"], a["T"],  # noqa: E731
                                                           a["eids"], a["B"], a["K"], a["mode"], 0, a["out"], None, None,
                                                           None))(dict(good, **kw))
    for kw, word in [(dict(K=0), b"num_negative"), (dict(K=65), b"num_negative"), (dict(T=0), b"num_node_type"),
                     (dict(T=33), b"num_node_type"), (dict(graph=C.byref(sharded)), b"num_part"), (dict(mode=0), b"mode"),
                     (dict(mode=1), b"mode"), (dict(mode=4), b"mode"), (dict(et=None), b"edge_type"),
                     (dict(nt=None), b"node_type"), (dict(nodes=None), b"type_nodes"), (dict(base=None), b"type_base"),
                     (dict(eids=None), b"edge_ids"), (dict(out=None), b"endpoints"), (dict(graph=None), b"graph")]:
        assert call(**kw) == INVALID and word in l.ggms_last_error(), (kw, l.ggms_last_error())
    assert call(B=0, eids=None, out=None) == 0 and call(B=0, K=65) == INVALID
    for mode in (2, 3):  # the untyped leaf keeps refusing the typed modes
        assert l.ggms_link_seeds(C.byref(g), p, 10, 5, mode, 0, p, None, None) == INVALID


@pytest.mark.parametrize("mode", ["typed_uniform", "typed_exclude"])
def test_the_engine_takes_the_modes_and_refuses_by_name(datasets, mode):
    out = run_config(datasets["ok"], dict(LINK, negative_mode=mode))
    assert out.returncode == 0 and out.stdout.split() == ["configured", "13", "20"], out.stderr[-2000:]
    no_hetero = {k: v for k, v in LINK.items() if k != "hetero_batch"}
    for extra, words in [(no_hetero, ["hetero_batch = on"]),
                         (dict(task="link_prediction", num_negative=2, _sample_type=8), ["khop_typed"]),
                         (dict(ON), ["task = link_prediction"])]:
        out = run_config(datasets["ok"], dict(extra, negative_mode=mode))
        assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]
        assert all(w in out.stderr for w in [f"negative_mode = {mode}"] + words), out.stderr[-2000:]
    out = run_config(datasets["ok"], LINK, tail="sam.get_graph_link_rel(0)")
    assert out.returncode < 0 and "samgraph_get_graph_link_rel needs negative_mode = typed_uniform" in out.stderr


def test_type_lists_equal_numpy():
    import torch
    from xgnn_amd import ops
    nt = np.random.RandomState(3).choice(5, 777, p=[0.4, 0.3, 0.0, 0.2, 0.1]).astype(np.uint8)  # type 2 has no node
    nodes, base = ops.type_lists(torch.from_numpy(nt), 6)
    want_nodes, want_base = tref.type_lists(nt, 6)
    assert nodes.dtype == base.dtype == torch.int32
    np.testing.assert_array_equal(nodes.numpy(), want_nodes)
    np.testing.assert_array_equal(base.numpy(), want_base)
