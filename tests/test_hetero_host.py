"""The heterogeneous batch view on the host: the numpy statement (tests/hetero_ref.py) against double loops, the nesting
property that lets one `local` array serve every layer, the dataset helpers, and the argument errors of both leaves, which
all come before the first device call (no GPU touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import hetero_ref as ref
from graphgen import powerlaw_csr
from xgnn_amd import _lib, datagen
from xgnn_amd._lib import lib

INVALID = -1  # GGMS_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    else:
        for x, y in zip(a, b):
            if x is None or y is None:
                assert x is None and y is None
            elif isinstance(x, list):
                assert len(x) == len(y)
                for u, v in zip(x, y):
                    np.testing.assert_array_equal(u, v)
            else:
                np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("T", [1, 2, 5, 32])
def test_nodes_statement_against_double_loops(T):
    rng = np.random.RandomState(T)
    node_type = rng.randint(0, T + (1 if T < 32 else 0), 300).astype(np.uint8)  # a value == T: no valid type
    nodes = rng.randint(0, 300, 400).astype(np.uint32)
    nodes[[3, 77, 399]] = [ref.EMPTY, 300, 1 << 31]
    cuts = [0, 1, 77, 400, 1000]
    got = ref.hetero_nodes(node_type, T, nodes, cuts)
    same(got, ref.hetero_nodes_loops(node_type, T, nodes, cuts))
    valid = got["ntype"] != ref.NO_TYPE
    assert not valid[[3, 77, 399]].any() and got["base"][T] == valid.sum()
    assert sorted(got["slot"][valid]) == list(range(int(valid.sum())))  # a permutation of the valid entries
    np.testing.assert_array_equal(got["typed_nodes"][got["slot"][valid]], nodes[valid])
    np.testing.assert_array_equal(got["cut_counts"][-1], np.diff(got["base"]))


@pytest.mark.parametrize("R", [1, 2, 5, 32])
def test_edges_statement_against_double_loops(R):
    rng = np.random.RandomState(R)
    local = rng.randint(0, 50, 60).astype(np.uint32)
    sizes = [0, 1, 130]
    rows = [rng.randint(0, 64, n).astype(np.uint32) for n in sizes]  # 60 .. 63: beyond `local`
    cols = [rng.randint(0, 64, n).astype(np.uint32) for n in sizes]
    eids = [rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in sizes]
    ets = [rng.randint(0, R + 2, n).astype(np.uint8) for n in sizes]  # R, R + 1: left out
    for e in (eids, None):
        got = ref.hetero_edges(rows, cols, e, ets, R, local)
        same(got, ref.hetero_edges_loops(rows, cols, e, ets, R, local))
    for i, n in enumerate(sizes):
        assert got[3][i, R] == (ets[i] < R).sum() == got[0][i].size


def test_a_layers_per_type_counts_are_the_counts_of_its_prefix():
    """The source sets of a batch's layers are nested prefixes of n2o: slicing `local` / `ntype` at a cut gives exactly
    the statement of the prefix alone, and the cut counts are that prefix's group sizes."""
    rng = np.random.RandomState(9)
    T = 3
    node_type = rng.randint(0, T, 500).astype(np.uint8)
    nodes = rng.permutation(500).astype(np.uint32)[:420]
    cuts = [8, 90, 420]
    whole = ref.hetero_nodes(node_type, T, nodes, cuts)
    for k, c in enumerate(cuts):
        part = ref.hetero_nodes(node_type, T, nodes[:c])
        np.testing.assert_array_equal(whole["local"][:c], part["local"])
        np.testing.assert_array_equal(whole["ntype"][:c], part["ntype"])
        np.testing.assert_array_equal(whole["cut_counts"][k], np.diff(part["base"]))
        for t in range(T):  # a type's nodes of the prefix are the head of its group
            a = int(whole["base"][t])
            np.testing.assert_array_equal(whole["typed_nodes"][a:a + int(whole["cut_counts"][k][t])],
                                          part["typed_nodes"][part["base"][t]:part["base"][t + 1]])


def test_relation_types_and_the_sorted_csr():
    ip, ix = powerlaw_csr(400, mean_deg=6, seed=2)
    T = 3
    nt = np.random.RandomState(1).randint(0, T, 400).astype(np.uint8)
    et = datagen.relation_types(ip, ix, nt, T)
    owner = np.repeat(np.arange(400), np.diff(ip.astype(np.int64)))
    assert et.dtype == np.uint8 and et.shape == ix.shape and et.max() < T * T
    np.testing.assert_array_equal(et // T, nt[owner])  # the destination is the list's owner
    np.testing.assert_array_equal(et % T, nt[ix])      # the source is the neighbour
    ix2, et2, perm = datagen.sort_lists_by_type(ip, ix, et)
    assert datagen.first_unsorted_list(ip, et2) is None
    np.testing.assert_array_equal(et2, datagen.relation_types(ip, ix2, nt, T))  # consistent after the re-sort too
    with pytest.raises(AssertionError, match="36 relations"):
        datagen.relation_types(ip, ix, np.zeros(400, np.uint8), 6)
    with pytest.raises(AssertionError, match="one type per node"):
        datagen.relation_types(ip, ix, nt[:-1], T)
    with pytest.raises(AssertionError, match="not below num_node_type"):
        datagen.relation_types(ip, ix, nt + 1, T)


def test_write_dataset_writes_node_types_and_refuses_bad_ones(tmp_path):
    g = datagen.make_graph("tiny", seed=3)
    n = g["meta"]["num_node"]
    nt = (np.arange(n) % 3).astype(np.uint8)
    d = datagen.write_dataset(str(tmp_path / "ok"), g, minimal=True, node_type=nt, num_node_type=3)
    np.testing.assert_array_equal(np.fromfile(os.path.join(d, "node_type.bin"), np.uint8), nt)
    meta = dict(line.split("\t") for line in open(os.path.join(d, "meta.txt")).read().splitlines())
    assert meta["NUM_NODE_TYPE"] == "3"
    d = datagen.write_dataset(str(tmp_path / "plain"), g, minimal=True)
    assert not os.path.exists(os.path.join(d, "node_type.bin")) and "NUM_NODE_TYPE" not in open(os.path.join(d, "meta.txt")).read()
    for kw, word in ((dict(node_type=nt, num_node_type=2), "node 2 has type 2"),
                     (dict(node_type=nt[:-1], num_node_type=3), "one type per node"),
                     (dict(node_type=nt, num_node_type=0), "1 .. 32"), (dict(node_type=nt, num_node_type=33), "1 .. 32"),
                     (dict(node_type=nt), "1 .. 32"), (dict(num_node_type=3), "without node_type")):
        with pytest.raises(AssertionError, match=word):
            datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, **kw)


def test_python_names_header_abi_and_counts_words():
    from xgnn_amd import ops
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    for name in ("int ggms_hetero_nodes(", "size_t ggms_hetero_nodes_workspace_bytes(", "int ggms_hetero_edges(",
                 "size_t ggms_hetero_edges_workspace_bytes("):
        assert name in text
    assert callable(ops.hetero_nodes) and callable(ops.hetero_edges)
    assert lib().ggms_abi_version() == 3  # unchanged
    assert "#define GGMS_COUNTS_WORDS(L) (3 * (L) + 8)" in text and _lib.COUNTS_WORDS(3) == 17  # the new counts live elsewhere


def test_workspace_bytes():
    wn, we = lib().ggms_hetero_nodes_workspace_bytes, lib().ggms_hetero_edges_workspace_bytes
    assert 0 < wn(100000, 3) <= 4096  # a histogram per 2048 nodes: no per-node state
    assert wn(100000, 3) < wn(100000, 32) < wn(1 << 24, 32)
    assert wn(0, 1) > 0  # an empty list still has its totals
    assert wn(100, 0) == 0 and wn(100, 33) == 0 and wn((1 << 32) - 1024, 3) == 0 and wn(1 << 40, 3) == 0
    one, three = (C.c_size_t * 1)(5200), (C.c_size_t * 3)(5200, 0, 100000)
    assert 0 < we(one, 1, 4) < we(three, 3, 4) <= 8192
    assert we(one, 0, 4) == 0 and we(one, 17, 4) == 0 and we(None, 1, 4) == 0 and we(one, 1, 0) == 0 and we(one, 1, 33) == 0
    assert we((C.c_size_t * 1)(1 << 33), 1, 4) == 0


def test_argument_errors_of_the_nodes_leaf():
    l = lib()
    p = lambda k: C.c_void_p(k << 20)  # noqa: E731  (never dereferenced)
    words = (C.c_uint32 * 3)(1, 4, 7)
    need = l.ggms_hetero_nodes_workspace_bytes(1000, 3)
    assert need > 0
    base = dict(node_type=p(1), num_node=5000, T=3, nodes=p(2), max_nodes=1000, n_dev=p(3), cut_base=p(4), cut_words=words,
                B=3, ntype=p(5), local=p(6), slot=p(7), typed_nodes=p(8), base_dev=p(9), cut_counts=p(10), ws=p(11),
                wsb=need, stream=None)
    call = lambda **kw: l.ggms_hetero_nodes(*[kw.get(k, v) for k, v in base.items()])  # noqa: E731
    for bad in (0, 33, 255):
        assert call(T=bad) == INVALID and b"num_type" in l.ggms_last_error()
    assert call(B=18) == INVALID and b"num_cut" in l.ggms_last_error()
    for name, word in (("node_type", b"node_type"), ("nodes", b"nodes"), ("ntype", b"ntype"), ("local", b"local"),
                       ("slot", b"slot"), ("typed_nodes", b"typed_nodes"), ("base_dev", b"base_dev"),
                       ("cut_base", b"cut_base_dev"), ("cut_words", b"cut_words_host"), ("cut_counts", b"cut_counts_dev")):
        assert call(**{name: None}) == INVALID, name
        assert b"invalid argument" in l.ggms_last_error() and word + b" is null" in l.ggms_last_error(), l.ggms_last_error()
    assert call(max_nodes=(1 << 32) - 1024) == INVALID and b"max_nodes" in l.ggms_last_error()
    assert call(ws=None) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(wsb=need - 1) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(wsb=l.ggms_hetero_nodes_workspace_bytes(1000, 2), T=32) == INVALID and b"workspace" in l.ggms_last_error()


def test_argument_errors_of_the_edges_leaf():
    l = lib()
    p = lambda k: C.c_void_p(k << 20)  # noqa: E731
    two = lambda a, b: (C.c_void_p * 2)(a << 20 if a else None, b << 20 if b else None)  # noqa: E731
    me = (C.c_size_t * 2)(100, 50)
    need = l.ggms_hetero_edges_workspace_bytes(me, 2, 4)
    assert need > 0
    base = dict(row=two(1, 2), col=two(3, 4), eid=two(5, 6), etype=two(7, 8), me=me, L=2, R=4, counts=p(9), local=p(10),
                num_local=1000, out_row=two(11, 12), out_col=two(13, 14), out_eid=two(15, 16), off=p(17), ws=p(18), wsb=need,
                stream=None)
    call = lambda **kw: l.ggms_hetero_edges(*[kw.get(k, v) for k, v in base.items()])  # noqa: E731
    for bad in (0, 17):
        assert call(L=bad) == INVALID and b"num_layer" in l.ggms_last_error()
    for bad in (0, 33):
        assert call(R=bad) == INVALID and b"num_rel" in l.ggms_last_error()
    for name, word in (("row", b"row"), ("col", b"col"), ("etype", b"etype"), ("me", b"max_edges"), ("counts", b"counts_dev"),
                       ("local", b"local"), ("out_row", b"out_row"), ("out_col", b"out_col"), ("off", b"rel_offsets_dev")):
        assert call(**{name: None}) == INVALID, name
        assert b"invalid argument" in l.ggms_last_error() and word + b" is null" in l.ggms_last_error(), l.ggms_last_error()
    assert call(eid=None) == INVALID and b"out_eid" in l.ggms_last_error()
    assert call(out_eid=None) == INVALID and b"out_eid" in l.ggms_last_error()
    assert call(row=two(None, 2)) == INVALID and b"row[0]" in l.ggms_last_error()
    assert call(out_eid=two(15, None)) == INVALID and b"eid[1]" in l.ggms_last_error()
    assert call(etype=two(7, None)) == INVALID and b"etype[1]" in l.ggms_last_error()
    assert call(me=(C.c_size_t * 2)(100, 1 << 33)) == INVALID and b"max_edges" in l.ggms_last_error()
    assert call(ws=None) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(wsb=need - 1) == INVALID and b"workspace" in l.ggms_last_error()
