"""ggms_edge_positions on the host: the numpy statement's own properties (tests/edge_positions_ref.py), the Python names,
the workspace size and the argument errors, which all come before the first device call (no GPU touched)."""
import ctypes as C
import os

import numpy as np

import edge_positions_ref as ref
from graphgen import powerlaw_csr
from xgnn_amd._lib import Graph, lib

INVALID = -1  # GGMS_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731


def test_positions_name_the_edge_and_lie_in_the_seeds_row():
    ip, ix = powerlaw_csr(2000, mean_deg=12, seed=3)
    rng = np.random.RandomState(1)
    pos = rng.randint(0, ix.size, 3000)
    col = (np.searchsorted(ip, pos, side="right") - 1).astype(np.uint32)  # the node whose list holds position p
    row = ix[pos]
    eid, = ref.edge_positions(ip, ix, [row], [col])
    assert (eid != ref.EMPTY).all()
    assert (ix[eid] == row).all()
    assert (ip[col] <= eid).all() and (eid < ip[col + 1]).all()
    assert (eid <= pos).all()  # the FIRST copy: at or before the position the target was taken from
    for e, p, c in zip(eid[:200], pos[:200], col[:200]):
        assert not (ix[ip[c]:e] == ix[p]).any()


def test_first_copy_absent_pairs_and_ids_that_are_no_node():
    ip = u32(0, 6, 6, 8)
    ix = u32(2, 1, 2, 1, 0, 2, 0, 0)
    row = u32(2, 1, 0, 2, 0, 1, 0, ref.EMPTY, 3, 0, 0)
    col = u32(0, 0, 0, 0, 2, 2, 1, 0, 0, ref.EMPTY, 3)
    eid, = ref.edge_positions(ip, ix, [row], [col])
    E = ref.EMPTY
    #                        first copies      list 2     absent, empty list, no nodes
    assert eid.tolist() == [0, 1, 4, 0, 6, E, E, E, E, E, E]


def test_the_id_map_comes_first_and_ids_beyond_it_are_empty():
    ip = u32(0, 2, 3, 3)
    ix = u32(1, 2, 0)
    n2o = u32(2, 0, 1)  # local 0 = node 2, local 1 = node 0, local 2 = node 1
    row = u32(2, 0, 1, 3, 1)
    col = u32(1, 1, 2, 1, 7)
    eid, = ref.edge_positions(ip, ix, [row], [col], id_map=n2o)
    assert eid.tolist() == [0, 1, 2, ref.EMPTY, ref.EMPTY]
    plain, = ref.edge_positions(ip, ix, [n2o[row[:3]]], [n2o[col[:3]]])
    assert plain.tolist() == [0, 1, 2]


def test_python_names_and_header():
    import samgraph.torch as sam
    from xgnn_amd import ops
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    assert "int ggms_edge_positions(" in text and "size_t ggms_edge_positions_workspace_bytes(" in text
    assert callable(ops.edge_positions)
    for name in ("get_graph_edge_ids", "get_graph_edge_feat", "get_graph_link_edge_ids"):
        assert callable(getattr(sam, name))
    assert lib().ggms_abi_version() == 3  # unchanged


def test_workspace_bytes():
    ws = lib().ggms_edge_positions_workspace_bytes
    one = (C.c_size_t * 1)(5200)
    three = (C.c_size_t * 3)(5200, 0, 100000)
    assert 0 < ws(one, 1) <= 1024  # one word per 64 edges and a counter: no per-edge state
    assert ws(one, 1) < ws(three, 3) <= 16 * 1024
    assert ws(one, 0) == 0 and ws(one, 17) == 0 and ws(None, 1) == 0
    assert ws((C.c_size_t * 1)(1 << 33), 1) == 0


def test_argument_errors():
    l = lib()
    g = Graph()
    g.indptr, g.indices, g.num_node = 1 << 20, 1 << 21, 100  # never dereferenced
    sharded = Graph.from_buffer_copy(g)
    sharded.num_part = 2
    no_indices = Graph.from_buffer_copy(g)
    no_indices.indices = None
    p = C.c_void_p(1 << 22)
    three = lambda a, b: (C.c_void_p * 2)(a, b)  # noqa: E731
    rows, cols, eids = three(1 << 23, 1 << 24), three(1 << 25, 1 << 26), three(1 << 27, 1 << 28)
    me = (C.c_size_t * 2)(100, 50)
    need = l.ggms_edge_positions_workspace_bytes(me, 2)
    assert need > 0
    base = dict(graph=C.byref(g), ne=1000, id_map=None, nmap=0, row=rows, col=cols, eid=eids, me=me, L=2, counts=p, ws=p,
                wsb=need, stream=None)
    call = lambda **kw: l.ggms_edge_positions(*[kw.get(k, v) for k, v in base.items()])  # noqa: E731
    assert call(graph=C.byref(sharded)) == INVALID and b"sharded" in l.ggms_last_error()
    for bad in (0xFFFFFFFF, 1 << 32, 1 << 40):
        assert call(ne=bad) == INVALID and b"32-bit" in l.ggms_last_error()
    for bad in (0, 17):
        assert call(L=bad) == INVALID and b"num_layer" in l.ggms_last_error()
    for name in ("row", "col", "eid", "me", "counts"):
        assert call(**{name: None}) == INVALID and b"invalid argument" in l.ggms_last_error(), name
    assert call(graph=None) == INVALID and call(graph=C.byref(no_indices)) == INVALID
    assert call(eid=three(1 << 27, None)) == INVALID and b"eid[1]" in l.ggms_last_error()
    assert call(row=three(None, 1 << 24)) == INVALID and b"row[0]" in l.ggms_last_error()
    assert call(ws=None) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(wsb=need - 1) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(me=(C.c_size_t * 2)(100, 1 << 33)) == INVALID
    # layers whose bounds are all 0: nothing to do, without a GPU
    assert call(me=(C.c_size_t * 2)(0, 0), row=three(None, None), col=three(None, None), eid=three(None, None)) == 0
