"""ggms_induced_edges on the host: the numpy statement (tests/induced_ref.py) against a brute-force double loop, its rules
for repeats, ids that are no node and truncation, and the leaf's argument refusals, which all come before the first
device call (no GPU touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import induced_ref as ref
from xgnn_amd import _lib
from xgnn_amd._lib import Graph, lib

INVALID = -1  # GGMS_ERR_INVALID
EMPTY = ref.EMPTY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731


def brute(ip, ix, nodes):
    """The definition, word for word."""
    num_node = len(ip) - 1
    nodes = [int(v) for v in nodes]

    def loc(v):
        if v >= num_node:
            return None
        for j, u in enumerate(nodes):
            if u == v:
                return j
        return None
    out, walked = [], 0
    for j, u in enumerate(nodes):
        if loc(u) != j:
            continue
        for p in range(int(ip[u]), int(ip[u + 1])):
            walked += 1
            l = loc(int(ix[p]))
            if l is not None:
                out.append((l, j, p))
    a = np.array(out, np.uint32).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2], walked


def multigraph(num_node, num_edge, rng):
    """Random lists with parallel edges and self-loops; some nodes have no list."""
    src = np.sort(rng.randint(0, num_node, num_edge))
    src[src % 7 == 3] = 0
    src.sort()
    ip = np.zeros(num_node + 1, np.uint32)
    ip[1:] = np.cumsum(np.bincount(src, minlength=num_node))
    ix = rng.randint(0, num_node, num_edge).astype(np.uint32)
    ix[::5] = src[::5]  # self-loops
    ix[1::9] = ix[0:-1:9]  # parallel edges (where both lie in one list)
    return ip, ix


@pytest.mark.parametrize("seed", range(6))
def test_ref_equals_the_double_loop_on_random_multigraphs(seed):
    rng = np.random.RandomState(seed)
    ip, ix = multigraph(60, 700, rng)
    nodes = rng.randint(0, 60, 5 + 9 * seed).astype(np.uint32)  # repeats included
    nodes[rng.randint(0, nodes.size, 2)] = (EMPTY, 60 + seed)
    row, col, eid, M, walked = ref.induced_edges(ip, ix, nodes)
    b = brute(ip, ix, nodes)
    assert M == b[0].size and walked == b[3]
    for got, want in zip((row, col, eid), b):
        np.testing.assert_array_equal(got, want)
    assert (ix[eid] == nodes[row]).all() and (ip[nodes[col]] <= eid).all() and (eid < ip[nodes[col].astype(np.int64) + 1]).all()
    if M:
        self_loops = int((row == col).sum())
        pairs = np.stack([row, col], 1)
        print(f"seed {seed}: {M} edges, {self_loops} self-loops, {M - np.unique(pairs, axis=0).shape[0]} parallel copies")
        assert np.unique(eid).size == M  # every edge once, parallel copies under their own position


def test_first_position_owns_and_is_the_target():
    ip = u32(0, 3, 5, 6)
    ix = u32(1, 2, 1, 0, 0, 2)  # 0: [1, 2, 1]  1: [0, 0]  2: [2]
    row, col, eid, M, walked = ref.induced_edges(ip, ix, u32(1, 0, 1, 0, 1))
    # owners: position 0 (node 1) and 1 (node 0); the later copies emit nothing, and targets map to the first position
    np.testing.assert_array_equal(col, u32(0, 0, 1, 1))
    np.testing.assert_array_equal(row, u32(1, 1, 0, 0))
    np.testing.assert_array_equal(eid, u32(3, 4, 0, 2))
    assert (M, walked) == (4, 5)


def test_ids_that_are_no_node_own_nothing_and_are_nobodys_target():
    ip = u32(0, 2, 3, 4)
    ix = u32(1, 2, 0, 2)
    row, col, eid, M, walked = ref.induced_edges(ip, ix, u32(EMPTY, 7, 2, 3, 0))
    np.testing.assert_array_equal(col, u32(2, 4))  # node 2's self-loop, then 0 -> 2
    np.testing.assert_array_equal(row, u32(2, 2))
    np.testing.assert_array_equal(eid, u32(3, 1))
    assert (M, walked) == (2, 3)
    assert ref.induced_edges(ip, ix, u32())[3:] == (0, 0)
    assert ref.induced_edges(ip, ix, u32(EMPTY, 3))[3:] == (0, 0)


def test_truncation_keeps_the_canonical_prefix():
    rng = np.random.RandomState(9)
    ip, ix = multigraph(40, 500, rng)
    nodes = rng.permutation(40)[:25].astype(np.uint32)
    full = ref.induced_edges(ip, ix, nodes)
    M = full[3]
    assert M > 10
    for cap in (M + 3, M, M - 1, 1, 0):
        got = ref.induced_edges(ip, ix, nodes, max_edges=cap)
        assert got[3] == M and got[4] == full[4]  # the count says what exists, not what was kept
        for a, b in zip(got[:3], full[:3]):
            np.testing.assert_array_equal(a, b[:min(M, cap)])


def test_header_names_and_abi():
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    for name in ("ggms_induced_edges", "ggms_induced_map_init", "ggms_induced_edges_workspace_bytes"):
        assert name + "(" in text and hasattr(lib(), name)
    assert lib().ggms_abi_version() == 3  # unchanged
    assert _lib.COUNTS_WORDS(3) == 17 and "#define GGMS_COUNTS_WORDS(L) (3 * (L) + 8)" in text  # no new counts word


def test_workspace_bytes():
    ws = lib().ggms_induced_edges_workspace_bytes
    # the prefix array and a word per 1024 nodes; two words per possible edge tile of 2048 and a word per 1024 tiles
    assert 4 * 100_000 <= ws(100_000, 0) <= 4 * 100_000 + 4096
    per_tile = (ws(1000, 1 << 31) - ws(1000, 0)) / ((1 << 31) / 2048)
    assert 8 <= per_tile <= 8.1
    assert ws(1000, 1 << 40) == ws(1000, (1 << 32) - 1)  # min(num_edge, 2^32 - 1)


def test_argument_errors():
    l = lib()
    g = Graph()
    g.indptr, g.indices, g.num_node = 1 << 20, 1 << 21, 100  # never dereferenced
    sharded = Graph.from_buffer_copy(g)
    sharded.num_part = 2
    no_indices = Graph.from_buffer_copy(g)
    no_indices.indices = None
    need = l.ggms_induced_edges_workspace_bytes(500, 9000)
    base = dict(graph=C.byref(g), ne=9000, nodes=1 << 22, mn=500, ndev=None, lo=1 << 23, row=1 << 24, col=1 << 25,
                eid=1 << 26, me=4000, counts=1 << 27, ws=1 << 28, wsb=need)

    def call(**kw):
        a = dict(base, **kw)
        return l.ggms_induced_edges(a["graph"], a["ne"], a["nodes"], a["mn"], a["ndev"], a["lo"], a["row"], a["col"],
                                    a["eid"], a["me"], a["counts"], a["ws"], a["wsb"], None)
    for name in ("nodes", "lo", "row", "col"):
        assert call(**{name: None}) == INVALID and b"null" in l.ggms_last_error(), name
    assert call(graph=None) == INVALID and b"null" in l.ggms_last_error()
    assert call(counts=None) == INVALID and b"null" in l.ggms_last_error()
    assert call(graph=C.byref(no_indices)) == INVALID and b"null" in l.ggms_last_error()
    assert call(ws=None) == INVALID and b"workspace" in l.ggms_last_error()
    assert call(wsb=need - 1) == INVALID and b"workspace" in l.ggms_last_error()
    for bad in (0xFFFFFFFF, 1 << 32, 1 << 40):
        assert call(ne=bad) == INVALID and b"32-bit" in l.ggms_last_error()
    for bad in ((1 << 32) - 1024, 1 << 32, 1 << 40):
        assert call(mn=bad, wsb=1 << 60) == INVALID and b"max_nodes" in l.ggms_last_error()
    assert call(graph=C.byref(sharded)) == INVALID and b"sharded" in l.ggms_last_error()
    assert l.ggms_induced_map_init(None, 10, None) == INVALID and b"null" in l.ggms_last_error()
