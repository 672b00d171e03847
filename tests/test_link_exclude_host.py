"""exclude_seed_edges on the host: the numpy statement (tests/link_exclude_ref.py) on hand-written cases, the header's
constants against the Python names, the argument errors of ggms_drop_pair_edges (no GPU touched) and which values of
the config key the engine takes."""
import ctypes as C
import os

import numpy as np
import pytest

import link_exclude_ref as ref
from config_run import run_config
from test_engine import make_dataset
from xgnn_amd._lib import lib

INVALID = -1  # GGMS_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731


def test_forward_and_reverse_on_one_layer():
    #            e: 0  1  2  3  4  5  6
    col = u32(1, 1, 2, 2, 1, 3, 2)
    row = u32(2, 5, 1, 1, 2, 3, 9)
    src, dst = u32(1), u32(2)  # the positive 1 -> 2: col = 1, row = 2
    (r, c), = ref.drop_pair_edges(src, dst, ref.FORWARD, [(row, col)])[0]
    assert r.tolist() == [5, 1, 1, 3, 9] and c.tolist() == [1, 2, 2, 3, 2]  # edges 0 and 4 (a multi-edge) are gone
    (r, c), = ref.drop_pair_edges(src, dst, ref.REVERSE, [(row, col)])[0]
    assert r.tolist() == [2, 5, 2, 3, 9] and c.tolist() == [1, 1, 1, 3, 2]  # edges 2 and 3: the mirror, twice
    out, dropped = ref.drop_pair_edges(src, dst, ref.FORWARD | ref.REVERSE, [(row, col)])
    assert out[0][0].tolist() == [5, 3, 9] and out[0][1].tolist() == [1, 3, 2] and dropped == [4]
    out, dropped = ref.drop_pair_edges(src, dst, 0, [(row, col)])
    assert out[0][0].tolist() == row.tolist() and dropped == [0]


def test_self_loop_repeated_and_empty_pairs():
    col = u32(3, 3, 4, 7, ref.EMPTY, 7)
    row = u32(3, 4, 3, ref.EMPTY, 7, 7)
    for which in (ref.FORWARD, ref.REVERSE):  # (u, u) matches its self-loop under either bit
        out, dropped = ref.drop_pair_edges(u32(3), u32(3), which, [(row, col)])
        assert out[0][0].tolist() == row[1:].tolist() and dropped == [1]
    # a repeated pair is one pair
    assert ref.pair_set(u32(3, 3, 3), u32(4, 4, 4), ref.FORWARD) == {(3, 4)}
    assert ref.drop_pair_edges(u32(3, 3), u32(4, 4), ref.FORWARD, [(row, col)])[1] == [1]
    # a pair holding EMPTY matches nothing, not even an edge that holds EMPTY in the same place
    assert ref.pair_set(u32(7, ref.EMPTY, ref.EMPTY), u32(ref.EMPTY, 7, ref.EMPTY), 3) == set()
    assert ref.drop_pair_edges(u32(7, ref.EMPTY), u32(ref.EMPTY, 7), 3, [(row, col)])[1] == [0]


def test_self_against_both_on_several_layers():
    src, dst = u32(0, 1), u32(1, 2)
    layers = [(u32(1, 0, 2, 1), u32(0, 1, 1, 2)), (u32(), u32()), (u32(0), u32(1))]
    out, dropped = ref.drop_pair_edges(src, dst, ref.WHICH_OF["self"], layers)
    assert [r.tolist() for r, _ in out] == [[0, 1], [], [0]] and dropped == [2, 0, 0]
    out, dropped = ref.drop_pair_edges(src, dst, ref.WHICH_OF["both"], layers)
    assert [r.tolist() for r, _ in out] == [[], [], []] and dropped == [4, 0, 1]
    assert ref.WHICH_OF == dict(none=0, self=1, both=3)


def test_header_constants_and_python_names():
    import samgraph.torch as sam
    from xgnn_amd import ops
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    assert "#define GGMS_DROP_FORWARD 1u" in text and "#define GGMS_DROP_REVERSE 2u" in text
    assert (ops.DROP_FORWARD, ops.DROP_REVERSE) == (ref.FORWARD, ref.REVERSE) == (1, 2)
    assert callable(ops.drop_pair_edges) and callable(ops.BatchSampler.drop_pair_edges)
    assert callable(sam.get_graph_num_excluded)
    assert lib().ggms_abi_version() == 3


def test_workspace_bytes():
    l = lib()
    ws = l.ggms_drop_pair_edges_workspace_bytes
    one = (C.c_size_t * 1)(5200)
    three = (C.c_size_t * 3)(5200, 0, 100000)
    small = ws(1, one, 1)
    assert small >= 8 * 5200  # the snapshot of row and col
    assert ws(8000, one, 1) > small  # the pair table grows with the pairs
    assert ws(1, three, 3) >= 8 * (5200 + 100000)
    assert ws(1, one, 0) == 0 and ws(1, one, 17) == 0 and ws(1, None, 1) == 0
    assert ws(1, (C.c_size_t * 1)(1 << 32), 1) == 0  # a layer bound beyond 32 bits


def test_drop_pair_edges_argument_errors():
    """Every check comes before the first launch: no GPU is needed to see them."""
    l = lib()
    call = l.ggms_drop_pair_edges
    p = C.c_void_p(1 << 20)  # never dereferenced
    rows, cols, null_row = (C.c_void_p * 2)(1 << 21, 1 << 22), (C.c_void_p * 2)(1 << 23, 1 << 24), (C.c_void_p * 2)(1 << 21, None)
    me = (C.c_size_t * 2)(100, 50)
    need = l.ggms_drop_pair_edges_workspace_bytes(10, me, 2)
    assert need > 0
    ok = lambda **kw: call(*[kw.get(k, v) for k, v in dict(  # noqa: E731
        src=p, dst=p, n=10, which=3, row=rows, col=cols, me=me, L=2, counts=p, dropped=None, ws=p, wsb=need,
        stream=None).items()])
    for bad in (4, 7, 0xFFFFFFFF):
        assert ok(which=bad) == INVALID and b"which" in l.ggms_last_error()
    for bad in (0, 17):
        assert ok(L=bad) == INVALID and b"num_layer" in l.ggms_last_error()
    assert ok(row=None) == INVALID and ok(col=None) == INVALID and ok(me=None) == INVALID and ok(counts=None) == INVALID
    assert ok(src=None) == INVALID and ok(dst=None) == INVALID
    assert ok(row=null_row) == INVALID and b"row[1]" in l.ggms_last_error()
    assert ok(ws=None) == INVALID and ok(wsb=need - 1) == INVALID and b"workspace" in l.ggms_last_error()
    assert ok(me=(C.c_size_t * 2)(100, 1 << 32)) == INVALID
    # nothing to do is fine -- without pairs, workspace or a GPU -- with the argument checks still in front of it
    assert ok(which=0, ws=None, wsb=0) == 0 and ok(n=0, src=None, dst=None, ws=None, wsb=0) == 0
    assert ok(which=4, n=0) == INVALID and ok(which=0, L=0) == INVALID and ok(n=0, counts=None) == INVALID


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("link_exclude_ds"))


LINK = dict(task="link_prediction")


@pytest.mark.parametrize("value", ["none", "self", "both"])
def test_the_key_is_taken_with_the_task(dataset, value):
    out = run_config(dataset["path"], dict(LINK, exclude_seed_edges=value))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[:3] == ["configured", "13", "20"]


@pytest.mark.parametrize("value", ["reverse", 7, "Both"])
def test_bad_values_are_refused_by_key_and_value(dataset, value):
    out = run_config(dataset["path"], dict(LINK, exclude_seed_edges=value))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "exclude_seed_edges" in out.stderr and f"exclude_seed_edges = {value}" in out.stderr, out.stderr[-2000:]


def test_without_the_task_the_key_is_not_read(dataset):
    for extra in (dict(exclude_seed_edges="reverse"), dict(task="node_classification", exclude_seed_edges="both")):
        out = run_config(dataset["path"], extra)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split()[:3] == ["configured", "13", "20"]
