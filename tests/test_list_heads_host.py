"""Inline list heads (include/ggms.h, "Inline list heads") on a host without a GPU: the byte-count rule, the argument
checks that come before any device call, and the handle registry -- attach, detach, re-attach, and the rule that a
handle is used only by a struct whose indptr, indices and num_node are the ones it was attached with."""
import ctypes as C
import os

from xgnn_amd import _lib
from xgnn_amd._lib import Graph, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GGMS_ERR_INVALID


def _err():
    return lib().ggms_last_error().decode()


def _graph(indptr=1 << 20, indices=1 << 24, num_node=600):
    g = Graph()  # the addresses are never dereferenced: the checks and the registry are host arithmetic
    g.indptr, g.indices, g.num_node = indptr, indices, num_node
    return g


def test_abi_version_is_still_3_and_the_struct_keeps_its_size():
    assert lib().ggms_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert C.sizeof(Graph) == 48 and Graph.heads_id.offset == 44 and Graph.heads_id.size == 4
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    assert "uint32_t heads_id;" in text and "#define GGMS_LIST_HEAD_BYTES 64" in text


def test_byte_count_rule():
    l = lib()
    assert l.ggms_list_heads_bytes(0) == 0 and l.ggms_list_heads_bytes(1) == 64
    assert l.ggms_list_heads_bytes(2_449_029) == 156_737_856            # products
    assert l.ggms_list_heads_bytes(111_059_956) == 7_107_837_184        # papers100M: past 2^32


def test_build_refuses_bad_arguments_before_any_device_call():
    l = lib()
    buf = C.c_void_p(1 << 30)
    g = _graph()
    assert l.ggms_list_heads_build(None, buf, 1 << 20, None) == INVALID
    assert l.ggms_list_heads_build(C.byref(g), None, 1 << 20, None) == INVALID
    assert l.ggms_list_heads_build(C.byref(g), buf, 64 * 600 - 1, None) == INVALID and "needed" in _err()  # short buffer
    assert l.ggms_list_heads_build(C.byref(g), C.c_void_p((1 << 30) + 32), 1 << 20, None) == INVALID       # misaligned
    no_csr = _graph(indptr=None)
    assert l.ggms_list_heads_build(C.byref(no_csr), buf, 1 << 20, None) == INVALID
    sharded = _graph()
    sharded.num_part = 2
    assert l.ggms_list_heads_build(C.byref(sharded), buf, 1 << 20, None) == INVALID and "unsharded" in _err()
    empty = _graph(num_node=0)
    assert l.ggms_list_heads_build(C.byref(empty), None, 0, None) == 0  # nothing to do is fine


def test_attach_refuses_bad_arguments():
    l = lib()
    g = _graph()
    assert l.ggms_list_heads_attach(None, C.c_void_p(1 << 30)) == INVALID
    assert l.ggms_list_heads_attach(C.byref(g), None) == INVALID
    assert l.ggms_list_heads_attach(C.byref(g), C.c_void_p((1 << 30) + 4)) == INVALID
    sharded = _graph()
    sharded.num_part = 3
    assert l.ggms_list_heads_attach(C.byref(sharded), C.c_void_p(1 << 30)) == INVALID and "unsharded" in _err()
    assert g.heads_id == 0 and sharded.heads_id == 0
    assert l.ggms_list_heads_detach(None) == INVALID


def test_attach_detach_reattach():
    l = lib()
    a, b = _graph(), _graph(indptr=2 << 20, indices=2 << 24, num_node=7)
    ha, hb = 1 << 30, 1 << 31
    assert l.ggms_list_heads_of(C.byref(a)) is None
    assert l.ggms_list_heads_attach(C.byref(a), C.c_void_p(ha)) == 0 and a.heads_id != 0
    assert l.ggms_list_heads_attach(C.byref(b), C.c_void_p(hb)) == 0 and b.heads_id not in (0, a.heads_id)
    assert l.ggms_list_heads_of(C.byref(a)) == ha and l.ggms_list_heads_of(C.byref(b)) == hb
    # attaching again replaces the table and does not leak the old handle
    first = a.heads_id
    assert l.ggms_list_heads_attach(C.byref(a), C.c_void_p(ha + 64)) == 0
    assert a.heads_id == first and l.ggms_list_heads_of(C.byref(a)) == ha + 64
    assert l.ggms_list_heads_detach(C.byref(a)) == 0 and a.heads_id == 0
    assert l.ggms_list_heads_of(C.byref(a)) is None and l.ggms_list_heads_of(C.byref(b)) == hb
    assert l.ggms_list_heads_detach(C.byref(a)) == 0  # nothing attached: nothing happens
    assert l.ggms_list_heads_attach(C.byref(a), C.c_void_p(ha)) == 0 and l.ggms_list_heads_of(C.byref(a)) == ha
    assert l.ggms_list_heads_detach(C.byref(a)) == 0 and l.ggms_list_heads_detach(C.byref(b)) == 0
    assert l.ggms_list_heads_of(C.byref(b)) is None


def test_a_struct_that_no_longer_matches_its_id_has_no_heads():
    l = lib()
    g = _graph()
    assert l.ggms_list_heads_attach(C.byref(g), C.c_void_p(1 << 30)) == 0
    sharded = Graph.from_buffer_copy(g)  # a sharded view never uses heads, whatever its id says
    sharded.num_part = 2
    assert l.ggms_list_heads_of(C.byref(sharded)) is None
    for field, value in (("indptr", 3 << 20), ("indices", 3 << 24), ("num_node", 601)):
        c = Graph.from_buffer_copy(g)  # same id, one value replaced
        setattr(c, field, value)
        assert l.ggms_list_heads_of(C.byref(c)) is None, field
        # and such a struct cannot release the handle of the real one
        assert l.ggms_list_heads_detach(C.byref(c)) == 0 and c.heads_id == 0
        assert l.ggms_list_heads_of(C.byref(g)) == 1 << 30, field
    stale = Graph.from_buffer_copy(g)
    assert l.ggms_list_heads_detach(C.byref(g)) == 0
    assert l.ggms_list_heads_of(C.byref(stale)) is None  # the id it carries is no longer live
    for garbage in (1, 200, 255, 256, 0xDEADBEEF, 0xFFFFFFFF):  # the word used to be padding
        junk = _graph()
        junk.heads_id = garbage
        assert l.ggms_list_heads_of(C.byref(junk)) is None


def test_registry_is_bounded():
    l = lib()
    gs = [_graph(indptr=(16 + i) << 20) for i in range(256)]
    rcs = [l.ggms_list_heads_attach(C.byref(g), C.c_void_p(1 << 30)) for g in gs]
    try:
        assert rcs[:255] == [0] * 255 and rcs[255] == INVALID and "handles" in _err()
        assert gs[255].heads_id == 0 and len({g.heads_id for g in gs[:255]}) == 255
    finally:
        for g in gs:
            assert l.ggms_list_heads_detach(C.byref(g)) == 0
    assert l.ggms_list_heads_attach(C.byref(gs[255]), C.c_void_p(1 << 30)) == 0
    assert l.ggms_list_heads_detach(C.byref(gs[255])) == 0
