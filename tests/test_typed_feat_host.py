"""Typed feature tables, host side: the two statements of ggms_gather_typed (tests/typed_feat_ref.py) agree, the dataset
writer's node_feat= files, meta keys and refusals, and the leaf's argument refusals and size arithmetic -- all of which
come before any device call, so they run without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import feat_formats as ff
import typed_feat_ref as ref
from feat_formats import BF16, F16, F32

torch = pytest.importorskip("torch")

SPECS = [(3, F32, F32), (8, F16, F32), None, (129, BF16, BF16), (100, F32, F16), (4, F16, BF16), (1, F16, F16)]


def small_case(T, n, seed, with_rank=True):
    rng = np.random.RandomState(seed)
    N = 400
    node_type = rng.randint(0, T, N).astype(np.uint8)
    rank = np.zeros(N, np.uint32)
    tables, groups = [], []
    cuts = np.sort(rng.randint(0, n + 1, T - 1))
    counts = np.diff(np.concatenate([[0], cuts, [n]]))
    for t in range(T):
        at = np.flatnonzero(node_type == t)
        rank[at] = np.arange(at.size)
        pool = at if at.size else np.array([0])
        g = pool[rng.randint(0, pool.size, counts[t])].astype(np.uint32)
        if g.size > 2:
            g[0], g[-1] = N + 3, 0xFFFFFFFF  # ids that are no node
        groups.append(g)
        spec = SPECS[t % len(SPECS)]
        if spec is None:
            tables.append(None)
            continue
        dim, src, out = spec
        rows = max(1, at.size - 2)  # the last two ranks lie beyond the table
        bits = ref.hashed_bits(t, rows, dim, src)
        if src != out:
            bits[np.isnan(ff.to_f32(bits, src))] = 0
        tables.append(dict(bits=bits, src=src, out=out, first_node=int(pool[0])))
    typed = np.concatenate(groups + [np.zeros(5, np.uint32)])
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return tables, typed, base, (rank if with_rank else None), N


@pytest.mark.parametrize("with_rank", [True, False])
@pytest.mark.parametrize("T", [1, 2, 5, 32])
def test_numpy_statement_equals_loop_statement(T, with_rank):
    for n in (0, 1, 40, 97):
        tables, typed, base, rank, N = small_case(T, n, 10 * T + n, with_rank)
        for max_nodes in (typed.size, n // 2):
            a = ref.gather_typed(tables, typed, base, max_nodes, rank, N)
            b = ref.gather_typed_loops(tables, typed, base, max_nodes, rank, N)
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[0], b[0])
            assert a[0].size == a[1][-1] <= ref.out_bytes(tables, max_nodes)


def test_offsets_are_16_byte_rounded_and_a_type_without_a_table_takes_no_bytes():
    tables = [dict(bits=np.zeros((9, 3), np.uint32), src=F32, out=F32, first_node=0), None,
              dict(bits=np.zeros((9, 5), np.uint16), src=F16, out=F16, first_node=0),
              dict(bits=np.zeros((9, 5), np.uint16), src=F16, out=F32, first_node=0)]
    off = ref.offsets(tables, [0, 3, 10, 13, 14], 100)
    assert off.tolist() == [0, 48, 48, 80, 112]  # 36 -> 48; nothing; 30 -> 32; 20 -> 32
    assert ref.offsets(tables, [0, 3, 10, 13, 14], 11).tolist() == [0, 48, 48, 64, 64]  # clamped at max_nodes = 11
    assert ref.offsets(tables, [0, 5, 2, 7, 7], 100).tolist() == [0, 64, 64, 96, 96]  # a word that runs backwards: empty
    out, _ = ref.gather_typed(tables, np.zeros(14, np.uint32), [0, 3, 10, 13, 14], 100, None, 1)
    assert out.size == 112 and not out.any()


# ---- the dataset -------------------------------------------------------------------------------------------------------
def tiny_graph(n=60):
    ip = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    ix = (np.arange(2 * n, dtype=np.uint32) * 7 + 1) % n
    return dict(indptr=ip, indices=ix, train_set=np.arange(10, dtype=np.uint32), meta=dict(feat_dim=4, num_class=3))


def write(path, node_feat, **kw):
    from xgnn_amd import datagen
    g = tiny_graph()
    n = g["indptr"].size - 1
    kw.setdefault("node_type", (np.arange(n) * 5 % 3).astype(np.uint8))
    kw.setdefault("num_node_type", 3)
    if kw["node_type"] is None:
        kw.pop("node_type"), kw.pop("num_node_type")
    feat = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
    return datagen.write_dataset(str(path), g, feat=feat, label=np.zeros(n, np.int64), node_feat=node_feat, **kw)


def read_meta(path):
    return dict(line.rstrip("\n").split("\t") for line in open(os.path.join(path, "meta.txt")))


def test_written_files_and_meta_keys_round_trip(tmp_path):
    nt = (np.arange(60) * 5 % 3).astype(np.uint8)
    rs = np.random.RandomState(0)
    a0 = rs.standard_normal((20, 16)).astype(np.float32)
    a2 = torch.from_numpy(rs.standard_normal((20, 40)).astype(np.float32)).to(torch.bfloat16)
    path = write(tmp_path / "d", [a0, None, a2])
    meta = read_meta(path)
    assert (meta["NODE_FEAT_DIM_0"], meta["NODE_FEAT_DIM_1"], meta["NODE_FEAT_DIM_2"]) == ("16", "0", "40")
    assert (meta["NODE_FEAT_DATA_TYPE_0"], meta["NODE_FEAT_DATA_TYPE_2"]) == ("F32", "BF16")
    assert meta["FEAT_DIM"] == "4" and meta["NUM_NODE_TYPE"] == "3"
    assert os.path.getsize(os.path.join(path, "feat.bin")) == 60 * 4 * 4  # the one-table file is written as before
    np.testing.assert_array_equal(np.fromfile(os.path.join(path, "node_feat_0.bin"), np.float32).reshape(20, 16), a0)
    np.testing.assert_array_equal(np.fromfile(os.path.join(path, "node_feat_2.bin"), np.uint16).reshape(20, 40),
                                  a2.view(torch.int16).numpy().view(np.uint16))
    assert not os.path.exists(os.path.join(path, "node_feat_1.bin"))
    assert (np.bincount(nt) == 20).all()
    # float16 through numpy
    path = write(tmp_path / "e", [None, a0.astype(np.float16), None])
    assert read_meta(path)["NODE_FEAT_DATA_TYPE_1"] == "F16"
    assert os.path.getsize(os.path.join(path, "node_feat_1.bin")) == 20 * 16 * 2
    # without node_feat nothing new is written
    path = write(tmp_path / "f", None)
    assert not any(k.startswith("NODE_FEAT") for k in read_meta(path))


@pytest.mark.parametrize("node_feat, kw, message", [
    ([np.zeros((20, 4), np.float32)] * 3, dict(node_type=None), "node_feat: needs node_type"),
    ([np.zeros((20, 4), np.float32)] * 2, {}, r"node_feat: one entry per node type \(3\), not 2"),
    ([np.zeros((19, 4), np.float32), None, None], {}, r"node_feat\[0\]: one row per node of type 0 \(20\), not 19"),
    ([None, None, np.zeros((21, 4), np.float16)], {}, r"node_feat\[2\]: one row per node of type 2 \(20\), not 21"),
    ([None, np.zeros(20, np.float32), None], {}, r"node_feat\[1\]: a 2-d \(rows, dim\) array, not rank 1"),
    ([None, np.zeros((20, 2, 2), np.float32), None], {}, r"node_feat\[1\]: a 2-d \(rows, dim\) array, not rank 3"),
    ([np.zeros((20, 4), np.float64), None, None], {}, r"node_feat\[0\]: dtype float64 \(F32, F16 or BF16\)"),
    ([None, None, np.zeros((20, 4), np.int32)], {}, r"node_feat\[2\]: dtype int32 \(F32, F16 or BF16\)"),
    ([None, torch.zeros((20, 4), dtype=torch.float8_e5m2), None], {},
     r"node_feat\[1\]: dtype torch.float8_e5m2 \(F32, F16 or BF16\)"),
    ([np.zeros((20, 0), np.float32), None, None], {}, r"node_feat\[0\]: rows of dim 0"),
])
def test_every_write_dataset_refusal_fires_by_name(tmp_path, node_feat, kw, message):
    with pytest.raises(AssertionError, match=message):
        write(tmp_path / "d", node_feat, **kw)


# ---- the leaf's arguments ----------------------------------------------------------------------------------------------
def c_tables(entries):
    """entries: (table address, num_rows, dim, src, out, first_node) per type"""
    from xgnn_amd import _lib
    arr = (_lib.TypedTable * max(1, len(entries)))()
    for t, e in enumerate(entries):
        arr[t] = _lib.TypedTable(*e)
    return arr


INVALID = -1  # GGMS_ERR_INVALID
A = 0x10000  # an address that is only ever looked at, never followed


def call(entries, out=A, out_bytes=1 << 40, T=None, typed=A, base=A, max_nodes=100, off=A, tables="given"):
    from xgnn_amd import _lib
    h = _lib.lib()
    ct = c_tables(entries) if tables == "given" else None
    rc = h.ggms_gather_typed(out, out_bytes, ct, len(entries) if T is None else T, typed, base, max_nodes, None, 0, off, None)
    return rc, h.ggms_last_error().decode()


GOOD = [(A, 10, 8, F32, F32, 0), (0, 0, 0, 0, 0, 0), (A, 10, 40, F16, F32, 0)]


@pytest.mark.parametrize("kw, message", [
    (dict(tables=None), "tables is NULL"),
    (dict(T=0), "num_type 0"),
    (dict(entries=GOOD * 11, T=33), "num_type 33"),
    (dict(out=None), "out is NULL"),
    (dict(typed=None), "typed_nodes is NULL"),
    (dict(base=None), "base_dev is NULL"),
    (dict(off=None), "out_offset_dev is NULL"),
    (dict(max_nodes=(1 << 32) - 1024), "max_nodes 4294966272"),
    (dict(entries=[(A, 10, 8, 1, F32, 0)]), r"tables\[0\].src_dtype 1"),
    (dict(entries=GOOD[:2] + [(A, 10, 8, F16, 16, 0)]), r"tables\[2\].out_dtype 16"),
    (dict(entries=[(A, 10, 8, 18, 18, 0)]), r"tables\[0\].src_dtype 18"),
    (dict(entries=[(0, 10, 8, F32, F32, 0)]), r"tables\[0\].table is NULL"),
    (dict(entries=GOOD[:2] + [(A + 1, 10, 8, F16, F16, 0)]), r"tables\[2\].table is not aligned to its 2-byte element"),
    (dict(entries=[(A + 2, 10, 8, F32, F16, 0)]), r"tables\[0\].table is not aligned to its 4-byte element"),
    (dict(out=A + 2), r"out is not aligned to the 4-byte element of type 0"),
    (dict(entries=[(A, 10, 8, F16, BF16, 0)], out=A + 1), r"out is not aligned to the 2-byte element of type 0"),
    (dict(out_bytes=100 * 160 + 47), "out_bytes 16047 is below ggms_gather_typed_out_bytes = 16048"),
    (dict(entries=[(A, 10, 8192 * 4, F32, F32, 0)]), r"tables\[0\].dim 32768 is a row of 8192 chunks"),
    (dict(entries=[(A + 4, 10, 8192, F32, F32, 0)]), r"tables\[0\].dim 8192 is a row of 8192 chunks"),
    (dict(entries=[(A, 10, 8192 * 4, F16, F32, 0)]), r"tables\[0\].dim 32768 is a row of 8192 chunks"),
])
def test_every_leaf_argument_refusal_fires_by_argument_name(kw, message):
    kw = dict(kw)
    rc, err = call(kw.pop("entries", GOOD), **kw)
    assert rc == INVALID, err
    import re
    assert err.startswith("ggms_gather_typed: invalid argument: ") and re.search(message, err), err


def test_the_widest_rows_below_the_bound_are_not_refused_for_their_width():
    """8191 chunks pass the argument checks (the call then fails at its first device call on a host without a GPU, or
    would run on one: so only out_bytes is made to refuse, which is the last check)."""
    rc, err = call([(A, 10, 8191 * 4, F32, F32, 0)], out_bytes=0)
    assert rc == INVALID and "out_bytes 0 is below" in err


def test_out_bytes_values():
    from xgnn_amd import _lib
    h = _lib.lib()
    f = h.ggms_gather_typed_out_bytes
    assert f(c_tables(GOOD), 3, 100) == 100 * 160 + 48
    assert f(c_tables(GOOD), 3, 0) == 48
    assert f(c_tables(GOOD[:1]), 1, 7) == 7 * 32 + 16
    assert f(c_tables([GOOD[1]] * 4), 4, 1000) == 64  # no type has a table
    assert f(c_tables([(A, 1, 100, F32, BF16, 0), (A, 1, 90, F16, F32, 0)]), 2, 10) == 10 * 360 + 32
    assert f(c_tables(GOOD), 3, (1 << 32) - 1025) == ((1 << 32) - 1025) * 160 + 48
    # out of range: 0
    assert f(None, 3, 100) == 0 and f(c_tables(GOOD), 0, 100) == 0 and f(c_tables(GOOD * 11), 33, 100) == 0
    assert f(c_tables(GOOD), 3, (1 << 32) - 1024) == 0
    assert f(c_tables([(A, 10, 8, 1, F32, 0)]), 1, 100) == 0 and f(c_tables([(A, 10, 8, F32, 3, 0)]), 1, 100) == 0
    for tables, n in ((GOOD, 100), (GOOD[:1], 7)):
        spec = [None if e[2] == 0 else dict(bits=np.zeros((1, e[2]), ff.BITS[e[3]]), src=e[3], out=e[4], first_node=0)
                for e in tables]
        assert f(c_tables(tables), len(tables), n) == ref.out_bytes(spec, n)


def test_abi_version_and_counts_words_are_unchanged():
    from xgnn_amd import _lib
    assert _lib.lib().ggms_abi_version() == 3 == _lib.ABI_VERSION
    assert [_lib.COUNTS_WORDS(L) for L in (1, 2, 3, 16)] == [11, 14, 17, 56]
    assert C.sizeof(_lib.TypedTable) == 32
