"""Q8ROW (row-scaled 8-bit) tables through the converting gathers (ggms_*_convert, include/ggms.h): every output is, bit
for bit, numpy's codes.astype(float32) * scale[:, None] + bias[:, None] narrowed by feat_convert_common.from_f32
(q8row_common.Table, computed once per table).  The tables are made so that another row's scale or bias cannot pass, the
pad bytes of every row hold 0xFF, and every output sits between canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_convert_common import BITS, F16, F32, TORCH, TORCH_BITS, tensor_bits
from q8row_common import OUT_IDS, OUTS, Q8ROW, make_table, stride

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFF
U8 = 3
CANARY = 64  # elements kept on either side of every output
# launch_chunks (xgnn_amd/csrc/extract.hip): rows of `rc >= 8192` chunks go to k_gather_long_rows (one workgroup per
# row), shorter ones to the tile sweep of k_gather_rows
LONG_ROW_CHUNKS = 8192


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


def sentinel(dt):
    return 0x5a5a5a5a if dt == F32 else 0x5a5a


def ids(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def dev_rows(rows, offset=0):
    """A device uint8 tensor holding the packed rows, its base `offset` bytes past a 256-byte boundary."""
    flat = torch.empty(rows.size + 256, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    t = flat[offset:offset + rows.size]
    t.copy_(torch.from_numpy(np.array(rows).ravel()))  # (a copy: the tables are read-only)
    return t.view(rows.shape)


class Out:
    """`rows x dim` output of dtype `dt` inside a sentinel-filled buffer: CANARY elements in front (+ `shift`, which
    misaligns the output) and behind."""

    def __init__(self, rows, dim, dt, shift=0):
        self.dt, self.n, self.lead = dt, rows * dim, CANARY + shift
        self.flat = torch.empty(self.lead + self.n + CANARY, dtype=TORCH[dt], device="cuda")
        self.flat.view(TORCH_BITS[dt]).fill_(sentinel(dt))
        self.t = self.flat[self.lead:self.lead + self.n].view(rows, dim)
        self.shape = (rows, dim)

    def untouched(self):
        return bool((tensor_bits(self.flat, self.dt) == sentinel(self.dt)).all())

    def check(self, dst_rows, want_bits, what):
        """Rows `dst_rows` hold `want_bits`, bit for bit; every other element of the buffer, canaries included, still
        holds the sentinel."""
        got = tensor_bits(self.flat, self.dt)
        body = got[self.lead:self.lead + self.n].reshape(self.shape)
        assert (got[:self.lead] == sentinel(self.dt)).all() and (got[self.lead + self.n:] == sentinel(self.dt)).all(), \
            f"{what}: bytes outside the output were written"
        untouched = np.ones(self.shape[0], bool)
        untouched[dst_rows] = False
        assert (body[untouched] == sentinel(self.dt)).all(), f"{what}: rows beyond the count / outside dst_index were written"
        bad = body[dst_rows] != want_bits
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at batch row {r} column {c}: got "
                                 f"{int(body[dst_rows][r, c]):#x}, want {int(want_bits[r, c]):#x}")


_TABLES = {}


def table(rows, dim):
    """(the table with its expected bits, its packed rows on the device), made once per shape and never written."""
    if (rows, dim) not in _TABLES:
        t = make_table(rows, dim, seed=1000 + dim)
        _TABLES[(rows, dim)] = (t, dev_rows(t.rows))
    return _TABLES[(rows, dim)]


def gather_case(ops, out_dt, dim, n, scatter=False, dev_count=False, mask=ALL_ONES, rows=512, shift=0, what=""):
    """One ggms_gather_scatter_convert call, checked.  The index starts with rows 0 .. 259 (column 0 of the first 256
    enumerates every code, 256 .. 258 are the rounding edges), continues with random rows (repeats included) and ends by
    repeating its first entries; counts that are no multiple of 64 end in a partial tile."""
    t, t_src = table(rows, dim)
    rs = np.random.RandomState(n + 7 * dim)
    n_max = n + 37 if dev_count else n  # device count below the bound: the rows past it stay untouched
    index = np.concatenate([np.arange(min(rows, 260)), rs.randint(0, rows, n_max)])[:n_max].astype(np.uint32)
    if n_max > 300:
        index[n_max - n_max // 8:] = index[:n_max // 8]  # repeats (the random part repeats rows as well)
    elif n_max > 1:
        index[-1] = index[0]
    if mask != ALL_ONES:
        index = (index.astype(np.uint64) + rs.randint(0, 1 << 20, n_max).astype(np.uint64) * (mask + 1)).astype(np.uint32)
    out_rows = n_max + 50 if scatter else n_max
    dst = rs.permutation(out_rows)[:n_max].astype(np.uint32) if scatter else np.arange(n_max, dtype=np.uint32)
    out = Out(max(out_rows, 1), dim, out_dt, shift)
    num_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if dev_count else None
    ops.gather_scatter_convert(out.t, t_src, ids(index) if n_max else torch.empty(0, dtype=torch.int32, device="cuda"),
                               ids(dst) if scatter else None, num=n_max, num_dev=num_dev, src_row_mask=mask,
                               src_dtype=ops.Q8ROW)
    out.check(dst[:n], t.want(out_dt, index[:n] & np.uint32(mask)), f"{what} dim={dim} n={n} scatter={scatter} "
              f"dev_count={dev_count} mask={mask:#x} shift={shift}")


# dims: chunks of 1 (1, 3), 2 (6, 130), 4 (4, 20, 100; the widest into f32) and 8 codes (8, 128, 768; into f16 / bf16),
# pad bytes of every length from 0 to 7, rows of fewer than 8 chunks (8 loads in flight per lane) and of more (16)
@pytest.mark.parametrize("dim", [1, 3, 4, 6, 8, 20, 100, 128, 130, 768])
@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_gather_decodes_with_the_rows_own_scale_and_bias(ops, out_dt, dim):
    for n in [0, 1, 63, 64, 65, 257, 4097]:
        gather_case(ops, out_dt, dim, n)
    for n in [65, 257]:  # dst_index scatter, the count on the device (n_max larger), both, and a row mask
        gather_case(ops, out_dt, dim, n, scatter=True)
        gather_case(ops, out_dt, dim, n, dev_count=True)
        gather_case(ops, out_dt, dim, n, scatter=True, dev_count=True, mask=255)


def test_the_table_carries_what_it_promises():
    """Every code in column 0, scales 2^20 apart and biases of either sign in neighbouring rows, rows of scale 0, and
    the rounding edges as exact f32 values."""
    t = make_table(512, 20, seed=1020)
    assert sorted(t.codes[:256, 0].tolist()) == list(range(256))
    s = np.abs(t.scale.astype(np.float64))
    both = (s[:-1] > 0) & (s[1:] > 0)
    ratio = np.maximum(s[:-1], s[1:])[both] / np.minimum(s[:-1], s[1:])[both]
    assert ratio.max() >= 2.0 ** 19 and (t.scale == 0).sum() >= 512 // 7 and (t.scale < 0).any()
    assert (np.sign(t.bias[:-1]) * np.sign(t.bias[1:]) < 0).sum() > 400
    assert (t.rows[:, 20:24] == 0xFF).all()
    f32 = t.bits[F32].view(np.float32)
    assert f32[256, 0] == 65520.0 and f32[257, 0] == 1 + 2.0 ** -11 and f32[257, 1] == 1 + 3 * 2.0 ** -11
    assert f32[258, 0] == 1 + 2.0 ** -8 and f32[258, 1] == 1 + 3 * 2.0 ** -8
    assert np.isinf(t.bits[F16].view(np.float16)[256, 0])  # 65520 is the f16 overflow tie: to even, which is inf


# the long-row kernel on both sides of its threshold, by chunk count: odd dims move in 1-code chunks (8191: tile sweep,
# 8193: long rows); 8 x 8191 and 8 x 8192 codes in 8-code chunks into the 16-bit types (tile sweep / long rows; into
# f32 both are long rows of 4-code chunks)
@pytest.mark.parametrize("dim", [LONG_ROW_CHUNKS - 1, LONG_ROW_CHUNKS + 1, 8 * (LONG_ROW_CHUNKS - 1), 8 * LONG_ROW_CHUNKS])
@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_long_rows_on_both_sides_of_the_threshold(ops, out_dt, dim):
    for scatter, dev_count in [(False, False), (True, True)]:
        gather_case(ops, out_dt, dim, 5, scatter=scatter, dev_count=dev_count, rows=8)


@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_misaligned_out_takes_a_narrower_chunk(ops, out_dt):
    """`out` one element past an aligned base: only 1-code chunks are aligned on the output side."""
    for dim in (128, 20):
        gather_case(ops, out_dt, dim, 257, shift=1, what="out offset")
        gather_case(ops, out_dt, dim, 65, scatter=True, dev_count=True, shift=1, what="out offset")


@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_a_source_base_off_the_8_byte_boundary_is_refused(ops, out_dt):
    """The trailer is read by one 8-byte load: a base 4 bytes off is GGMS_ERR_INVALID with a message, nothing launched."""
    from xgnn_amd import lib
    t = make_table(64, 20, seed=3)
    src = dev_rows(t.rows, offset=4)
    assert src.data_ptr() % 8 == 4
    out = Out(64, 20, out_dt)
    rc = lib().ggms_gather_scatter_convert(out.t.data_ptr(), src.data_ptr(), ids(np.arange(64)).data_ptr(), None, 64, None, 20,
                                           Q8ROW, out_dt, ALL_ONES,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"8-byte aligned" in lib().ggms_last_error()
    torch.cuda.synchronize()
    assert out.untouched()
    # the same through a shard pointer and through the host slot of the cached gather
    good = dev_rows(t.rows)
    for parts, host in [([src], good), ([good], src)]:
        rc = lib().ggms_extract_cached_convert(out.t.data_ptr(), ids(np.arange(64)).data_ptr(), 64, None,
                                               ids(np.arange(64)).data_ptr(), ops.part_pointer_table(parts).ptr(), 0,
                                               host.data_ptr(), 20, Q8ROW, out_dt, None,
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"8-byte aligned" in lib().ggms_last_error()
    torch.cuda.synchronize()
    assert out.untouched()


def _cache_layout(N, num_cached, seed):
    rank = np.random.RandomState(seed).permutation(N)
    tab = np.full(N, ALL_ONES, np.uint32)
    tab[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    return rank, tab


def _pinned(b):
    return torch.from_numpy(np.array(b)).pin_memory()


@pytest.fixture(scope="module")
def store():
    """One 512-node table of dim 20 behind every cached / tiered case."""
    return make_table(512, 20, seed=11)


@pytest.mark.parametrize("frac,P", [(0.0, 0), (0.3, 0), (0.3, 3), (1.0, 2)])
@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_extract_cached_convert(ops, store, out_dt, frac, P):
    """Hits from P shards (0: one array) of packed rows, misses from the pinned host table; the miss count equals that of
    the plain GGMS_U8 call at dim = stride, whose rows are the packed rows' bytes."""
    N, dim, n, st = 512, 20, 300, stride(20)
    num_cached = int(N * frac)
    b = store.rows
    rank, tab = _cache_layout(N, num_cached, 5)
    np_parts = [b[rank[:num_cached]][p::max(P, 1)] for p in range(max(P, 1))]
    parts = [dev_rows(np.ascontiguousarray(x).reshape(-1, st)) for x in np_parts]
    ptab = ops.part_pointer_table(parts)
    host = _pinned(b)
    nodes = np.random.RandomState(9).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, dim, out_dt)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, ops.Q8ROW, t_nodes, t_tab, ptab, P, host, num_miss=miss)
    out.check(np.arange(n), store.want(out_dt, nodes), f"cached frac={frac} P={P}")
    plain = torch.empty((n, st), dtype=torch.uint8, device="cuda")
    miss_plain = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached(plain, t_nodes, t_tab, ptab, P, host, num_miss=miss_plain)
    assert int(miss.item()) == int(miss_plain.item()) == int((tab[nodes] == ALL_ONES).sum())
    assert plain.cpu().numpy().tobytes() == b[nodes].tobytes()


@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_extract_cached_convert_full_cache_in_node_order(ops, store, out_dt):
    """table == NULL: slot = node id, no miss tier."""
    N, dim, n, P = 512, 20, 300, 3
    b = store.rows
    parts = [dev_rows(np.ascontiguousarray(b[p::P])) for p in range(P)]
    nodes = np.random.RandomState(2).randint(0, N, n).astype(np.uint32)
    out = Out(n, dim, out_dt)
    miss = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, ops.Q8ROW, ids(nodes), None, ops.part_pointer_table(parts), P, None, num_miss=miss)
    out.check(np.arange(n), store.want(out_dt, nodes), "full cache")
    assert int(miss.item()) == 0


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_extract_tiered_convert(ops, store, out_dt, P):
    """Replica + P shards + the host slot, all packed rows; the four tier counters equal those of the plain GGMS_U8
    call at dim = stride."""
    from xgnn_amd import lib
    N, dim, n, num_cached, R, me, st = 512, 20, 300, 260, 40, P - 1, stride(20)
    b = store.rows
    rank, tab = _cache_layout(N, num_cached, 6)
    replica = dev_rows(np.ascontiguousarray(b[rank[:R]]))
    parts = [dev_rows(np.ascontiguousarray(b[rank[R + p:num_cached:P]])) for p in range(P)]
    ptab = ops.part_pointer_table(parts)
    host = _pinned(b)
    nodes = np.random.RandomState(4).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, dim, out_dt)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.extract_tiered_convert(out.t, ops.Q8ROW, t_nodes, t_tab, replica, ptab, P, me, host, tier_rows=counters)
    out.check(np.arange(n), store.want(out_dt, nodes), f"tiered P={P}")
    t = ops._feature_tiers(t_tab, replica, ptab, P, me, host)
    plain = torch.empty((n, st), dtype=torch.uint8, device="cuda")
    counters_plain = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = lib().ggms_extract_tiered(plain.data_ptr(), t_nodes.data_ptr(), n, None, C.byref(t), st, U8,
                                   counters_plain.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    slots = tab[nodes].astype(np.int64)
    missed, shard = tab[nodes] == ALL_ONES, (slots - R) % P
    hit = ~missed
    want = [int(missed.sum()), int((hit & (slots >= R) & (shard != me)).sum()),
            int((hit & (slots >= R) & (shard == me)).sum()), int((hit & (slots < R)).sum())]
    assert counters.cpu().tolist() == counters_plain.cpu().tolist() == want and sum(want) == n
    assert plain.cpu().numpy().tobytes() == b[nodes].tobytes()


def test_the_plain_byte_gather_moves_the_packed_rows(ops):
    """A Q8ROW table that has to move as bytes is a GGMS_U8 table of dim = stride: trailer and pad bytes included."""
    for dim, n in [(100, 1000), (128, 257), (3, 65)]:
        t, t_src = table(512, dim)
        index = np.random.RandomState(1).randint(0, 512, n).astype(np.uint32)
        out = torch.zeros((n, stride(dim)), dtype=torch.uint8, device="cuda")
        ops.gather_scatter(out, t_src, ids(index), None)
        assert out.cpu().numpy().tobytes() == t.rows[index].tobytes()


def test_illegal_pairs_launch_nothing(ops):
    """Q8ROW is a source of the converting gathers into F32 / F16 / BF16 and nothing else: as an output, into U8 or FP8,
    into itself, or through a plain entry point it is GGMS_ERR_INVALID with a message."""
    from xgnn_amd import lib
    h = lib()
    out = torch.full((8, 16), 0x5a, dtype=torch.uint8, device="cuda")
    src = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    for src_dt, dst_dt in [(F32, Q8ROW), (F16, Q8ROW), (U8, Q8ROW), (16, Q8ROW), (Q8ROW, U8), (Q8ROW, 16), (Q8ROW, 17),
                           (Q8ROW, Q8ROW), (Q8ROW, 1), (Q8ROW, 6)]:
        assert h.ggms_gather_scatter_convert(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, src_dt,
                                             dst_dt, ALL_ONES, s) == -1, (src_dt, dst_dt)
        assert b"no conversion" in h.ggms_last_error(), (src_dt, dst_dt, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         Q8ROW, None, s) == -1 and b"no conversion" in h.ggms_last_error()
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, Q8ROW, U8, None,
                                         s) == -1 and b"no conversion" in h.ggms_last_error()
    # the plain entry points: no element size, the existing invalid-argument refusal
    assert h.ggms_extract(out.data_ptr(), src.data_ptr(), index.data_ptr(), 8, 4, Q8ROW, s) == -1
    assert len(h.ggms_last_error()) > 0
    assert h.ggms_gather_scatter(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, Q8ROW, s) == -1
    assert len(h.ggms_last_error()) > 0
    assert h.ggms_gather_scatter_masked(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, Q8ROW, 7,
                                        s) == -1 and b"no conversion" in h.ggms_last_error()
    assert h.ggms_extract_cached(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, Q8ROW, None,
                                 s) == -1
    assert h.ggms_extract_tiered(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, Q8ROW, None, s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a).all()
