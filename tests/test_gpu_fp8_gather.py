"""FP8 (E4M3 / E5M2) tables through the converting gathers (ggms_*_convert, include/ggms.h): every output is the CPU cast
of the closed-form truth table (fp8_common.truth, checked against torch in test_fp8_decode_table.py) -- bitwise, because
every finite code is exact in f32, f16 and bf16; NaN codes must give NaN; -0.0 stays -0.0."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_convert_common import BITS, F16, F32, TORCH, TORCH_BITS, tensor_bits
from fp8_common import (E4M3, E5M2, FP8, FP8_NAMES, FP8_PAIRS, FP8_TORCH, OUTS, assert_decoded, decode_bits, table_bytes)

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFF
CANARY = 64  # elements kept on either side of every output
# launch_chunks (xgnn_amd/csrc/extract.hip): rows of `rc >= 8192` chunks go to k_gather_long_rows (one workgroup per
# row), shorter ones to the tile sweep of k_gather_rows
LONG_ROW_CHUNKS = 8192
PAIR_IDS = [f"{FP8_NAMES[s]}-{ {0: 'F32', 2: 'F16', 7: 'BF16'}[d]}" for s, d in FP8_PAIRS]


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


def sentinel(dt):
    return 0x5a5a5a5a if dt == F32 else 0x5a5a


def ids(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def dev_table(b, fmt, offset=0):
    """A device tensor of the FP8 dtype holding bytes `b`, its base `offset` bytes past a 256-byte boundary."""
    flat = torch.empty(b.size + 256, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    t = flat[offset:offset + b.size]
    t.copy_(torch.from_numpy(b.ravel()))
    return t.view(b.shape).view(FP8_TORCH[fmt])


class Out:
    """`rows x dim` output of dtype `dt` inside a sentinel-filled buffer: CANARY elements in front (+ `shift`, which
    misaligns the output) and behind."""

    def __init__(self, rows, dim, dt, shift=0):
        self.dt, self.n, self.lead = dt, rows * dim, CANARY + shift
        self.flat = torch.empty(self.lead + self.n + CANARY, dtype=TORCH[dt], device="cuda")
        self.flat.view(TORCH_BITS[dt]).fill_(sentinel(dt))
        self.t = self.flat[self.lead:self.lead + self.n].view(rows, dim)
        self.want = np.full((rows, dim), sentinel(dt), BITS[dt])  # rows no call writes keep the sentinel

    def check(self, src_bytes, fmt, what):
        """Rows whose source bytes are given in `src_bytes` (a dict row -> bytes, or an array for all rows) are decoded;
        every other element of the buffer, canaries included, still holds the sentinel."""
        got = tensor_bits(self.flat, self.dt)
        body = got[self.lead:self.lead + self.n].reshape(self.want.shape)
        assert (got[:self.lead] == sentinel(self.dt)).all() and (got[self.lead + self.n:] == sentinel(self.dt)).all(), \
            f"{what}: bytes outside the output were written"
        rows, b = src_bytes
        untouched = np.ones(self.want.shape[0], bool)
        untouched[rows] = False
        assert (body[untouched] == sentinel(self.dt)).all(), f"{what}: rows beyond the count / outside dst_index were written"
        assert_decoded(body[rows], b, fmt, self.dt, what)


_TABLES = {}


def table(fmt, rows, dim, offset=0):
    key = (fmt, rows, dim, offset)
    if key not in _TABLES:
        b = table_bytes((rows, dim), seed=fmt * 1000 + dim)
        _TABLES[key] = (b, dev_table(b, fmt, offset))
    return _TABLES[key]


def gather_case(ops, fmt, out_dt, dim, n, scatter=False, dev_count=False, mask=ALL_ONES, rows=512, offset=0, shift=0,
                what=""):
    """One ggms_gather_scatter_convert call, checked.  The index starts with rows 0 .. 255 (column 0 of those rows
    enumerates every code), continues with random rows (repeats included) and ends by repeating its first entries."""
    b, t_src = table(fmt, rows, dim, offset)
    rs = np.random.RandomState(n + 7 * dim)
    n_max = n + 37 if dev_count else n  # device count below the bound: the rows past it stay untouched
    index = np.concatenate([np.arange(min(rows, 256)), rs.randint(0, rows, n_max)])[:n_max].astype(np.uint32)
    index[n_max - n_max // 4:] = index[:n_max // 4]  # repeats
    if mask != ALL_ONES:
        index = (index.astype(np.uint64) + rs.randint(0, 1 << 20, n_max).astype(np.uint64) * (mask + 1)).astype(np.uint32)
    out_rows = n_max + 50 if scatter else n_max
    dst = rs.permutation(out_rows)[:n_max].astype(np.uint32) if scatter else np.arange(n_max, dtype=np.uint32)
    out = Out(max(out_rows, 1), dim, out_dt, shift)
    num_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if dev_count else None
    ops.gather_scatter_convert(out.t, t_src, ids(index) if n_max else torch.empty(0, dtype=torch.int32, device="cuda"),
                               ids(dst) if scatter else None, num=n_max, num_dev=num_dev, src_row_mask=mask)
    out.check((dst[:n], b[index[:n] & np.uint32(mask)]), fmt, f"{what} dim={dim} n={n} scatter={scatter} "
              f"dev_count={dev_count} mask={mask:#x} offset={offset} shift={shift}")


# dims: chunks of 1 (1, 3), 2 (6, 130), 4 (4, 20, 100; the widest into f32) and 8 elements (8, 128, 768, 1032; into f16 /
# bf16), rows of fewer than 8 chunks (8 loads in flight per lane) and of more (16), tiles whose chunk count is no
# multiple of the 64 lanes x loads in flight, and this feature's real shapes
@pytest.mark.parametrize("dim", [1, 3, 4, 6, 8, 20, 100, 128, 130, 768, 1032])
@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_gather_decodes_every_code(ops, pair, dim):
    fmt, out_dt = pair
    for n in [0, 1, 63, 64, 65, 257, 4097]:
        gather_case(ops, fmt, out_dt, dim, n)
    for n in [65, 257]:  # dst_index scatter, the count on the device (n_max larger), both, and a row mask
        gather_case(ops, fmt, out_dt, dim, n, scatter=True)
        gather_case(ops, fmt, out_dt, dim, n, dev_count=True)
        gather_case(ops, fmt, out_dt, dim, n, scatter=True, dev_count=True, mask=255)


# the long-row kernel on both sides of its threshold, by chunk count: odd dims move in 1-element chunks (8191: tile
# sweep, 8193: long rows); 8 x 8191 and 8 x 8192 elements in 8-element chunks into the 16-bit types (tile sweep / long
# rows; into f32 both are long rows of 4-element chunks)
@pytest.mark.parametrize("dim", [LONG_ROW_CHUNKS - 1, LONG_ROW_CHUNKS + 1, 8 * (LONG_ROW_CHUNKS - 1), 8 * LONG_ROW_CHUNKS])
@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_long_rows_on_both_sides_of_the_threshold(ops, pair, dim):
    fmt, out_dt = pair
    for scatter, dev_count in [(False, False), (True, True)]:
        gather_case(ops, fmt, out_dt, dim, 5, scatter=scatter, dev_count=dev_count, rows=8)


@pytest.mark.parametrize("offset", [1, 2, 4])
@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_misaligned_table_takes_a_narrower_chunk(ops, pair, offset):
    """The table's base 1, 2 and 4 bytes past a 16-byte boundary: chunks of 1, 2 and 4 elements are what stays aligned."""
    fmt, out_dt = pair
    for dim in (128, 20):
        gather_case(ops, fmt, out_dt, dim, 257, offset=offset, what="table offset")
        gather_case(ops, fmt, out_dt, dim, 65, scatter=True, offset=offset, what="table offset")


@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_misaligned_out_takes_a_narrower_chunk(ops, pair):
    """`out` one element past an aligned base: only 1-element chunks are aligned on the output side."""
    fmt, out_dt = pair
    for dim in (128, 20):
        gather_case(ops, fmt, out_dt, dim, 257, shift=1, what="out offset")
        gather_case(ops, fmt, out_dt, dim, 65, scatter=True, dev_count=True, shift=1, what="out offset")


def _cache_layout(N, num_cached, seed):
    rank = np.random.RandomState(seed).permutation(N)
    tab = np.full(N, ALL_ONES, np.uint32)
    tab[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    return rank, tab


def _pinned(b):
    return torch.from_numpy(b).pin_memory()


@pytest.mark.parametrize("frac,P", [(0.0, 0), (0.3, 0), (0.3, 3), (1.0, 2)])
@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_extract_cached_convert(ops, pair, frac, P):
    """Hits from P shards (0: one array) of FP8 rows, misses from the pinned FP8 host table; the miss count equals the
    plain call's, whose rows are the table's bytes."""
    fmt, out_dt = pair
    N, dim, n = 500, 20, 300
    num_cached = int(N * frac)
    b = table_bytes((N, dim), seed=11 + fmt)
    rank, tab = _cache_layout(N, num_cached, 5)
    np_parts = [b[rank[:num_cached]][p::max(P, 1)] for p in range(max(P, 1))]
    parts = [dev_table(np.ascontiguousarray(x).reshape(-1, dim), fmt) for x in np_parts]
    ptab = ops.part_pointer_table(parts)
    host = _pinned(b)
    nodes = np.random.RandomState(9).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, dim, out_dt)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, FP8_TORCH[fmt], t_nodes, t_tab, ptab, P, host, num_miss=miss)
    out.check((np.arange(n), b[nodes]), fmt, f"cached frac={frac} P={P}")
    plain = torch.empty((n, dim), dtype=FP8_TORCH[fmt], device="cuda")
    miss_plain = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached(plain, t_nodes, t_tab, ptab, P, host, num_miss=miss_plain)
    assert int(miss.item()) == int(miss_plain.item()) == int((tab[nodes] == ALL_ONES).sum())
    assert plain.view(torch.uint8).cpu().numpy().tobytes() == b[nodes].tobytes()


@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_extract_cached_convert_full_cache_in_node_order(ops, pair):
    """table == NULL: slot = node id, no miss tier."""
    fmt, out_dt = pair
    N, dim, n, P = 500, 20, 300, 3
    b = table_bytes((N, dim), seed=12 + fmt)
    parts = [dev_table(np.ascontiguousarray(b[p::P]), fmt) for p in range(P)]
    nodes = np.random.RandomState(2).randint(0, N, n).astype(np.uint32)
    out = Out(n, dim, out_dt)
    miss = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, FP8_TORCH[fmt], ids(nodes), None, ops.part_pointer_table(parts), P, None, num_miss=miss)
    out.check((np.arange(n), b[nodes]), fmt, "full cache")
    assert int(miss.item()) == 0


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("pair", FP8_PAIRS, ids=PAIR_IDS)
def test_extract_tiered_convert(ops, pair, P):
    """Replica + P shards + the host slot, all FP8; the four tier counters equal the plain call's."""
    from xgnn_amd import lib
    fmt, out_dt = pair
    N, dim, n, num_cached, R, me = 512, 20, 300, 260, 40, P - 1
    b = table_bytes((N, dim), seed=13 + fmt)
    rank, tab = _cache_layout(N, num_cached, 6)
    replica = dev_table(np.ascontiguousarray(b[rank[:R]]), fmt)
    parts = [dev_table(np.ascontiguousarray(b[rank[R + p:num_cached:P]]), fmt) for p in range(P)]
    ptab = ops.part_pointer_table(parts)
    host = _pinned(b)
    nodes = np.random.RandomState(4).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, dim, out_dt)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.extract_tiered_convert(out.t, FP8_TORCH[fmt], t_nodes, t_tab, replica, ptab, P, me, host, tier_rows=counters)
    out.check((np.arange(n), b[nodes]), fmt, f"tiered P={P}")
    t = ops._feature_tiers(t_tab, replica, ptab, P, me, host)
    plain = torch.empty((n, dim), dtype=FP8_TORCH[fmt], device="cuda")
    counters_plain = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = lib().ggms_extract_tiered(plain.data_ptr(), t_nodes.data_ptr(), n, None, C.byref(t), dim, fmt,
                                   counters_plain.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    slots = tab[nodes].astype(np.int64)
    missed, shard = tab[nodes] == ALL_ONES, (slots - R) % P
    hit = ~missed
    want = [int(missed.sum()), int((hit & (slots >= R) & (shard != me)).sum()),
            int((hit & (slots >= R) & (shard == me)).sum()), int((hit & (slots < R)).sum())]
    assert counters.cpu().tolist() == counters_plain.cpu().tolist() == want and sum(want) == n
    assert plain.view(torch.uint8).cpu().numpy().tobytes() == b[nodes].tobytes()


@pytest.mark.parametrize("fmt", FP8, ids=[FP8_NAMES[f] for f in FP8])
def test_same_dtype_is_the_plain_byte_gather(ops, fmt):
    """src_dtype == out_dtype == F8*: the rows' bytes, as ggms_gather_scatter_masked moves a U8 table."""
    from xgnn_amd import lib
    for dim, n in [(100, 1000), (128, 257), (3, 65)]:
        b, t_src = table(fmt, 512, dim)
        index = np.random.RandomState(1).randint(0, 1 << 31, n).astype(np.uint32)
        t_index = ids(index)
        out = torch.zeros((n, dim), dtype=FP8_TORCH[fmt], device="cuda")
        ops.gather_scatter_convert(out, t_src, t_index, None, src_row_mask=511)
        ref = torch.zeros((n, dim), dtype=torch.uint8, device="cuda")
        rc = lib().ggms_gather_scatter_masked(ref.data_ptr(), t_src.data_ptr(), t_index.data_ptr(), None, n, None, dim, 3,
                                              511, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert out.view(torch.uint8).cpu().numpy().tobytes() == ref.cpu().numpy().tobytes() == b[index & 511].tobytes()
        plain = torch.zeros((n, dim), dtype=FP8_TORCH[fmt], device="cuda")
        ops.gather_scatter(plain, t_src, ids(index & 511), None)
        assert plain.view(torch.uint8).cpu().numpy().tobytes() == b[index & 511].tobytes()


def test_illegal_pairs_launch_nothing(ops):
    """FP8 is a source only: as the output of another source, or of the other FP8 format, it is GGMS_ERR_INVALID with a
    message; codes 8 .. 15 stay unknown."""
    from xgnn_amd import lib
    h = lib()
    out = torch.full((8, 4), 0x5a, dtype=torch.uint8, device="cuda")
    src = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    for src_dt, dst_dt, word in [(F32, E4M3, b"conversion"), (F32, E5M2, b"conversion"), (F16, E4M3, b"conversion"),
                                 (E4M3, E5M2, b"conversion"), (E5M2, E4M3, b"conversion"), (E4M3, 3, b"conversion"),
                                 (E4M3, 8, b"invalid argument"), (12, F32, b"invalid argument")]:
        assert h.ggms_gather_scatter_convert(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, src_dt,
                                             dst_dt, ALL_ONES, s) == -1, (src_dt, dst_dt)
        assert word in h.ggms_last_error() and len(h.ggms_last_error()) > 0, (src_dt, dst_dt, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         E4M3, None, s) == -1
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, F16, E5M2, None,
                                         s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a).all()
