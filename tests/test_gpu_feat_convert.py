"""The converting gathers (ggms_*_convert, include/ggms.h) against numpy / torch conversions on the CPU, bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from feat_convert_common import (BF16, BITS, F16, F32, NAMES, PAIRS, TORCH, TORCH_BITS, assert_same_bits, convert_bits,
                                 table_bits, tensor_bits)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a5a5a
ALL_ONES = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


def dev_bits(bits, dt):
    """A device tensor of dtype TORCH[dt] holding these raw bits."""
    return torch.from_numpy(bits.view(np.int32 if dt == F32 else np.int16)).cuda().view(TORCH[dt])


def sentinel_out(rows, dim, dt):
    t = torch.empty((rows, dim), dtype=TORCH[dt], device="cuda")
    t.view(TORCH_BITS[dt]).fill_(SENTINEL & 0x7fff if dt != F32 else SENTINEL)
    return t


def sentinel_bits(shape, dt):
    return np.full(shape, SENTINEL & 0x7fff if dt != F32 else SENTINEL, BITS[dt])


def ids(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


_TABLES = {}


def table(dt, rows, dim):
    """(raw bits, device tensor) of one table per (dtype, shape): built once, never written."""
    key = (dt, rows, dim)
    if key not in _TABLES:
        bits = table_bits(dt, (rows, dim), seed=dt * 1000 + dim)
        _TABLES[key] = (bits, dev_bits(bits, dt))
    return _TABLES[key]


def run_gather(ops, src_dt, dst_dt, dim, n, scatter, dev_count, mask, rows=2048, seed=0):
    """One ggms_gather_scatter_convert call and its expected output bits."""
    bits, t_src = table(src_dt, rows, dim)
    rs = np.random.RandomState(seed + n + 7 * dim)
    n_max = n + 37 if dev_count else n  # device count below the bound: the rows past it keep the sentinel
    index = rs.randint(0, 1 << 32, n_max, dtype=np.uint64).astype(np.uint32) if mask != ALL_ONES \
        else rs.randint(0, rows, n_max).astype(np.uint32)
    out_rows = n_max + 50 if scatter else n_max
    dst = rs.permutation(out_rows)[:n_max].astype(np.uint32) if scatter else np.arange(n_max, dtype=np.uint32)
    out = sentinel_out(max(out_rows, 1), dim, dst_dt)
    num_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if dev_count else None
    ops.gather_scatter_convert(out, t_src, ids(index) if n_max else torch.empty(0, dtype=torch.int32, device="cuda"),
                               ids(dst) if scatter else None, num=n_max, num_dev=num_dev, src_row_mask=mask)
    want = sentinel_bits((max(out_rows, 1), dim), dst_dt)
    want[dst[:n]] = convert_bits(bits[index[:n] & np.uint32(mask)], src_dt, dst_dt)
    return tensor_bits(out, dst_dt), want


# dim: chunks of 1, 1, 2 and 4 elements, then the widest chunk a pair has (8 between the 16-bit types, else 4); rows of
# fewer than 8 chunks keep 8 loads in flight per lane (dims 1, 7, 6; 32 between the 16-bit types), the others 16
@pytest.mark.parametrize("dim", [1, 7, 6, 100, 32, 128])
@pytest.mark.parametrize("pair", PAIRS, ids=[f"{NAMES[s]}-{NAMES[d]}" for s, d in PAIRS])
def test_gather_scatter_convert(ops, pair, dim):
    """Every pair x every row shape, over n x {identity, dst_index} x {host count, device count} x {no mask, 2^4 - 1}."""
    src_dt, dst_dt = pair
    for n, scatter, dev_count, mask in itertools.product([0, 1, 63, 64, 65, 1000], [False, True], [False, True],
                                                         [ALL_ONES, 15]):
        got, want = run_gather(ops, src_dt, dst_dt, dim, n, scatter, dev_count, mask)
        assert_same_bits(got, want, dst_dt, f"n={n} scatter={scatter} dev_count={dev_count} mask={mask:#x}")


@pytest.mark.parametrize("pair", [(F16, F32), (F32, BF16)], ids=["F16-F32", "F32-BF16"])
def test_long_rows(ops, pair):
    """dim 65536 = 16384 chunks of 4 elements: the one-workgroup-per-row kernel."""
    src_dt, dst_dt = pair
    for scatter in (False, True):
        got, want = run_gather(ops, src_dt, dst_dt, 65536, 3, scatter, False, ALL_ONES, rows=8)
        assert_same_bits(got, want, dst_dt, f"scatter={scatter}")


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{NAMES[s]}-{NAMES[d]}" for s, d in PAIRS])
def test_misaligned_out_takes_a_narrower_chunk_and_gives_the_same_bits(ops, pair):
    """`out` two elements past an aligned base: only 2-element chunks are still aligned on the output side."""
    src_dt, dst_dt = pair
    dim, n = 128, 65
    bits, t_src = table(src_dt, 2048, dim)
    index = np.random.RandomState(3).randint(0, 2048, n).astype(np.uint32)
    flat = torch.zeros(n * dim + 8, dtype=TORCH[dst_dt], device="cuda")
    out = flat[2:2 + n * dim].view(n, dim)
    assert out.data_ptr() == flat.data_ptr() + 2 * flat.element_size()
    ops.gather_scatter_convert(out, t_src, ids(index), None)
    assert_same_bits(tensor_bits(out, dst_dt), convert_bits(bits[index], src_dt, dst_dt), dst_dt)
    assert not flat[:2].view(TORCH_BITS[dst_dt]).any() and not flat[2 + n * dim:].view(TORCH_BITS[dst_dt]).any()


def _cache_layout(N, num_cached, seed):
    rs = np.random.RandomState(seed)
    rank = rs.permutation(N)
    tab = np.full(N, ALL_ONES, np.uint32)
    tab[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    return rank, tab


@pytest.mark.parametrize("P", [0, 1, 3])
@pytest.mark.parametrize("pair", [(F16, F32), (F32, BF16), (BF16, F16)], ids=["F16-F32", "F32-BF16", "BF16-F16"])
def test_extract_cached_convert(ops, pair, P):
    """Hits from P shards (0: one array), misses from a pinned host table; the miss count equals the plain call's."""
    src_dt, dst_dt = pair
    N, dim, n, num_cached = 500, 20, 300, 200
    bits = table_bits(src_dt, (N, dim), seed=11)
    rank, tab = _cache_layout(N, num_cached, 5)
    np_parts = [bits[rank[:num_cached]][p::max(P, 1)] for p in range(max(P, 1))]
    parts = [dev_bits(np.ascontiguousarray(x), src_dt) for x in np_parts]
    ptab = ops.part_pointer_table(parts)
    host = torch.from_numpy(bits.view(np.int32 if src_dt == F32 else np.int16)).pin_memory()
    nodes = np.random.RandomState(9).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = sentinel_out(n, dim, dst_dt)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out, TORCH[src_dt], t_nodes, t_tab, ptab, P, host, num_miss=miss)
    assert_same_bits(tensor_bits(out, dst_dt), convert_bits(bits[nodes], src_dt, dst_dt), dst_dt)
    plain = torch.empty((n, dim), dtype=TORCH[src_dt], device="cuda")
    miss_plain = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached(plain, t_nodes, t_tab, ptab, P, host, num_miss=miss_plain)
    assert int(miss.item()) == int(miss_plain.item()) == int((tab[nodes] == ALL_ONES).sum())
    assert tensor_bits(plain, src_dt).tobytes() == bits[nodes].tobytes()


@pytest.mark.parametrize("P", [0, 3])
def test_extract_cached_convert_full_cache_in_node_order(ops, P):
    """table == NULL: slot = node id, no miss tier."""
    src_dt, dst_dt = F16, F32
    N, dim, n = 500, 20, 300
    bits = table_bits(src_dt, (N, dim), seed=12)
    parts = [dev_bits(np.ascontiguousarray(bits[p::max(P, 1)]), src_dt) for p in range(max(P, 1))]
    nodes = np.random.RandomState(2).randint(0, N, n).astype(np.uint32)
    out = sentinel_out(n, dim, dst_dt)
    miss = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out, TORCH[src_dt], ids(nodes), None, ops.part_pointer_table(parts), P, None, num_miss=miss)
    assert_same_bits(tensor_bits(out, dst_dt), convert_bits(bits[nodes], src_dt, dst_dt), dst_dt)
    assert int(miss.item()) == 0


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("pair", [(F16, F32), (F32, F16)], ids=["F16-F32", "F32-F16"])
def test_extract_tiered_convert(ops, pair, P):
    """Replica + P shards + host rows behind a host_row_mask; the four tier counters equal the plain call's."""
    src_dt, dst_dt = pair
    N, dim, n, num_cached, R, me, mask = 512, 20, 300, 260, 40, P - 1, 255
    bits = table_bits(src_dt, (N, dim), seed=13)
    rank, tab = _cache_layout(N, num_cached, 6)
    replica = dev_bits(np.ascontiguousarray(bits[rank[:R]]), src_dt)
    parts = [dev_bits(np.ascontiguousarray(bits[rank[R + p:num_cached:P]]), src_dt) for p in range(P)]
    ptab = ops.part_pointer_table(parts)
    host = torch.from_numpy(bits.view(np.int32 if src_dt == F32 else np.int16)).pin_memory()
    nodes = np.random.RandomState(4).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = sentinel_out(n, dim, dst_dt)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.extract_tiered_convert(out, TORCH[src_dt], t_nodes, t_tab, replica, ptab, P, me, host, tier_rows=counters,
                               host_row_mask=mask)
    missed = tab[nodes] == ALL_ONES
    rows = np.where(missed, nodes & mask, nodes)  # a host row is node & mask; every other tier holds the node's own row
    assert_same_bits(tensor_bits(out, dst_dt), convert_bits(bits[rows], src_dt, dst_dt), dst_dt)
    # the plain call on the same inputs (its wrapper takes no mask: the struct is filled here)
    from xgnn_amd import lib
    t = ops._feature_tiers(t_tab, replica, ptab, P, me, host, mask)
    plain = torch.empty((n, dim), dtype=TORCH[src_dt], device="cuda")
    counters_plain = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = lib().ggms_extract_tiered(plain.data_ptr(), t_nodes.data_ptr(), n, None, C.byref(t), dim,
                                   ops.DTYPE_CODE[TORCH[src_dt]], counters_plain.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    slots = tab[nodes].astype(np.int64)
    shard = (slots - R) % P
    hit = ~missed
    want = [int(missed.sum()), int((hit & (slots >= R) & (shard != me)).sum()),
            int((hit & (slots >= R) & (shard == me)).sum()), int((hit & (slots < R)).sum())]
    assert counters.cpu().tolist() == counters_plain.cpu().tolist() == want and sum(want) == n
    assert tensor_bits(plain, src_dt).tobytes() == bits[rows].tobytes()


def test_invalid_arguments_launch_nothing(ops):
    from xgnn_amd import lib
    h = lib()
    out = sentinel_out(8, 4, F32)
    src = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    U8, I64 = 3, 6

    def call(o, dim, src_dt, dst_dt):
        return h.ggms_gather_scatter_convert(o, src.data_ptr(), index.data_ptr(), None, 8, None, dim, src_dt, dst_dt,
                                             ALL_ONES, s)
    for args, word in [((out.data_ptr(), 4, F32, U8), b"conversion"), ((out.data_ptr(), 4, I64, F32), b"conversion"),
                       ((out.data_ptr(), 0, F16, F32), b"invalid argument"), ((None, 4, F16, F32), b"invalid argument"),
                       ((out.data_ptr(), 4, F16, 8), b"invalid argument")]:
        assert call(*args) == -1, args
        assert word in h.ggms_last_error(), (args, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         U8, None, s) == -1
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 9, None, 4, F32,
                                         F16, None, s) == -1  # too many parts
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, I64, F32, None,
                                         s) == -1
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, None, 4, F16, F32, None, s) == -1
    torch.cuda.synchronize()
    assert (tensor_bits(out, F32) == SENTINEL).all()


def test_same_dtype_is_the_plain_gather(ops):
    """(F32, F32): byte-identical to ggms_gather_scatter_masked; the same holds for a dtype that never converts."""
    from xgnn_amd import lib
    n, dim = 1000, 100
    bits, t_src = table(F32, 2048, dim)
    index = np.random.RandomState(1).randint(0, 1 << 31, n).astype(np.uint32)
    t_index = ids(index)
    out = sentinel_out(n, dim, F32)
    ops.gather_scatter_convert(out, t_src, t_index, None, src_row_mask=1023)
    ref = sentinel_out(n, dim, F32)
    rc = lib().ggms_gather_scatter_masked(ref.data_ptr(), t_src.data_ptr(), t_index.data_ptr(), None, n, None, dim, F32,
                                          1023, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert tensor_bits(out, F32).tobytes() == tensor_bits(ref, F32).tobytes() == bits[index & 1023].tobytes()
    bytes_src = torch.arange(64 * 10, dtype=torch.uint8, device="cuda").view(64, 10)
    got = torch.zeros((5, 10), dtype=torch.uint8, device="cuda")
    ops.gather_scatter_convert(got, bytes_src, ids([3, 1, 63, 0, 3]), None)
    assert torch.equal(got, bytes_src[[3, 1, 63, 0, 3]])
