"""What the converting-gather tests of every source family share (test_gpu_feat_convert.py, test_gpu_fp8_gather.py,
test_gpu_q8row_gather.py): the table on the device, the output between canaries, the index plan of one
ggms_gather_scatter_convert call, and the cached / full-cache / tiered calls with their plain twins.  What a call must deliver is the family's statement (feat_formats.Table); what an
output is judged by is feat_formats.check_output."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_formats import ALL_ONES, Q8ROW, TORCH, TORCH_BITS, U8, check_output, pair_id, sentinel, tensor_bits

CANARY = 64  # elements kept on either side of every output


def pairs(fam, *which, ids=None):
    """Parametrises a test over (source, output) pairs: `which`, or all the family's."""
    which = which or fam.pairs
    return pytest.mark.parametrize("pair", which, ids=ids or [pair_id(p) for p in which])


def ids(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def to_device(stored, fmt, offset=0):
    """A device tensor of dtype TORCH[fmt] holding the stored rows, its base `offset` bytes past a 256-byte boundary."""
    b = np.ascontiguousarray(stored).view(np.uint8)
    flat = torch.empty(b.size + 256, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    t = flat[offset:offset + b.size]
    t.copy_(torch.from_numpy(np.array(b).ravel()))  # (a copy: the tables are read-only)
    return t.view(b.shape).view(TORCH[fmt])


def _pinned(stored):
    return torch.from_numpy(np.array(stored).view(np.uint8)).pin_memory()


class Out:
    """`rows x dim` output of dtype `dt` inside a sentinel-filled buffer: CANARY elements in front (+ `shift`, which
    misaligns the output) and behind."""

    def __init__(self, rows, dim, dt, shift=0):
        self.dt, self.shape, self.lead = dt, (rows, dim), CANARY + shift
        self.flat = torch.empty(self.lead + rows * dim + CANARY, dtype=TORCH[dt], device="cuda")
        self.flat.view(TORCH_BITS[dt]).fill_(sentinel(dt))
        self.t = self.flat[self.lead:self.lead + rows * dim].view(rows, dim)

    def untouched(self):
        return bool((tensor_bits(self.flat, self.dt) == sentinel(self.dt)).all())

    def check(self, dst_rows, table, src_rows, what):
        """Rows `dst_rows` hold rows `src_rows` of `table` as its format decodes into this dtype; nothing else was
        written."""
        check_output(tensor_bits(self.flat, self.dt), self.dt, self.lead, self.shape, dst_rows,
                     table.want(self.dt, src_rows), table.nan(src_rows), what, table.code_of(src_rows))


_DEVICE = {}


def shared_table(fam, fmt, rows, dim, offset=0):
    """(the family's shared gather table, the same on the device): made once per shape and never written."""
    t = fam.table(fmt, rows, dim)
    if (id(t), offset) not in _DEVICE:
        _DEVICE[(id(t), offset)] = to_device(t.stored, fmt, offset)
    return t, _DEVICE[(id(t), offset)]


def gather_case(ops, fam, fmt, out_dt, dim, n, scatter=False, dev_count=False, mask=ALL_ONES, rows=None, offset=0, shift=0,
                what=""):
    """One ggms_gather_scatter_convert call, checked.  The index starts with the family's head rows (those that
    enumerate every code and hold the rounding edges), continues with random rows (repeats included) and ends by
    repeating its first entries; under a row mask every entry gets random bits above the mask.  Counts that are no
    multiple of 64 end in a partial tile."""
    rows = fam.rows if rows is None else rows
    t, t_src = shared_table(fam, fmt, rows, dim, offset)
    rs = np.random.RandomState(n + 7 * dim)
    n_max = n + 37 if dev_count else n  # device count below the bound: the rows past it stay untouched
    index = np.concatenate([np.arange(min(rows, fam.head)), rs.randint(0, rows, n_max)])[:n_max].astype(np.uint32)
    k = fam.tail(n_max)
    index[n_max - k:] = index[:k]  # repeats (the random part repeats rows as well)
    if mask != ALL_ONES:
        index = (index.astype(np.uint64) + rs.randint(0, 1 << 20, n_max).astype(np.uint64) * (mask + 1)).astype(np.uint32)
    out_rows = n_max + 50 if scatter else n_max
    dst = rs.permutation(out_rows)[:n_max].astype(np.uint32) if scatter else np.arange(n_max, dtype=np.uint32)
    out = Out(max(out_rows, 1), dim, out_dt, shift)
    num_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if dev_count else None
    ops.gather_scatter_convert(out.t, t_src, ids(index) if n_max else torch.empty(0, dtype=torch.int32, device="cuda"),
                               ids(dst) if scatter else None, num=n_max, num_dev=num_dev, src_row_mask=mask, src_dtype=fmt)
    out.check(dst[:n], t, index[:n] & np.uint32(mask), f"{what} dim={dim} n={n} scatter={scatter} dev_count={dev_count} "
              f"mask={mask:#x} offset={offset} shift={shift}")


def main_calls(ops, fam, pair, dim):
    """Every (n, dst_index scatter, count on the device, row mask) of the family at one row shape."""
    for n, scatter, dev_count, mask in fam.calls:
        gather_case(ops, fam, *pair, dim, n, scatter=scatter, dev_count=dev_count, mask=mask)


def long_row_calls(ops, fam, pair, dim):
    """launch_chunks (xgnn_amd/csrc/extract.hip): rows of 8192 chunks and more go to k_gather_long_rows (one workgroup
    per row), shorter ones to the tile sweep of k_gather_rows."""
    for scatter, dev_count in fam.long_calls:
        gather_case(ops, fam, *pair, dim, fam.long_n, scatter=scatter, dev_count=dev_count, rows=8)


def table_offset_calls(ops, fam, pair, offset):
    for dim, n, scatter in fam.offset_calls:
        gather_case(ops, fam, *pair, dim, n, scatter=scatter, offset=offset, what="table offset")


def shifted_out_calls(ops, fam, pair):
    """`out` fam.shift elements past an aligned base: only chunks of that many elements are aligned on the output side."""
    for dim, n, scatter, dev_count in fam.shifted:
        gather_case(ops, fam, *pair, dim, n, scatter=scatter, dev_count=dev_count, shift=fam.shift, what="out offset")


def _cache_layout(N, num_cached, seed):
    """(nodes by rank, node -> cache slot or ALL_ONES): the first num_cached nodes of a random ranking are cached."""
    rank = np.random.RandomState(seed).permutation(N)
    tab = np.full(N, ALL_ONES, np.uint32)
    tab[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    return rank, tab


def _plain_out(t, n):
    """An output for the plain (non-converting) twin of a call: n stored rows, and the dtype code they move as."""
    cols = t.stored.shape[1]
    return torch.empty((n, cols), dtype=TORCH[t.fmt], device="cuda"), cols, U8 if t.fmt == Q8ROW else t.fmt


def _parts(rows, t, P):
    return [to_device(np.ascontiguousarray(rows[p::max(P, 1)]).reshape(-1, t.stored.shape[1]), t.fmt) for p in range(max(P, 1))]


def cached_case(ops, t, out_dt, frac, P, n=300):
    """ggms_extract_cached_convert: hits from P shards (0: one array) of stored rows, misses from the pinned host table;
    the miss count equals the plain call's, whose rows are the stored bytes."""
    N, b = t.stored.shape[0], t.stored
    num_cached = int(N * frac)
    rank, tab = _cache_layout(N, num_cached, 5)
    ptab = ops.part_pointer_table(_parts(b[rank[:num_cached]], t, P))
    host = _pinned(b)
    nodes = np.random.RandomState(9).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, t.dim, out_dt)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, t.fmt, t_nodes, t_tab, ptab, P, host, num_miss=miss)
    out.check(np.arange(n), t, nodes, f"cached frac={frac} P={P}")
    plain, _, _ = _plain_out(t, n)
    miss_plain = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_cached(plain, t_nodes, t_tab, ptab, P, host, num_miss=miss_plain)
    assert int(miss.item()) == int(miss_plain.item()) == int((tab[nodes] == ALL_ONES).sum())
    assert plain.view(torch.uint8).cpu().numpy().tobytes() == b[nodes].tobytes()


def full_cache_case(ops, t, out_dt, P, n=300):
    """ggms_extract_cached_convert with table == NULL: slot = node id, no miss tier."""
    nodes = np.random.RandomState(2).randint(0, t.stored.shape[0], n).astype(np.uint32)
    out = Out(n, t.dim, out_dt)
    miss = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    ops.extract_cached_convert(out.t, t.fmt, ids(nodes), None, ops.part_pointer_table(_parts(t.stored, t, P)), P, None,
                               num_miss=miss)
    out.check(np.arange(n), t, nodes, f"full cache P={P}")
    assert int(miss.item()) == 0


def tiered_case(ops, t, out_dt, P, host_mask=0, n=300, num_cached=260, R=40):
    """ggms_extract_tiered_convert: replica + P shards + host rows (behind host_row_mask, where the family sets one); the
    four tier counters equal those of the plain call on the same tiers, whose rows are the stored bytes."""
    from xgnn_amd import lib
    N, b, me = t.stored.shape[0], t.stored, P - 1
    rank, tab = _cache_layout(N, num_cached, 6)
    replica = to_device(np.ascontiguousarray(b[rank[:R]]), t.fmt)
    parts = [to_device(np.ascontiguousarray(b[rank[R + p:num_cached:P]]), t.fmt) for p in range(P)]
    ptab = ops.part_pointer_table(parts)
    host = _pinned(b)
    nodes = np.random.RandomState(4).randint(0, N, n).astype(np.uint32)
    t_nodes, t_tab = ids(nodes), ids(tab)
    out = Out(n, t.dim, out_dt)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.extract_tiered_convert(out.t, t.fmt, t_nodes, t_tab, replica, ptab, P, me, host, tier_rows=counters,
                               host_row_mask=host_mask)
    missed = tab[nodes] == ALL_ONES
    # a host row is node & mask; every other tier holds the node's own row
    rows = np.where(missed, nodes & host_mask, nodes) if host_mask else nodes
    out.check(np.arange(n), t, rows, f"tiered P={P}")
    # the plain call on the same inputs (its wrapper takes no mask: the struct is filled here)
    tiers = ops._feature_tiers(t_tab, replica, ptab, P, me, host, host_mask)
    plain, cols, code = _plain_out(t, n)
    counters_plain = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = lib().ggms_extract_tiered(plain.data_ptr(), t_nodes.data_ptr(), n, None, C.byref(tiers), cols, code,
                                   counters_plain.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    slots = tab[nodes].astype(np.int64)
    shard, hit = (slots - R) % P, ~missed
    want = [int(missed.sum()), int((hit & (slots >= R) & (shard != me)).sum()),
            int((hit & (slots >= R) & (shard == me)).sum()), int((hit & (slots < R)).sum())]
    assert counters.cpu().tolist() == counters_plain.cpu().tolist() == want and sum(want) == n
    assert plain.view(torch.uint8).cpu().numpy().tobytes() == b[rows].tobytes()
